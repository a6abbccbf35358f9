"""SfMPipeline.reconstruct_from_features on the device against the same driver over the restatements
(tests/sfm_pipeline_restatement.py) on the planted scenes of tests/sfm_chain_inputs.py: the records of what crosses every
boundary -- the selection scores, the correspondences, the registrations, the new points, the rows and states of every
bundle adjustment, the drops -- are compared bit for bit, via sfm_chain.first_difference.

The scenes' keypoints and the matches that the chain of tests/sfm_chain.py verified are fed directly (matches= bypasses the
descriptor matching), so the F-RANSACs of the chain are not computed again, and the restatement pipeline shares the chain's
memo of identical calls; its host share is 6 to 9 s a scene, once per process, as the chain's.

The precondition of tests/test_hip_sfm_chain.py is kept: the device takes log from the C library, so no stop of a RANSAC of
the pipeline may be decided within 2 of the end of a batch.  That is a condition on the inputs, not a tolerance; the scenes
meet it under the correspondence order of include/amvs_sfm.h as they are (asserted below)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_chain as ch  # noqa: E402
import sfm_chain_inputs as ci  # noqa: E402
import sfm_pipeline_restatement as pr  # noqa: E402
from sfm_chain import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
BATCH_ENDS = (1024, 2048, 3072, 4096, 5000)


@pytest.fixture(scope="module")
def pipeline():
    import amvs
    from amvs.core.camera import Camera
    with amvs.Engine(8, 8, 1, np.eye(3, dtype=np.float32)) as e:
        yield amvs.SfMPipeline(Camera(ci.K), engine=e)


def restated(name):
    sc, matches, rec, ops = pr.restated(name)
    assert all(min(abs(N - k) for k in BATCH_ENDS) >= 2 for _, N in ops.log_decided)
    return sc, matches, rec


def on_the_device(pipeline, sc, matches):
    rec = {}
    points, colors, poses = pipeline.reconstruct_from_features(sc["keypoints"], matches=matches, record=rec)
    return rec, points, colors, poses


@pytest.mark.parametrize("name", ["noisy", "edges"])
def test_every_boundary_bit_for_bit(pipeline, name):
    sc, matches, want = restated(name)
    got, points, colors, poses = on_the_device(pipeline, sc, matches)
    where = ch.first_difference(got, want, same=same_bits)
    assert where is None, f"{name}: the pipeline's record first differs from the restatement's at {where}"
    assert got["registered"] == want["registered"] and sorted(poses) == list(range(7 if name == "edges" else 6))
    assert len(got["bundles"]) == (3 if name == "edges" else 2) and got["final"]["failed"] == []
    # what the caller gets: the live points, normalised as the reference does it
    assert points.shape == (len(got["final"]["ids"]), 3) and colors.shape == points.shape and (colors == 127).all()
    assert np.abs(np.median(points, axis=0)).max() < 1e-9
    assert abs(np.percentile(np.linalg.norm(points, axis=1), 90) - 10.0) < 1e-9


def test_the_same_scene_twice_on_one_pipeline(pipeline):
    sc, matches, _ = restated("noisy")
    first = on_the_device(pipeline, sc, matches)
    edges = restated("edges")
    on_the_device(pipeline, edges[0], edges[1])                              # another scene in between
    second = on_the_device(pipeline, sc, matches)
    where = ch.first_difference(second[0], first[0], same=same_bits)
    assert where is None, f"the second run first differs from the first at {where}"
    assert same_bits(first[1], second[1])


def test_more_views_than_a_bundle_adjustment_takes_are_refused_up_front(pipeline):
    with pytest.raises(ValueError):
        pipeline.reconstruct_from_features([np.zeros((0, 2), np.float32)] * 257, matches={(0, 1): np.zeros((0, 2), np.int32)})


def planted_features(sc, seed=5, noise=6):
    """One 128-d uint8 descriptor per planted track plus uniform noise of +-`noise` per entry; a keypoint of no track gets a
    descriptor of its own."""
    from amvs.core import ImageFeatures
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 236, (int(max(t.max() for t in sc["track"])) + 1, 128))
    feats = []
    for kp, track in zip(sc["keypoints"], sc["track"]):
        d = np.where((track >= 0)[:, None], base[np.maximum(track, 0)], rng.integers(20, 236, (len(track), 128)))
        d = np.clip(d + rng.integers(-noise, noise + 1, d.shape), 0, 255).astype(np.uint8)
        feats.append(ImageFeatures(kp, d, (1080, 1920)))
    return feats


def test_end_to_end_with_descriptors(pipeline):
    """Descriptor matching, verification, and the reconstruction, on the six views of `noisy` with planted descriptors: the
    matcher pairs the keypoints of one track, all 15 pairs come out with 1 193 rows in all, and the planted false matches of the
    scene are gone.  Measured on the restatement pipeline (tests/sfm_pipeline_restatement.py) run on exactly those matches:
    rotation 0.175 degrees, centre 0.0201 and point 0.0483 baselines, RMS 1.06 px, 160 points compared, none mixed (more
    observations a point than on the scene's own matches, and the initial pair another: hence other numbers than there).
    Asserted: ten times each, all six views registered, at least 120 planted points compared, none mixed."""
    sc = ci.scene("noisy")
    feats = planted_features(sc)
    rec = {}
    matches = pipeline.match_image_pairs(feats, window_size=6)
    assert len(matches) >= 10 and all(len(m) >= 15 for m in matches.values())
    images = [np.full((900, 1920, 3), (10 * v + 5, 10 * v + 6, 10 * v + 7), np.uint8) for v in range(6)]       # BGR, one colour a view; the
    # scene's pictures are 1920 x 1080: cut to 900 rows, 7 of the 160 first observations fall outside
    points, colors, poses = pipeline.reconstruct_from_features(feats, images=images, record=rec)
    assert sorted(poses) == list(range(6)) and rec["final"]["failed"] == []
    # a point has the colour of its first observation's view at that pixel, as RGB; outside the image it keeps 127
    rows = rec["final"]["observations"]
    first = rows[np.unique(rows[:, 1], return_index=True)[1]]
    inside = (np.rint(first[:, 2]) >= 0) & (np.rint(first[:, 2]) < 1920) & (np.rint(first[:, 3]) >= 0) & (np.rint(first[:, 3]) < 900)
    want = np.where(inside[:, None], (10 * first[:, :1] + [7, 6, 5]).astype(np.uint8), np.uint8(127))
    assert np.array_equal(rec["final"]["ids"], first[:, 1].astype(np.int64)) and np.array_equal(colors, want) and inside.sum() == 153 and len(inside) == 160
    at = [{(float(u), float(v)): k for k, (u, v) in enumerate(kp)} for kp in sc["keypoints"]]
    obs = {}
    for v, p, x, y in rec["final"]["observations"]:
        obs.setdefault(int(p), {})[int(v)] = at[int(v)][(float(np.float32(x)), float(np.float32(y)))]
    e = ch.truth_errors(sc, dict(rec, observations=obs))
    print(f"end to end: rotation {e['rotation']:.3g} degrees, centre {e['centre']:.3g}, point {e['point']:.3g} baselines, "
          f"rms {e['rms']:.3g} px, {len(e['compared'])} points compared, {len(matches)} pairs")
    assert e["rotation"] < 1.75 and e["centre"] < 0.201 and e["point"] < 0.483 and e["rms"] < 10.6
    assert e["mixed"] == [] and len(e["compared"]) >= 120

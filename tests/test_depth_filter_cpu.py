"""The cross-view depth-map filter without a GPU: the restatement of tests/depth_filter_restatement.py against itself
(loops against the NumPy twin), the input family of tests/depth_filter_inputs.py against the coverage the GPU comparison
relies on, the properties and the accuracy of the definition on a scene with known depths, and the host-only pieces of
the feature (the second header and its binding table, the neighbour rows, the new keywords).
tests/test_hip_depth_filter.py compares the device with the same restatement."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_filter_inputs as fi  # noqa: E402
import depth_filter_restatement as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured by the restatement on make_scene(5, 48, 64) with relative noise 0.002, 5 % outliers 5 to 40 % off and 3 % of the
# pixels below the confidence (depth_filter_inputs.scene_maps, seed 31; max_px 1, max_rel 0.01, min_consistent 2, every
# other map as neighbour); seeds 32 to 34 give 0 surviving outliers, 0.1003 to 0.1032 inliers lost and 1.219e-3 to
# 1.235e-3:
#     outliers surviving        0 of 748      inliers lost (mostly at the image borders, where fewer than two other
#     views see the point)   0.1000          relative RMS depth error of the kept inliers   2.000e-3 before, 1.219e-3 after
# Gates: the measured value plus 25 % towards the bad side, for another noise seed.  A margin on a measured zero is zero and
# a single coincidence would break it, so the outliers get the bound 1 in 100 instead: an outlier is at least 5 % off and
# max_rel is 1 %, so it survives only if two other views hold outliers that agree with it.
OUTLIERS_SURVIVING_MAX = 0.01
INLIERS_LOST_MAX = 0.1000 * 1.25
RMS_AFTER_MAX = 1.219e-3 * 1.25


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_RESTATED = {}


def restated(case, refine=True):
    """(depth, count, (valid, kept), counters) of the case by the twin, computed once."""
    key = (case.name, refine)
    if key not in _RESTATED:
        _RESTATED[key] = fr.depth_filter_np(*case.args(refine=refine))
    return _RESTATED[key]


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("case", fi.small_family(), ids=lambda c: c.name)
def test_loops_and_twin_agree_bit_for_bit(case, refine):
    want = restated(case, refine)
    got = fr.depth_filter(*case.args(refine=refine))
    assert same(got, want)
    assert got[3] == want[3], "the counters of the two forms differ"


def test_family_reaches_every_guard_and_edge():
    """What keeps the GPU comparison from silently leaving a case out: every counter of the restatement reaches 20 over the
    inputs the GPU comparison runs (the whole family), the two exact ties at least once, and an input built for an edge
    reaches it on its own."""
    total = dict.fromkeys(fr.COUNTERS, 0)
    for case in fi.family():
        own = restated(case)[3]
        for edge in case.edges:
            assert own[edge] >= 1, f"{case.name} was built for {edge} and does not reach it"
        for k, v in own.items():
            total[k] += v
    print(total)
    assert all(v >= (1 if k in fr.TIE_COUNTERS else 20) for k, v in total.items()), total
    shapes = {c.shape for c in fi.family()}
    assert (2, 2) in shapes and {len(c.poses) for c in fi.family()} >= {1, 2, 3, 5}
    assert max(c.depth.size for c in fi.small_family()) <= 5 * 48 * 64
    big = [c for c in fi.family() if c.big]
    assert len(big) == 1 and big[0].shape[0] * big[0].shape[1] > 256 * 256 and len(big[0].poses) == 2


def test_exact_ties_are_exact():
    """The constructed ties: every pixel pair of depth_ties meets fabs(Y_2 - d) == max_rel * d, every in-image pair of e2_tie
    meets e2 == max_px^2, and both count as consistent; one float32 step further they fail."""
    c = restated(fi.by_name("depth_ties"))[3]
    assert c["depth_tie"] == 96 and c["depth_fail"] == 96 and c["e2_fail"] == 0
    c = restated(fi.by_name("e2_tie"))[3]
    assert c["e2_tie"] > 0 and c["e2_fail"] == 0 and c["consistent"] >= c["e2_tie"]
    f = restated(fi.by_name("e2_fail"))[3]
    assert f["e2_fail"] == c["e2_tie"] and f["e2_tie"] == 0


@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_family_tells_every_near_miss_from_the_definition(variant):
    """On the inputs the GPU comparison runs.  The loops take the same variant: on the inputs without a scene they are held
    to the twin's near-miss bit for bit, so that neither form's variant code goes unrun."""
    differing = []
    for case in fi.family():
        got = fr.depth_filter_np(*case.args(), variant=variant)
        if not same(got, restated(case)):
            differing.append(case.name)
        if not case.big and not case.name.startswith("scene_"):
            loops = fr.depth_filter(*case.args(), variant=variant)
            assert same(loops, got), f"{case.name}: the loops' {variant}"
    print(variant, differing)
    assert differing, f"no input of the family tells {variant} from the definition"


def test_unknown_variant_is_refused():
    case = fi.by_name("tiny_2x2")
    with pytest.raises(ValueError):
        fr.depth_filter_np(*case.args(), variant="no_such_variant")
    with pytest.raises(ValueError):
        fr.depth_filter(*case.args(), variant="no_such_variant")


# ------------------------------------------------------------------------------------------------ properties ---
@pytest.mark.parametrize("case", fi.family(), ids=lambda c: c.name)
def test_properties_of_the_definition(case):
    depth, count, (n_valid, n_kept), _ = restated(case)
    plain, plain_count, plain_counts, _ = restated(case, refine=False)
    # refine = 0 returns input depths or 0, and keeps what refine = 1 keeps
    kept = plain != 0
    assert np.array_equal(bits(plain)[kept], bits(case.depth)[kept]) and not plain[~kept].any()
    assert np.array_equal(kept, depth != 0) and np.array_equal(count, plain_count) and plain_counts == (n_valid, n_kept)
    assert n_kept == int(kept.sum()) and n_valid >= n_kept
    # a kept refined depth lies within [d (1 - max_rel), d (1 + max_rel)] up to one float32 rounding
    d = case.depth.astype(np.float64)[kept]
    rel = float(np.float32(case.max_rel))
    lo, hi = (d * (1.0 - rel)).astype(np.float32), (d * (1.0 + rel)).astype(np.float32)
    assert np.all(depth[kept] >= np.nextafter(lo, np.float32(0))) and np.all(depth[kept] <= np.nextafter(hi, np.float32(np.inf)))
    # counts are whole numbers between 0 and the row's neighbour number, and 0 at invalid pixels
    rows = fr.neighbour_rows(len(case.poses), case.neighbours)
    for j, row in enumerate(rows):
        assert count[j].min() >= 0 and count[j].max() <= sum(i >= 0 for i in row)
    assert np.array_equal(count, np.floor(count))
    valid = (case.depth > 0) & (case.depth <= np.finfo(np.float32).max) & (case.conf >= np.float32(case.min_confidence))
    assert not count[~valid].any() and n_valid == int(valid.sum())
    assert np.all(count[kept] >= case.min_consistent) and np.all(count[valid & ~kept] < case.min_consistent)


@pytest.mark.parametrize("name", ["shifted_views", "scene_5_views", "scene_ragged_rows"])
def test_raising_min_consistent_only_removes_pixels(name):
    case = fi.by_name(name)
    before = None
    for m in (1, 2, 3, 4, 5):
        depth, count, (_, n_kept), _ = fr.depth_filter_np(*case.args(min_consistent=m))
        kept = depth != 0
        if before is not None:
            assert not (kept & ~before[0]).any() and n_kept <= before[1]
            assert np.array_equal(bits(depth)[kept], bits(before[2])[kept]) and np.array_equal(count, before[3])
        before = (kept, n_kept, depth, count)
    assert before[1] == 0                        # (no row has five neighbours)


def test_accuracy_on_the_scene():
    case = fi.by_name("scene_5_views")
    truth, outlier = case.extra["truth"], case.extra["outlier"]
    depth = restated(case)[0]
    valid = case.conf >= np.float32(case.min_confidence)
    kept = depth != 0
    surviving = (kept & outlier & valid).sum() / (outlier & valid).sum()
    inlier = valid & ~outlier
    lost = 1.0 - (kept & inlier).sum() / inlier.sum()
    sel = kept & inlier
    rms_before = np.sqrt(np.mean((case.depth.astype(np.float64)[sel] / truth[sel] - 1.0) ** 2))
    rms_after = np.sqrt(np.mean((depth.astype(np.float64)[sel] / truth[sel] - 1.0) ** 2))
    print(f"outliers surviving {surviving:.4f} ({int((outlier & valid).sum())} planted), inliers lost {lost:.4f}, relative RMS depth "
          f"error of the kept inliers {rms_before:.3e} before, {rms_after:.3e} after")
    assert surviving <= OUTLIERS_SURVIVING_MAX
    assert lost <= INLIERS_LOST_MAX
    assert rms_after <= RMS_AFTER_MAX and rms_after < rms_before


# -------------------------------------------------------------------------------- symbols, rows and keywords ---
def test_second_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_depth.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(amvs_\w+)\(", header, re.M))
    assert declared == set(_lib.DEPTH_SIGNATURES) == {"amvs_depth_filter"}
    assert not declared & set(_lib.SIGNATURES)
    assert '#include "amvs.h"' in header
    lib = _lib.load()
    for name, (res, args) in _lib.DEPTH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the declaration's parameter count is the table's
    decl = re.search(r"^int amvs_depth_filter\((.*?)\);", header, re.M | re.S).group(1)
    assert len(decl.split(",")) == len(_lib.DEPTH_SIGNATURES["amvs_depth_filter"][1]) == 19
    from amvs.engine import Engine
    assert callable(Engine.depth_filter)


def test_parameter_errors_need_no_device():
    """A NULL context is refused before anything else happens, whatever the other arguments."""
    from amvs import _lib
    lib = _lib.load()
    cnt = (C.c_int64 * 2)()
    K = (C.c_double * 12)()
    assert lib.amvs_depth_filter(None, 1, None, None, 0, K, K, K, None, 0, 1.0, 1.0, 0.01, 1, 1, None, None, 0, cnt) == -1
    assert lib.amvs_depth_filter(None, 0, None, None, 7, None, None, None, None, -1, 1.0, -1.0, 0.0, 0, 1, None, None, 9, None) == -1


def test_neighbour_rows_follow_the_stereo_class():
    """nearest_map_neighbours: the rule and the stable order of DenseStereoReconstructor._find_neighbors."""
    import amvs
    from amvs.core.camera import CameraPose
    from amvs.core.dense_stereo import DenseStereoReconstructor
    from amvs.core.utils import nearest_map_neighbours
    rng = np.random.default_rng(41)
    centers = rng.normal(0, 2, (7, 3))
    centers[5] = 2 * centers[0] - centers[3]                     # (a tie: 3 and 5 are equally far from 0)
    poses = {i: CameraPose(R=np.eye(3), t=-centers[i]) for i in range(7)}
    ds = DenseStereoReconstructor(amvs.Camera(K=np.eye(3), dist=np.zeros(5)), device=0)
    for k in (1, 3, 6, 9):
        rows = nearest_map_neighbours(centers, k)
        assert rows.dtype == np.int32 and rows.shape == (7, min(k, 6))
        for j in range(7):
            assert list(rows[j]) == ds._find_neighbors(j, list(range(7)), poses, k=k)
    assert nearest_map_neighbours(centers, None) is None and nearest_map_neighbours(centers[:1], 3) is None
    with pytest.raises(ValueError):
        nearest_map_neighbours(centers, 0)


def test_keywords_are_there_and_off_by_default():
    from amvs.core.dense_stereo import DenseStereoReconstructor
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    want = dict(geometric_filter=False, filter_px=1.0, filter_min_views=2, filter_refine=True, filter_neighbours=None)
    for fn, rel in ((PatchMatchMVS.reconstruct, 0.01), (PatchMatchMVS.reconstruct_mesh, 0.01), (DenseStereoReconstructor.reconstruct, None)):
        params = inspect.signature(fn).parameters
        for name, default in dict(want, filter_rel=rel).items():
            assert params[name].default == default and params[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, name)


def test_stereo_default_filter_rel_covers_a_plane_spacing():
    from amvs.core.dense_stereo import DenseStereoReconstructor
    depths = 1.0 / np.linspace(1 / 8.0, 1 / 0.5, 64)                # (the class's plane list, far to near)
    rel = DenseStereoReconstructor.plane_spacing(depths)
    steps = np.abs(np.diff(depths)) / np.minimum(depths[:-1], depths[1:])
    assert rel == steps.max() and np.all(steps <= rel) and rel == steps[0]

"""Hole filling (amvs_tsdf_fill) without a GPU: the vectorised restatement (tests/mesh_fill_restatement.py) against its
plain-loop statement on every small case, what the family of tests/mesh_fill_inputs.py reaches, the named near-misses,
the properties the header promises, and the scenes with an analytic truth (DESIGN.md section 8 "Hole filling").

These tests pin the restatement and the family, not the device code: all but the last two run NumPy alone and would pass
without the library's fill.  What holds the kernel to the restatement is tests/test_hip_mesh_fill.py, on the GPU; the last
two here (reconstruct_mesh's argument checks, the ABI's two names) need the feature and fail without it."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_fill_inputs as fi  # noqa: E402
import mesh_fill_restatement as fr  # noqa: E402
import mesh_restatement as mr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
LAST = max(fi.STEPS)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_volume(a, b):
    """tsdf, weight and colour sums bit for bit (garbage behind unobserved points included: nobody writes it)."""
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:3], b[:3]))


@functools.lru_cache(maxsize=None)
def _family():
    return fi.family()


@functools.lru_cache(maxsize=None)
def _loop(index, min_neighbours):
    """fill_loop of member `index` at the largest step count, with the statistics of its walk."""
    stats = {}
    out = fr.fill_loop(*_family()[index][1].arrays()[:3], LAST, min_neighbours, stats=stats)
    return out, stats


def test_the_family_is_what_the_issue_lists():
    names = [n for n, _ in _family()]
    assert len(names) == len(set(names)) == 3 * len(mv.RANDOM_SIGN_SHAPES) + 5
    first = fr.fill(*_family()[0][1].arrays()[:3], LAST)
    assert first[4] == [1852, 1, 0, 0, 0]                              # the 25 % family fills in one step
    big = fi.large_sphere()
    assert big.dims == (160, 160, 160) and (160 ** 3 + 255) // 256 == 16000


@pytest.mark.parametrize("min_neighbours", fi.MIN_NEIGHBOURS)
def test_vectorised_restatement_equals_the_loop(min_neighbours):
    """Both statements of the header's definition agree bit for bit, at every step count (a run of fewer steps is a prefix
    of the loop's: its generations tell which points it has reached)."""
    for index, (name, v) in enumerate(_family()):
        (lt, lw, lc, lgen, lcounts), _ = _loop(index, min_neighbours)
        for steps in fi.STEPS:
            t, w, c, gen, counts = fr.fill(*v.arrays()[:3], steps, min_neighbours)
            what = f"{name}, {steps} steps, {min_neighbours} neighbours"
            reached = lgen <= steps + 1
            assert np.array_equal(gen, np.where(reached, lgen, 0)), what
            assert counts == lcounts[:steps], what
            # a point the shorter run has not reached still holds the input
            expect = [np.where(reached, lt, v.tsdf), np.where(reached, lw, v.weight), np.where(reached[..., None], lc, v.color)]
            assert _same_volume((t, w, c), expect), what


def test_family_coverage():
    filled_with, refused_with = np.zeros(7, np.int64), np.zeros(7, np.int64)
    from_filled = lone_negative_zero = 0
    five_in_a_row = []
    faces = np.zeros(6, bool)
    corner = False
    for index, (name, v) in enumerate(_family()):
        for mn in fi.MIN_NEIGHBOURS:
            (_, _, _, gen, counts), stats = _loop(index, mn)
            filled_with += stats["filled_with"]
            refused_with += stats["refused_with"]
            from_filled += stats["from_filled"]
            lone_negative_zero += stats["lone_negative_zero"]
            if all(n > 0 for n in counts[:5]):
                five_in_a_row.append((name, mn))
            f = gen >= 2
            faces |= [f[..., 0].any(), f[..., -1].any(), f[:, 0].any(), f[:, -1].any(), f[0].any(), f[-1].any()]
            corner = corner or bool(f[::f.shape[0] - 1, ::f.shape[1] - 1, ::f.shape[2] - 1].any())
    assert filled_with[0] == 0 and (filled_with[1:] > 0).all(), filled_with       # every count 1 .. 6 at a filled point
    assert refused_with[6] == 0 and (refused_with[:6] > 0).all(), refused_with   # every count 0 .. 5 at a refused one
    assert five_in_a_row, "no volume fills something in each of five consecutive steps"
    assert from_filled > 0 and lone_negative_zero > 0
    assert faces.all() and corner


def test_lone_negative_zero_gives_positive_zero():
    """+0.0f + -0.0f = +0.0f: outside for the extraction."""
    v = fi.plane_with_slab()
    t, w, _, gen, _ = fr.fill(*v.arrays()[:3], 1)
    got = t[6, 3, 4]
    assert gen[6, 3, 4] == 2 and v.tsdf[5, 3, 4] == 0 and np.signbit(v.tsdf[5, 3, 4]) and got == 0 and not np.signbit(got)


def test_single_point_grows_as_a_clipped_l1_ball():
    v = fi.single_point()
    nx, ny, nz = v.dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dist = abs(i - 3) + abs(j - 1) + abs(k - 2)
    t, w, c, gen, counts = fr.fill(*v.arrays()[:3], LAST)
    assert np.array_equal(gen, np.where(dist <= LAST, dist + 1, 0))
    assert counts == [int((dist == s).sum()) for s in range(1, LAST + 1)]
    assert (t[gen > 0] == F32(-0.375)).all() and (w[gen > 1] == 1).all()
    assert np.array_equal(c[gen > 1], np.broadcast_to(np.array([10.0, 20.0, 30.0], F32), c[gen > 1].shape))


@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_near_misses_change_some_case(variant):
    """Each named near-miss of the definition differs from it on some member of the family: the comparison with the
    device would catch a kernel that made it."""
    for index, (name, v) in enumerate(_family()):
        if v.tsdf.size > 12000:
            continue
        for mn in (1, 2):
            right, _ = _loop(index, mn)
            wrong = fr.fill_loop(*v.arrays()[:3], LAST, mn, variant=variant)
            observed = right[1] > 0
            differs = (not np.array_equal(right[3], wrong[3]) or not np.array_equal(_bits(right[1]), _bits(wrong[1]))
                       or not np.array_equal(_bits(right[0])[observed], _bits(wrong[0])[observed])
                       or not np.array_equal(_bits(right[2])[observed], _bits(wrong[2])[observed]))
            if differs:
                return
    pytest.fail(f"near-miss {variant!r} changes no case of the family")


def test_properties():
    for name, v in _family():
        tsdf, weight, color = v.arrays()[:3]
        for mn in (1, 2):
            whole = fr.fill(tsdf, weight, color, 5, mn)
            first = fr.fill(tsdf, weight, color, 2, mn)
            both = fr.fill(*first[:3], 3, mn)
            assert _same_volume(whole, both), f"{name}: fill(2) then fill(3) is not fill(5)"
            t, w, c, gen, counts = whole
            seen = weight > 0
            assert np.array_equal(gen == 1, seen)
            assert np.array_equal(_bits(t)[seen], _bits(tsdf)[seen]) and np.array_equal(_bits(w)[seen], _bits(weight)[seen])
            assert np.array_equal(_bits(c)[seen], _bits(color)[seen]), f"{name}: an observed point changed"
            assert counts == [int((gen == s + 1).sum()) for s in range(1, 6)], name
            assert np.array_equal(w > 0, gen > 0) and (w[gen > 1] == 1).all()
            # untouched where nothing was filled
            assert np.array_equal(_bits(t)[gen == 0], _bits(tsdf)[gen == 0])
            if (gen > 1).any():
                # A mean of values in [lo, hi] lies in [lo, hi] in exact arithmetic.  In float32 a step rounds at most 5 sums
                # and 1 quotient, each by at most 2^-24 of a magnitude that stays below max |observed| (1 + 2^-20), so a point
                # of generation s + 1 leaves the interval by at most s * 6 * 2^-24 * max |observed|: (x + x + x) / 3 need not
                # be x.  That is the slack, and nothing wider.
                slack = F32(5 * 6 * 2.0 ** -24) * np.abs(tsdf[seen]).max() * F32(1 + 2.0 ** -20)
                assert tsdf[seen].min() - slack <= t[gen > 1].min() and t[gen > 1].max() <= tsdf[seen].max() + slack, name
                mean =color[seen] / weight[seen][:, None]
                assert (c[gen > 1] >= mean.min(axis=0) - 1e-3).all() and (c[gen > 1] <= mean.max(axis=0) + 1e-3).all(), name


def test_nothing_to_fill():
    for v in (mv.constant_volume(0.75), fi.all_unobserved()):
        for mn in fi.MIN_NEIGHBOURS:
            out = fr.fill(*v.arrays()[:3], 5, mn)
            assert out[4] == [0] * 5 and _same_volume(out, v.arrays())


# ---- against an analytic truth ------------------------------------------------------------------------------

def test_sphere_with_a_tube_closes_after_four_steps():
    """(a): sphere_volume(33) without the tube x^2 + y^2 < 0.2^2, z > 0 (592 points).  Measured: as given defects (0, 60)
    and 18 000 faces; 4 steps fill 277, 189, 113, 13 points and close it at the intact sphere's 18 408 faces with every
    vertex within 0.0401 of the radius; after 2 steps it is still open, (0, 28).  The gate is one voxel, 0.0625:
    interpolating between grid points cannot promise less."""
    v, hidden = fi.sphere_with_tube(33)
    intact = mv.sphere_volume(33).extract()
    assert int(hidden.sum()) == 592
    before = fi.mesh_report(*v.arrays())
    print("as given:", before)
    assert before["defects"][0] == 0 and before["defects"][1] > 0
    t, w, c, gen, counts = fr.fill(*v.arrays()[:3], 2)
    two = fi.mesh_report(t, w, c, v.origin, v.voxel)
    print("2 steps:", counts, two)
    assert two["defects"][0] == 0 and two["defects"][1] > 0
    t, w, c, gen, counts = fr.fill(*v.arrays()[:3], 4)
    four = fi.mesh_report(t, w, c, v.origin, v.voxel)
    print("4 steps:", counts, four)
    assert four["defects"] == (0, 0) and four["faces"] == len(intact[1])
    assert four["worst"] <= float(v.voxel)
    assert (before["defects"], before["faces"], two["defects"], counts, four["faces"]) == ((0, 60), 18000, (0, 28), [277, 189, 113, 13], 18408)


@functools.lru_cache(maxsize=None)
def _integrated(views):
    sc = fi.axis_scene(views)
    return sc, sc.integrate()


def test_six_axis_views_with_an_unsure_cap_close_after_two_steps():
    """(b): six axis views of the sphere, confidence 0 within cos > 0.96 of (1,1,1)/sqrt(3).  Measured: as integrated
    defects (0, 60); after 2 steps (0, 0), 9 536 vertices, 19 068 faces, worst radial error 0.060 = 0.96 voxel.  The gate
    is 1.5 voxels: the measured value plus half a voxel for the integration's nearest-pixel depth lookup."""
    sc, (t, w, c) = _integrated(6)
    before = fi.mesh_report(t, w, c, sc.origin, sc.voxel)
    print("as integrated:", before)
    assert before["defects"][0] == 0 and before["defects"][1] > 0
    ft, fw, fc, gen, counts = fr.fill(t, w, c, 2)
    after = fi.mesh_report(ft, fw, fc, sc.origin, sc.voxel)
    print("2 steps:", counts, after)
    assert after["defects"] == (0, 0)
    assert after["worst"] < 1.5 * float(sc.voxel)


def test_three_views_the_unseen_half_is_invented():
    """(c), the limitation, recorded: the same scene from the first three views only.  After 8 steps the unseen half is
    closed by an invented surface (measured: 1 089 vertices more than 2 voxels off the sphere, the worst 0.45 off); with
    min_neighbours = 2 it is 274 and 0.31, and the mesh is not yet closed.  Gated: closed, and that the invention shows; the
    figures are printed."""
    sc, (t, w, c) = _integrated(3)
    before = fi.mesh_report(t, w, c, sc.origin, sc.voxel)
    ft, fw, fc, _, counts = fr.fill(t, w, c, 8)
    one = fi.mesh_report(ft, fw, fc, sc.origin, sc.voxel)
    ft, fw, fc, _, counts2 = fr.fill(t, w, c, 8, 2)
    two = fi.mesh_report(ft, fw, fc, sc.origin, sc.voxel)
    print("as integrated:", before, "\n8 steps:", counts, one, "\n8 steps, 2 neighbours:", counts2, two)
    assert before["defects"][1] > 0 and one["defects"] == (0, 0)
    assert one["far"] > two["far"] > 0 == before["far"] and one["worst"] > two["worst"] > 2.0 * float(sc.voxel)


def test_reconstruct_mesh_refuses_bad_fill_arguments_before_any_work():
    import amvs
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera = amvs.Camera(K=np.array([[30.0, 0, 16.0], [0, 30.0, 12.0], [0, 0, 1]]), dist=np.zeros(5))
    pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=1, num_samples=2, min_views=2, seed=2, device=0)
    for bad in (-1, 65, 1000, 1.5, "2", None, True, np.nan, np.inf, [2]):
        with pytest.raises(ValueError, match="fill_holes_voxels must be an integer in 0 .. 64"):
            pm.reconstruct_mesh(None, None, None, fill_holes_voxels=bad)
    for bad in (0, 7, -1, 1.5, "2", None, True, np.nan, [2]):
        with pytest.raises(ValueError, match="fill_min_neighbours must be an integer in 1 .. 6"):
            pm.reconstruct_mesh(None, None, None, fill_holes_voxels=2, fill_min_neighbours=bad)


def test_header_signatures_and_state_table_name_the_fill():
    from amvs import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "amvs.h")).read()
    for name in ("amvs_tsdf_fill", "amvs_tsdf_fetch_fill"):
        assert name in _lib.SIGNATURES and f"int {name}(amvs_ctx *ctx" in header
    assert len(_lib.SIGNATURES["amvs_tsdf_fill"][1]) == 5 and len(_lib.SIGNATURES["amvs_tsdf_fetch_fill"][1]) == 2
    pkg = [d for d in os.listdir(root) if os.path.isfile(os.path.join(root, d, "csrc", "amvs_mesh_state.h"))]
    assert "tsdf_fill" in open(os.path.join(root, pkg[0], "csrc", "amvs_mesh_state.h")).read()


def test_filling_the_box_of_the_unobserved_points_is_filling_the_volume():
    """What test_hip_mesh_fill.py relies on for the 160^3 sphere: a step reads nothing but the 6-neighbours of unobserved
    points, so the restatement on their box grown by one point, put back, is the restatement on the whole volume."""
    for v in (fi.sphere_with_tube(33)[0], fi.plane_with_slab(), _family()[0][1]):
        for mn in (1, 3):
            whole, part = fr.fill(*v.arrays()[:3], 4, mn), fi.fill_cropped(v, 4, mn)
            assert _same_volume(whole, part) and np.array_equal(whole[3], part[3]) and whole[4] == part[4]

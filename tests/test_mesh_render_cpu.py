"""The restatement of the mesh rasteriser, the visibility counts and their filter (tests/mesh_render_restatement.py)
against plain per-pixel loops, the top-left rule, an analytic sphere and the concentric-spheres scene, and the
hand-built inputs (tests/mesh_render_inputs.py) each asserted to do what it was built for.  No GPU: the device code is
compared with the same restatement, bit for bit, in tests/test_hip_mesh_render.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_inputs as ri  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32


def _render(case):
    return rr.render(case.verts, case.faces, case.K, case.poses, case.near, case.H, case.W)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def sphere():
    return ri.sphere_mesh(33)


def test_restatement_equals_per_pixel_loops_on_the_hand_built_inputs():
    for case in ri.hand_built():
        depth, face, skipped = _render(case)
        ld, lf, ls = rr.render_loops(case.verts, case.faces, case.K, case.poses, case.near, case.H, case.W)
        assert np.array_equal(face, lf), case.name
        assert np.array_equal(_bits(depth), _bits(ld)), case.name
        assert np.array_equal(skipped, ls), case.name
        assert np.array_equal(face >= 0, depth > 0), case.name


def test_restatement_equals_per_pixel_loops_through_rotated_cameras():
    """The hand-built cases look along +z from the origin, where a mistaken row of R or K could hide: small meshes
    through the six cameras of views_for (general rotations, one camera inside the mesh's box) and the axis views."""
    import mesh_clean_inputs as ci
    H, W = 24, 32
    n_skipped = n_drawn = 0
    for m in (ci.closed_book(), ci.tie(), ci.threshold()):
        K, poses, near = ri.views_for(m.verts, 6, H, W)
        for cams, Kc in ((poses, K), (ri.axis_views(3.0), np.array([[20.0, 1.5, 15.0], [0.25, 22.0, 13.0], [0.001, -0.002, 1.0]], F32))):
            depth, face, skipped = rr.render(m.verts, m.faces, Kc, cams, near, H, W)
            ld, lf, ls = rr.render_loops(m.verts, m.faces, Kc, cams, near, H, W)
            assert np.array_equal(face, lf) and np.array_equal(_bits(depth), _bits(ld)) and np.array_equal(skipped, ls), m.name
            n_skipped += int(skipped.sum())
            n_drawn += int((face >= 0).sum())
    assert n_skipped > 0 and n_drawn > 1000                     # neither path is vacuous


def test_every_shared_edge_pixel_is_covered_exactly_once():
    case = ri.shared_edges()
    cover = np.zeros((case.H, case.W), np.int64)
    for f in range(len(case.faces)):
        _, face, _ = rr.render(case.verts, case.faces[f:f + 1], case.K, case.poses, case.near, case.H, case.W)
        cover += face[0] >= 0
    (x0, y0, _, y1), (_, _, x2, _) = ri.SHARED_QUADS
    inside = np.zeros_like(cover)
    inside[y0:y1, x0:x2] = 1                                     # top and left edges in, bottom and right out
    assert np.array_equal(cover, inside)
    # the pixels the shared edges pass through are among them: both diagonals and the common vertical edge
    on_edges = [(k, k) for k in range(3, 10)] + [(10, y) for y in range(3, 10)] + [(20 - k, k) for k in range(3, 10)]
    assert all(cover[y, x] == 1 for x, y in on_edges)
    # drawn together, every covered pixel names one of the two faces that meet there, and depth varies over the quads
    depth, face, _ = _render(case)
    assert np.array_equal(face[0] >= 0, inside.astype(bool))
    assert set(np.unique(face[0])) == {-1, 0, 1, 2, 3}
    assert len(np.unique(depth[0][inside == 1])) >= 9            # 1 / z is linear over a quad of 8 pixels: ninths


def test_hand_built_cases_do_what_they_were_built_for():
    depth, face, skipped = _render(ri.coincident())
    assert skipped[0] == 0 and (face[0] >= 0).sum() > 40 and set(np.unique(face[0])) == {-1, 0}    # the smallest id wins
    alone = [rr.render(ri.coincident().verts, ri.coincident().faces[f:f + 1], ri.K_HAND, ri.IDENTITY, ri.NEAR, ri.H, ri.W)
             for f in range(3)]
    assert all(np.array_equal(_bits(a[0]), _bits(depth)) for a in alone)       # equal depth bits, either winding

    depth, face, skipped = _render(ri.behind_near())
    assert skipped[0] == 1 and set(np.unique(face[0])) == {-1, 0}
    zc = rr.project(ri.behind_near().verts, ri.K_HAND, ri.IDENTITY, ri.NEAR)[0]
    assert (zc <= ri.NEAR).sum() == 1

    depth, face, skipped = _render(ri.beyond_limit())
    _, u, _, _, usable, _, _ = rr.project(ri.beyond_limit().verts, ri.K_HAND, ri.IDENTITY, ri.NEAR)
    assert skipped[0] == 1 and set(np.unique(face[0])) == {-1, 0}
    assert (~usable).sum() == 1 and u[~usable][0] > 2.0 ** 20

    case = ri.zero_area()
    depth, face, skipped = _render(case)
    s = rr.Setup(case.verts, case.faces, case.K, case.poses[0], case.near, case.H, case.W)
    assert skipped[0] == 0 and s.usable_face.all() and (s.area_all == 0).all() and (face[0] == -1).all()

    case = ri.whole_image()
    depth, face, skipped = _render(case)
    s = rr.Setup(case.verts, case.faces, case.K, case.poses[0], case.near, case.H, case.W)
    assert skipped[0] == 0 and (face[0] == 0).all() and s.box_all[0] == case.H * case.W       # the box is clamped
    assert np.abs(s.x).max() > 256 * 4000 and len(np.unique(depth[0])) > 50

    case = ri.off_image()
    depth, face, skipped = _render(case)
    s = rr.Setup(case.verts, case.faces, case.K, case.poses[0], case.near, case.H, case.W)
    assert skipped[0] == 0 and (face[0] == -1).all() and (depth[0] == 0).all()
    assert s.usable_face.all() and (s.area_all != 0).all() and (s.box_all == 0).all() and len(s.face) == 0

    case = ri.everything()
    depth, face, skipped = _render(case)
    assert skipped[0] == 2 and (face[0] >= 0).all() and len(np.unique(face[0])) >= 7


def test_reversed_winding_gives_the_same_coverage_and_face_ids():
    for case in (ri.shared_edges(), ri.everything()):
        _, face, skipped = _render(case)
        _, rface, rskipped = _render(ri.reversed_winding(case))
        assert np.array_equal(face, rface) and np.array_equal(skipped, rskipped), case.name


def _analytic_sphere_depth(H, W, focal, distance, radius):
    K = ri.pinhole(focal, H, W).astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs - K[0, 2]) / focal, (ys - K[1, 2]) / focal, np.ones((H, W))], -1)
    dc, dd = d[..., 2] * distance, (d * d).sum(-1)
    disc = dc * dc - dd * (distance * distance - radius * radius)
    hit = disc > 0
    return np.where(hit, (dc - np.sqrt(np.where(hit, disc, 0))) / dd, 0.0), hit


def test_sphere_from_six_axis_views_against_the_analytic_depth(sphere):
    from scipy.ndimage import binary_fill_holes
    v, f, _ = sphere
    H, W, focal, distance = 48, 64, 60.0, 3.0
    voxel = float(mv.sphere_volume(33).voxel)
    depth, face, skipped = rr.render(v, f, ri.pinhole(focal, H, W), ri.axis_views(distance), 0.1, H, W)
    ref, hit = _analytic_sphere_depth(H, W, focal, distance, 0.8)
    assert (skipped == 0).all()
    worst = rms = 0.0
    for m in range(6):
        mask = face[m] >= 0
        assert np.array_equal(binary_fill_holes(mask), mask), f"view {m}: holes"
        both = mask & hit
        err = np.abs(depth[m][both].astype(np.float64) - ref[both])
        print(f"view {m}: {int(mask.sum())} pixels, {int((mask != hit).sum())} off the analytic silhouette, "
              f"max {err.max() / voxel:.3f} voxel, rms {np.sqrt((err ** 2).mean()) / voxel:.4f} voxel")
        assert (mask != hit).sum() <= 2 and both.sum() > 700         # 2 of 871 pixels: DESIGN.md section 8
        worst, rms = max(worst, err.max()), max(rms, np.sqrt((err ** 2).mean()))
    assert worst <= voxel and rms <= 0.2 * voxel


def test_concentric_spheres_the_filter_removes_exactly_the_inner_one():
    v, f, c, n_outer_v, n_outer_f = ri.concentric_spheres()
    H, W = 37, 53
    K, poses = ri.pinhole(50.0, H, W), ri.axis_views(3.0)
    voxel = mv.sphere_volume(33).voxel
    depth, face, skipped = rr.render(v, f, K, poses, 0.1, H, W)
    assert (skipped == 0).all() and face.max() < n_outer_f                    # no inner face in any map
    counts = rr.visibility(v, K, poses, 0.1, depth, voxel)
    assert counts.dtype == np.int32 and counts[:n_outer_v].min() >= 1 and counts[n_outer_v:].max() == 0
    fv, ff, fc = rr.filter_visible(v, f, c, counts, 1)
    assert np.array_equal(fv.view(np.uint32), v[:n_outer_v].view(np.uint32))
    assert np.array_equal(ff, f[:n_outer_f]) and np.array_equal(fc, c[:n_outer_v])
    assert mv.directed_edge_defects(ff, len(fv)) == (0, 0)
    edges = len(np.unique(np.sort(np.concatenate([ff[:, [0, 1]], ff[:, [1, 2]], ff[:, [2, 0]]]), axis=1), axis=0))
    assert len(fv) - edges + len(ff) == 2
    # a vertex needs more views than any has: nothing is left
    assert [len(a) for a in rr.filter_visible(v, f, c, counts, 7)] == [0, 0, 0]


def test_visibility_guards():
    """In front of near, inside the image by floorf(u + 0.5f), nothing drawn counts as seen, and the tolerance is
    inclusive."""
    verts = np.array([ri.at_pixel(5, 5, 2.0), ri.at_pixel(5, 5, 4.0), ri.at_pixel(-0.5, 3, 2.0), ri.at_pixel(-0.75, 3, 2.0),
                      ri.at_pixel(ri.W - 0.5, 3, 2.0), (0.0, 0.0, 0.25), ri.at_pixel(20, 20, 8.0)], F32)
    depth = np.zeros((1, ri.H, ri.W), F32)
    depth[0, 5, 5] = 2.0
    for tol, expect in ((0.0, [1, 0, 1, 0, 0, 0, 1]), (2.0, [1, 1, 1, 0, 0, 0, 1]), (1.9999, [1, 0, 1, 0, 0, 0, 1])):
        counts = rr.visibility(verts, ri.K_HAND, ri.IDENTITY, ri.NEAR, depth, tol)
        assert counts.tolist() == expect, tol

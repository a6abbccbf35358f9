"""The restatement of the colours from the views and of the colour render (tests/mesh_color_restatement.py) against
plain loops, what the family of tests/mesh_color_inputs.py reaches (so that the bit-for-bit comparison on the device,
tests/test_hip_mesh_color.py, cannot silently leave a branch out), an analytic sphere, the concentric-spheres scene, a
photometric property of the colour render, and the named near-misses of the definition.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_inputs as ci  # noqa: E402
import mesh_clean_restatement as cr  # noqa: E402
import mesh_color_inputs as ki  # noqa: E402
import mesh_color_restatement as kr  # noqa: E402
import mesh_render_inputs as ri  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
import mesh_volumes as mv  # noqa: E402

F32 = np.float32
FULL_K = np.array([[20.0, 1.5, 15.0], [0.25, 22.0, 13.0], [0.001, -0.002, 1.0]], F32)


def _case_maps(case):
    return rr.render(case.verts, case.faces, case.K, case.poses, case.near, case.H, case.W)[:2]


def _color(case, depth, min_cos, best, tolerance=None, **kw):
    tol = case.tolerance if tolerance is None else tolerance
    return kr.color_views(case.verts, case.normals, case.colors, case.K, case.poses, case.near, depth, case.images, tol, min_cos,
                          best, **kw)


def test_restatement_equals_the_loops_on_the_hand_built_cases():
    for case in ki.hand_built():
        depth, face = _case_maps(case)
        for min_cos in ki.MIN_COS:
            for best in (False, True):
                got = _color(case, depth, min_cos, best)
                ref = kr.color_views_loops(case.verts, case.normals, case.colors, case.K, case.poses, case.near, depth, case.images,
                                           case.tolerance, min_cos, best)
                assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], (case.name, min_cos, best)
        args = (case.verts, case.faces, got[0], case.K, case.poses, case.near, depth, face)
        assert np.array_equal(kr.render_color(*args), kr.render_color_loops(*args)), case.name


def test_restatement_equals_the_loops_through_rotated_cameras_and_a_full_K():
    """The hand-built cases look along +z through a diagonal K, where a mistaken row of R or K could hide."""
    H, W = 24, 32
    reached = drawn = 0
    for m in (ci.closed_book(), ci.threshold(), ci.Mesh("sphere 11^3", *mv.sphere_volume(11).extract()[:2], seed=12)):
        normals = cr.normals(m.verts, m.faces)
        K, poses, near = ri.views_for(m.verts, 6, H, W)
        for cams, Kc in ((poses, K), (ri.axis_views(3.0), FULL_K)):
            depth, face, _ = rr.render(m.verts, m.faces, Kc, cams, near, H, W)
            images = ki.images_for(6, H, W, 99)
            for best in (False, True):
                cnt = {}
                got = kr.color_views(m.verts, normals, m.colors, Kc, cams, near, depth, images, near, 0.0, best, counters=cnt)
                ref = kr.color_views_loops(m.verts, normals, m.colors, Kc, cams, near, depth, images, near, 0.0, best)
                assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], (m.name, best)
                reached += cnt["reached"]
            args = (m.verts, m.faces, got[0], Kc, cams, near, depth, face)
            assert np.array_equal(kr.render_color(*args), kr.render_color_loops(*args)), m.name
            drawn += int((face >= 0).sum())
    assert reached > 100 and drawn > 1000                       # neither comparison is vacuous


def test_the_family_reaches_every_branch():
    """Counted over exactly what test_hip_mesh_color.py compares bit for bit (DESIGN.md section 8 records the counts)."""
    total, uncoloured, differ = {}, 0, 0
    for H, W in ki.SIZES:
        for mem in ki.family(H, W):
            depth, _ = mem.maps()
            for n in mem.n_views:
                for tol in mem.tolerances:
                    for min_cos in ki.MIN_COS:
                        args = (mem.verts, mem.normals, mem.colors, mem.K, mem.poses[:n], mem.near, depth[:n], mem.images[:n], tol, min_cos)
                        blend, nb = kr.color_views(*args, False, counters=total)
                        best, nk = kr.color_views(*args, True)
                        assert nb == nk
                        uncoloured += len(mem.verts) - nb
                        differ += int((blend != best).any(axis=1).sum())
    print(f"family: {total}, {uncoloured} vertices left uncoloured, {differ} differ between blend and best view")
    for name in ("reached", "border", "undrawn", "nearer", "farther", "cosine"):
        assert total[name] >= 100, (name, total)
    assert uncoloured >= 20 and differ >= 20


def _footprint(case, depth, vertex):
    zc, u, v = rr.project(case.verts[vertex:vertex + 1], case.K, case.poses[0], case.near)[:3]
    x0, y0 = int(np.floor(u[0])), int(np.floor(v[0]))
    return zc[0], u[0], v[0], x0, y0, depth[0][y0:y0 + 2, x0:x0 + 2]


def test_hand_built_cases_reach_their_own_edges():
    def run(case, min_cos=0.0, best=False, **kw):
        depth, _ = _case_maps(case)
        cnt = {}
        out, n = _color(case, depth, min_cos, best, counters=cnt, **kw)
        return depth, out, (out != case.colors).any(axis=1), cnt, n

    case = ki.integer_u()
    depth, out, changed, cnt, n = run(case)
    zc, u, v, x0, y0, d = _footprint(case, depth, case.focus["integer u"])
    assert u == 7.0 and v == 6.25 and (d == 2.0).all() and changed[case.focus["integer u"]]
    img = case.images[0].astype(np.float64)
    expect = np.floor(0.75 * img[6, 7] + 0.25 * img[7, 7] + 0.5)[::-1]          # ax = 0: the left column alone
    assert np.array_equal(out[case.focus["integer u"]], expect)
    zero = case.focus["zero normal"]
    assert not case.normals[zero].any() and (_footprint(case, depth, zero)[5] == 2.0).all() and not changed[zero]
    assert cnt["cosine"] == 1 and not changed[case.focus["right edge"]] and cnt["undrawn"] > 0

    case = ki.borders()
    depth, out, changed, cnt, n = run(case)
    assert (depth[0] > 0).all()
    for name, x0, y0, taken in (("x0 = 0", 0, 5, True), ("x0 = -1", -1, 5, False), ("x0 = W - 2", ri.W - 2, 5, True),
                                ("x0 = W - 2, integer", ri.W - 2, 5, True), ("x0 = W - 1", ri.W - 1, 5, False),
                                ("y0 = 0", 5, 0, True), ("y0 = -1", 5, -1, False), ("y0 = H - 2", 5, ri.H - 2, True),
                                ("y0 = H - 1", 5, ri.H - 1, False)):
        _, u, v, *_ = _footprint(case, np.zeros((1, 2 * ri.H, 2 * ri.W)), case.focus[name])
        assert (int(np.floor(u)), int(np.floor(v))) == (x0, y0) and changed[case.focus[name]] == taken, name
    assert cnt["border"] >= 50 and cnt["undrawn"] == cnt["nearer"] == cnt["farther"] == 0

    case = ki.one_undrawn()
    depth, out, changed, cnt, n = run(case)
    d = _footprint(case, depth, case.focus["inner corner"])[5]
    assert (d > 0).sum() == 3 and d[1, 1] == 0 and not changed[case.focus["inner corner"]] and changed[case.focus["inside"]]

    case = ki.two_sheets()
    depth, out, changed, cnt, n = run(case)
    zc, _, _, _, _, d = _footprint(case, depth, case.focus["behind the near sheet"])
    assert zc == 4.0 and (d == 2.0).all() and not changed[case.focus["behind the near sheet"]]
    zc, _, _, _, _, d = _footprint(case, depth, case.focus["near, on the outline"])
    assert zc == 2.0 and (d > 0).all() and (d == 2.0).any() and (d == 4.0).any() and not changed[case.focus["near, on the outline"]]
    zc, _, _, _, _, d = _footprint(case, depth, case.focus["near, right edge"])
    assert zc == 2.0 and (d == 4.0).all() and not changed[case.focus["near, right edge"]]
    zc, _, _, _, _, d = _footprint(case, depth, case.focus["far, straddling"])
    assert zc == 4.0 and (d == 2.0).any() and (d == 4.0).any() and not changed[case.focus["far, straddling"]]
    assert changed[case.focus["far, clear"]] and changed[case.focus["near, inside"]] and cnt["nearer"] > 0 and cnt["farther"] > 0
    # with more than the whole depth difference as tolerance nothing is occluded any more
    assert run(case, tolerance=2.5)[3]["nearer"] == 0

    case = ki.twin_cameras()
    depth, best, _, _, _ = run(case, best=True)
    alone = kr.color_views(case.verts, case.normals, case.colors, case.K, case.poses[:1], case.near, depth[:1], case.images[:1],
                           case.tolerance, 0.0, True)[0]
    assert np.array_equal(best, alone) and not np.array_equal(case.images[0], case.images[1])     # the lower index wins
    blend = run(case)[1]
    assert (blend != best).any()

    case = ki.twin_constant()
    depth, out, changed, cnt, n = run(case)
    axis = case.focus["on the axis"]
    cos = -case.normals[axis] @ case.verts[axis] / np.linalg.norm(case.verts[axis])
    assert cos == 1.0 and out[axis].tolist() == [11, 11, 11]                    # q = 10.5 exactly, rounded half up
    assert run(case, best=True)[1][axis].tolist() == [10, 10, 10]

    case = ki.fused_tap()
    depth, out, changed, cnt, n = run(case, best=True)
    zc, u, v, x0, y0, d = _footprint(case, depth, case.focus["tap"])
    assert u == ki.FUSED_AX and v == 6.0 and (x0, y0) == (0, 6) and out[case.focus["tap"]].tolist() == [7, 7, 7]

    case = ki.grazing()
    at0, at5 = run(case, 0.0), run(case, 0.5)
    assert at0[3]["cosine"] == 0 and at5[3]["cosine"] >= 5 and at5[4] < at0[4] and at5[3]["reached"] >= 20

    # a vertex no view sees keeps its colour, in every case
    for case in ki.hand_built():
        depth, out, changed, cnt, n = run(case)
        assert 0 < n == changed.sum() < len(case.verts) and np.array_equal(out[~changed], case.colors[~changed]), case.name


# ---- the analytic sphere ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sphere():
    (v, f, c), K, poses, near, H, W, *_ = ki.sphere_case()
    images, hits = ki.sphere_images()
    depth, face, _ = rr.render(v, f, K, poses, near, H, W)
    return dict(v=v, f=f, c=c, K=K, poses=poses, near=near, H=H, W=W, images=images, hits=hits, depth=depth, face=face,
                normals=cr.normals(v, f), voxel=mv.sphere_volume(33).voxel)


# measured on the restatement: maximum 1.62 codes, mean 0.304; the gate is that maximum plus one code for the final
# rounding and one for the half-voxel geometric error the render's sphere test allows
SPHERE_GATE = 1.62 + 2


def test_sphere_colours_against_the_analytic_function(sphere):
    s = sphere
    out, n = kr.color_views(s["v"], s["normals"], s["c"], s["K"], s["poses"], s["near"], s["depth"], s["images"], s["voxel"], 0.2, False)
    # the recoloured vertices are those whose result does not depend on the colour they started with
    args = (s["K"], s["poses"], s["near"], s["depth"], s["images"], s["voxel"], 0.2, False)
    colored = (kr.color_views(s["v"], s["normals"], np.zeros_like(s["c"]), *args)[0] ==
               kr.color_views(s["v"], s["normals"], np.full_like(s["c"], 255), *args)[0]).all(axis=1)
    assert colored.sum() == n and n > 0.9 * len(s["v"])
    truth = ki.sphere_colour(s["v"].astype(np.float64))[:, ::-1]               # B, G, R -> the mesh's R, G, B
    err = np.abs(out[colored].astype(np.float64) - truth[colored])
    print(f"sphere: {n} of {len(s['v'])} vertices recoloured, error max {err.max():.2f} codes, mean {err.mean():.3f}")
    assert err.max() <= SPHERE_GATE


def test_concentric_spheres_the_inner_vertices_keep_their_colours():
    v, f, c, n_outer_v, n_outer_f = ri.concentric_spheres()
    H, W = 37, 53
    K, poses = ri.pinhole(50.0, H, W), ri.axis_views(3.0)
    voxel = mv.sphere_volume(33).voxel
    depth = rr.render(v, f, K, poses, 0.1, H, W)[0]
    images = ki.images_for(6, H, W, 41)
    images[3:5] = images[:2][:, ::-1]                                           # noise in every view
    normals = cr.normals(v, f)
    for best in (False, True):
        for start in (np.zeros_like(c), np.full_like(c, 255)):
            out, n = kr.color_views(v, normals, start, K, poses, 0.1, depth, images, voxel, 0.2, best)
            assert np.array_equal(out[n_outer_v:], start[n_outer_v:]) and 0 < n <= n_outer_v


def test_the_colour_render_comes_closer_to_the_images(sphere):
    """TSDF-style starting colours -- the mean over all six images of the nearest pixel, taken without any occlusion
    test -- against the colours from the views: mean absolute difference between the colour render and the input image
    over the drawn pixels, summed over the views."""
    s = sphere
    total, hits = np.zeros((len(s["v"]), 3)), np.zeros(len(s["v"]))
    for m in range(6):
        zc, u, v = rr.project(s["v"], s["K"], s["poses"][m], s["near"])[:3]
        fx, fy = np.floor(u + F32(0.5)).astype(np.int64), np.floor(v + F32(0.5)).astype(np.int64)
        ok = (zc > s["near"]) & (fx >= 0) & (fx < s["W"]) & (fy >= 0) & (fy < s["H"])
        total[ok] += s["images"][m][fy[ok], fx[ok]][:, ::-1]
        hits += ok
    start = np.floor(total / np.maximum(hits, 1)[:, None] + 0.5).astype(np.uint8)
    after = kr.color_views(s["v"], s["normals"], start, s["K"], s["poses"], s["near"], s["depth"], s["images"], s["voxel"], 0.2, False)[0]

    def distance(colors):
        pic = kr.render_color(s["v"], s["f"], colors, s["K"], s["poses"], s["near"], s["depth"], s["face"])
        drawn = s["face"] >= 0
        return sum(np.abs(pic[m][drawn[m]].astype(np.float64) - s["images"][m][drawn[m]][:, ::-1]).mean() for m in range(6))

    before, now = distance(start), distance(after)
    print(f"photometric distance, summed over six views: {before:.3f} codes before, {now:.3f} after")
    assert now < before


def test_every_named_near_miss_changes_some_result(sphere):
    s = sphere
    cases = [(c, _case_maps(c)[0]) for c in ki.hand_built()]
    for miss in kr.NEAR_MISSES:
        found = False
        for case, depth in cases:
            for min_cos in ki.MIN_COS:
                for best in (False, True):
                    ref = _color(case, depth, min_cos, best)
                    got = _color(case, depth, min_cos, best, miss=miss)
                    found = found or not np.array_equal(ref[0], got[0]) or ref[1] != got[1]
        if not found:                                               # the sphere, in six general views of noise
            noise = ki.images_for(6, s["H"], s["W"], 5)
            args = (s["v"], s["normals"], s["c"], s["K"], s["poses"], s["near"], s["depth"], noise, s["voxel"], 0.2)
            for best in (False, True):
                found = found or not np.array_equal(kr.color_views(*args, best)[0], kr.color_views(*args, best, miss=miss)[0])
        assert found, miss

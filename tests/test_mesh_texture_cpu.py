"""The restatement of the texture and of the textured render (tests/mesh_texture_restatement.py) against plain loops, the
layout's properties, what the family of tests/mesh_texture_inputs.py reaches (so that the bit-for-bit comparison on the
device, tests/test_hip_mesh_texture.py, cannot silently leave a branch out), the named near-misses of the definition, the
OBJ / MTL / PNG writer, an analytic sphere, and the argument rules of reconstruct_mesh that need no device.  No GPU."""
import functools
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_restatement as cr  # noqa: E402
import mesh_color_restatement as kr  # noqa: E402
import mesh_render_restatement as rr  # noqa: E402
import mesh_texture_inputs as ti  # noqa: E402
import mesh_texture_restatement as tr  # noqa: E402

F32 = np.float32


def _maps(case):
    return rr.render(case.verts, case.faces, case.K, case.poses, case.near, case.H, case.W)[:2]


def _texture(case, depth, N, cpr=0, min_cos=0.0, best=False, **kw):
    return tr.texture(case.verts, case.faces, case.colors, case.K, case.poses, case.near, depth, case.images, case.tolerance, min_cos,
                      best, N, cpr, **kw)


@functools.lru_cache(maxsize=None)
def _family(H, W):
    return ti.family(H, W)


def test_restatement_equals_the_loops_on_the_hand_built_cases():
    for case in ti.hand_built():
        depth, face = _maps(case)
        for N, cpr, min_cos, best in ((2, 0, 0.0, False), (3, 1, 0.5, True), (1, 3, 0.0, True)) + \
                (((8, 0, 0.0, False),) if len(case.faces) <= 16 else ()):
            got = _texture(case, depth, N, cpr, min_cos, best)
            ref = tr.texture_loops(case.verts, case.faces, case.colors, case.K, case.poses, case.near, depth, case.images,
                                   case.tolerance, min_cos, best, N, cpr)
            what = (case.name, N, cpr, min_cos, best)
            assert np.array_equal(got[0], ref[0]) and got[2:] == ref[2:], what
            assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), what
            args = (case.verts, case.faces, got[0], case.K, case.poses, case.near, depth, face, N, cpr)
            assert np.array_equal(tr.render_texture(*args), tr.render_texture_loops(*args)), what


def test_hand_built_cases_reach_their_own_edges():
    # (a) the hypotenuse's midpoint is drawn, by a face whose hypotenuse it is, with g1 = g2 = 0.5: pulled back at even N
    case = ti.hypotenuse()
    depth, face = _maps(case)
    assert face[0, 8, 8] == 0 and depth[0, 8, 8] == 2.0
    only = np.full_like(face, -1)
    only[0, 8, 8] = face[0, 8, 8]
    for N in (2, 8):
        atlas = _texture(case, depth, N)[0]
        cnt = {}
        pic = tr.render_texture(case.verts, case.faces, atlas, case.K, case.poses, case.near, depth, only, N, counters=cnt)
        assert cnt["pull-back"] == 1 and cnt["outside set"] == 0
        # on the hypotenuse halfway between corners 1 and 2: the mean of the face's texels (N/2, N/2) -- exactly that texel
        i = N // 2
        assert np.array_equal(pic[0, 8, 8], atlas[i, i])
        cnt = {}
        tr.render_texture(case.verts, case.faces, atlas, case.K, case.poses, case.near, depth, only, N, miss="no pull-back", counters=cnt)
        assert cnt["outside set"] == 1
    # (b) the owned corner pixels: g exactly 1 at the corner, the lookup clamped, the pixel exactly that corner's texel
    case = ti.corner_triangles()
    depth, face = _maps(case)
    for N in (1, 3, 8):
        atlas = _texture(case, depth, N)[0]
        cnt = {}
        pic = tr.render_texture(case.verts, case.faces, atlas, case.K, case.poses, case.near, depth, face, N, counters=cnt)
        assert cnt["corner clamp"] == 4 and cnt["outside set"] == 0 and 0 < cnt["exchanged"] < int((face >= 0).sum())
        cols = tr.layout(len(case.faces), N)[0]
        for t, (x, y) in enumerate(ti.CORNER_A):
            assert face[0, y, x] == t
            k = t % 3                                                # which corner of face t the vertex A is
            X, Y = tr.atlas_position(np.array([t]), (0, N, 0)[k], (0, 0, N)[k], N, cols)
            assert np.array_equal(pic[0, y, x], atlas[Y[0], X[0]]), (N, t)
    # (c) the sheet that faces the camera: every drawn pixel through exchanged corners.  With an atlas of fall-back texels
    # alone (maps in which nothing is drawn) the textured render is the colour render of the same mesh, within the texel
    # grid's rounding -- through the right g, and far from it through the exchanged one
    case = ti.corner_sheet()
    depth, face = _maps(case)
    atlas, _, n_texels, n_textured = _texture(case, np.zeros_like(depth), 8, counters=(cnt := {}))
    assert n_textured == 0 and cnt["fallen back"] + cnt["gutter fallen back"] == n_texels
    cnt = {}
    args = (case.verts, case.faces, atlas, case.K, case.poses, case.near, depth, face, 8)
    pic = tr.render_texture(*args, counters=cnt)
    assert cnt["exchanged"] == int((face >= 0).sum()) > 100
    flat = kr.render_color(case.verts, case.faces, case.colors, case.K, case.poses, case.near, depth, face)
    wrong = tr.render_texture(*args, miss="g not exchanged back")
    drawn = face >= 0
    err = np.abs(pic[drawn].astype(int) - flat[drawn].astype(int)).max()
    assert err <= 2 < np.abs(wrong[drawn].astype(int) - flat[drawn].astype(int)).max(), err
    back = ti.corner_sheet(True)
    cnt = {}
    assert _texture(back, depth, 3)[3] == 0
    tr.render_texture(back.verts, back.faces, atlas, back.K, back.poses, back.near, depth, face, 8, counters=cnt)
    assert cnt["exchanged"] == 0
    # (d) the degenerate face: zero normal, all of its texels fall back, its neighbours are reached
    case = ti.degenerate()
    depth, face = _maps(case)
    f = case.focus["face"]
    assert not tr._face_frames(case.verts, case.faces)[1][f].any()
    zero = np.zeros_like(case.colors)
    a0, a255 = (tr.texture(case.verts, case.faces, col, case.K, case.poses, case.near, depth, case.images, case.tolerance, 0.0, False, 3)
                for col in (zero, np.full_like(zero, 255)))
    tex = tr.face_texels(3)
    fid = np.full(len(tex), f)
    X, Y = tr.atlas_position(fid, tex[:, 0], tex[:, 1], 3, tr.layout(len(case.faces), 3)[0])
    assert not a0[0][Y, X].any() and (a255[0][Y, X] == 255).all() and a0[3] == a255[3] > 0
    # (e) two sheets: faces with texels of both kinds
    case = ti.ki.two_sheets()
    depth, face = _maps(case)
    a0, a255 = (tr.texture(case.verts, case.faces, col, case.K, case.poses, case.near, depth, case.images, case.tolerance, 0.0, False, 8)
                for col in (np.zeros_like(case.colors), np.full_like(case.colors, 255)))
    same = (a0[0] == a255[0]).all(axis=2)
    tex = tr.face_texels(8)
    mixed = 0
    for f in range(len(case.faces)):
        X, Y = tr.atlas_position(np.full(len(tex), f), tex[:, 0], tex[:, 1], 8, tr.layout(len(case.faces), 8)[0])
        mixed += 0 < same[Y, X].sum() < len(tex)
    assert mixed >= 4
    # (f) constant images 10 and 11 in twin cameras: 10.5 rounds half up wherever both views reach, the first view wins alone
    case = ti.ki.twin_constant()
    depth, face = _maps(case)
    blend = _texture(case, depth, 3, counters=(cnt := {}))
    best = _texture(case, depth, 3, best=True)
    vals = set(np.unique(blend[0][(blend[0] != 0).all(axis=2) & (blend[0] == blend[0][..., :1]).all(axis=2)]).tolist())
    assert 11 in vals and cnt["reached"] > 50
    assert ((blend[0] == 11).all(axis=2) <= (best[0] == 10).all(axis=2)).all() and (blend[0] == 11).all(axis=2).sum() > 50


def test_layout_properties():
    """Every atlas texel belongs to at most one face; a face's set has (N+1)(N+2)/2 + N texels -- the N+1 rows j = 0 .. N
    hold N+2-j texels each (i <= N+1-j), except that i <= N cuts one off row j = 0 and row j = N has 2 (i = 0, 1):
    sum_{j=0..N} (N+2-j) - 1 = (N+1)(N+2) - N(N+1)/2 - 1 = (N+1)(N+2)/2 + N; every lookup's taps lie in the face's own set."""
    shapes = set()
    for H, W in ti.SIZES:
        jobs, refused = _family(H, W)
        shapes |= {(len(j.mem.faces), j.N, j.cells_per_row) for j in jobs}
    assert len(shapes) >= 200
    for F, N, cpr in sorted(shapes):
        cols, rows, Wt, Ht = tr.layout(F, N, cpr)
        C = N + 3
        n_cells = (F + 1) // 2
        if F == 0:
            assert (cols, rows, Wt, Ht) == (0, 0, 0, 0)
            continue
        assert cols == (cpr or cols) and cols * rows >= n_cells > cols * (rows - 1) and (Wt, Ht) == (cols * C, rows * C)
        if cpr == 0:
            assert cols * cols >= n_cells > (cols - 1) * (cols - 1)
        tex = tr.face_texels(N)
        count = sum(1 for i in range(N + 1) for j in range(N + 1) if i + j <= N + 1)          # from the set's definition
        assert len(tex) == count == (N + 1) * (N + 2) // 2 + N
        assert tex.min() == 0 and tex.max() == N and (tex.sum(axis=1) <= N + 1).all() and len({tuple(t) for t in tex.tolist()}) == count
        fi = np.repeat(np.arange(F, dtype=np.int64), count)
        X, Y = tr.atlas_position(fi, np.tile(tex[:, 0], F), np.tile(tex[:, 1], F), N, cols)
        assert X.min() >= 0 and X.max() < Wt and Y.min() >= 0 and Y.max() < Ht
        flat = Y * Wt + X
        assert len(np.unique(flat)) == len(flat), (F, N, cpr)
        # corners 0, 1, 2 are texels (0,0), (N,0), (0,N), and the UVs are their centres with v up
        uv = tr.uvs(F, N, cpr)
        for k, (i, j) in enumerate(((0, 0), (N, 0), (0, N))):
            cx, cy = tr.atlas_position(np.arange(F), i, j, N, cols)
            assert np.array_equal(np.floor(uv[:, k, 0].astype(np.float64) * Wt), cx)
            assert np.array_equal(np.floor((1.0 - uv[:, k, 1].astype(np.float64)) * Ht), cy)
    for N in ti.TEXELS + (5, 64):
        member = np.zeros((N + 2, N + 2), bool)
        member[tuple(tr.face_texels(N).T)] = True
        steps = np.arange(16 * N + 1) / 16.0                          # x and y, exact
        x, y = (a.ravel() for a in np.meshgrid(steps, steps))
        inside = x + y <= N
        g1, g2 = (x[inside] / N).astype(F32), (y[inside] / N).astype(F32)
        i, j, ax, ay, pull, clamped = tr.lookup(g1, g2, N)
        assert pull.any() == (N > 1) and clamped.any() and (ax >= 0).all() and (ax <= 1).all() and (ay >= 0).all() and (ay <= 1).all()
        for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
            assert member[i + di, j + dj].all(), N
        if N > 1:
            i, j = tr.lookup(g1, g2, N, miss="no pull-back")[:2]
            assert not member[i + 1, j + 1].all()


def test_the_family_reaches_every_branch():
    """Counted over exactly what test_hip_mesh_texture.py compares bit for bit (DESIGN.md section 8 records the counts)."""
    total, differ = {}, 0
    for H, W in ti.SIZES:
        jobs, refused = _family(H, W)
        assert len(refused) >= 6
        for job in jobs:
            ref = job.reference(counters=total)
            job.render_reference(counters=total)
            if job.best and job.n > 1 and len(job.mem.faces) <= 2500:
                m = job.mem
                blend = tr.texture(m.verts, m.faces, m.colors, m.K, m.poses[:job.n], m.near, m.maps()[0][:job.n], m.images[:job.n],
                                   job.tolerance, job.min_cos, False, job.N, job.cells_per_row)
                assert blend[3] == ref[3]
                differ += int((blend[0] != ref[0]).any(axis=2).sum())
    print(f"family: {total}, {differ} texels differ between blend and best view")
    assert total["reached"] >= 1000 and total["fallen back"] >= 100
    assert total["gutter reached"] >= 100 and total["gutter fallen back"] >= 100
    assert differ >= 20
    assert total["pull-back"] >= 10 and total["corner clamp"] >= 10 and total["exchanged"] >= 100
    assert total["outside set"] == 0
    odd = {len(j.mem.faces) for H, W in ti.SIZES for j in _family(H, W)[0]}
    assert 1 in odd and sum(1 for F in odd if F % 2) >= 4


def test_every_named_near_miss_changes_some_result():
    cases = [(c, _maps(c)) for c in ti.hand_built()]
    for miss in tr.NEAR_MISSES:
        found = False
        for case, (depth, face) in cases:
            for N in (2, 3):
                ref = _texture(case, depth, N)
                got = _texture(case, depth, N, miss=miss, vertex_normals=case.normals)
                found = found or not np.array_equal(ref[0], got[0]) or not np.array_equal(ref[1], got[1]) or ref[3] != got[3]
                args = (case.verts, case.faces, ref[0], case.K, case.poses, case.near, depth, face, N)
                cnt = {}
                found = found or not np.array_equal(tr.render_texture(*args), tr.render_texture(*args, miss=miss, counters=cnt))
                # without the pull-back the fourth tap has weight 0, so the bytes agree: what changes is that it is read
                # from outside the face's set, another face's texel or none
                found = found or cnt["outside set"] > 0
        if not found:                                               # a curved mesh, where a vertex normal is not its face's
            import mesh_render_inputs as ri
            import mesh_volumes as mv
            v, f, c = mv.sphere_volume(11).extract()
            K, poses, near = ri.views_for(v, 6, 24, 32)
            depth = rr.render(v, f, K, poses, near, 24, 32)[0]
            args = (v, f, c, K, poses, near, depth, ti.ki.images_for(6, 24, 32, 5), near, 0.5, False, 2)
            ref, got = tr.texture(*args), tr.texture(*args, miss=miss, vertex_normals=cr.normals(v, f))
            found = not np.array_equal(ref[0], got[0]) or ref[3] != got[3]
        assert found, miss


# ---- the writer -----------------------------------------------------------------------------------------------

def _decode_png(data):
    """8-bit RGB, filter 0 on every row: the subset save_mesh_obj writes."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, bits, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (bits, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)


def test_save_mesh_obj_round_trip(tmp_path):
    from amvs.core.utils import save_mesh_obj
    case = ti.corner_sheet()
    depth, _ = _maps(case)
    for N, cpr, with_normals in ((3, 0, False), (8, 5, True), (1, 1, True)):
        atlas, uv, _, _ = _texture(case, depth, N, cpr)
        path = tmp_path / f"sheet{N}" / "mesh.obj"
        save_mesh_obj(case.verts, case.faces, uv, atlas, path, normals=case.normals if with_normals else None)
        image = _decode_png((path.parent / "mesh.png").read_bytes())
        assert np.array_equal(image, atlas)
        try:
            from PIL import Image
            assert np.array_equal(np.asarray(Image.open(path.parent / "mesh.png").convert("RGB")), atlas)
        except ImportError:
            pass
        mtl = (path.parent / "mesh.mtl").read_text().split("\n")
        assert "newmtl mesh" in mtl and "map_Kd mesh.png" in mtl
        rows = [ln.split() for ln in path.read_text().splitlines()]
        assert ["mtllib", "mesh.mtl"] in rows and ["usemtl", "mesh"] in rows
        v = np.array([r[1:] for r in rows if r[0] == "v"], np.float64).astype(F32)
        vt = np.array([r[1:] for r in rows if r[0] == "vt"], np.float64).astype(F32)
        vn = np.array([r[1:] for r in rows if r[0] == "vn"], np.float64).astype(F32).reshape(-1, 3)
        fs = [[[int(x) for x in corner.split("/")] for corner in r[1:]] for r in rows if r[0] == "f"]
        assert np.array_equal(v.view(np.uint32), case.verts.view(np.uint32)) and np.array_equal(vt.view(np.uint32), uv.reshape(-1, 2).view(np.uint32))
        assert len(vn) == (len(case.verts) if with_normals else 0) and len(fs) == len(case.faces)
        if with_normals:
            assert np.array_equal(vn.view(np.uint32), case.normals.view(np.uint32))
        Ht, Wt = atlas.shape[:2]
        cols = tr.layout(len(case.faces), N, cpr)[0]
        for f, corners in enumerate(fs):
            assert [c[0] - 1 for c in corners] == case.faces[f].tolist() and [c[1] - 1 for c in corners] == [3 * f, 3 * f + 1, 3 * f + 2]
            assert all(len(c) == (3 if with_normals else 2) and (not with_normals or c[2] == c[0]) for c in corners)
            for k, (i, j) in enumerate(((0, 0), (N, 0), (0, N))):
                u, w = (float(x) for x in vt[3 * f + k])
                # the pixel whose centre (+0.5) is at (u, 1 - v) of the image
                px, py = int(np.floor(u * Wt)), int(np.floor((1.0 - w) * Ht))
                assert abs(u * Wt - (px + 0.5)) < 1e-2 and abs((1.0 - w) * Ht - (py + 0.5)) < 1e-2
                X, Y = tr.atlas_position(np.array([f]), i, j, N, cols)
                assert (px, py) == (int(X[0]), int(Y[0])) and np.array_equal(image[py, px], atlas[Y[0], X[0]])
    with pytest.raises(ValueError, match="uv"):
        save_mesh_obj(case.verts, case.faces, uv[:-1], atlas, tmp_path / "bad.obj")
    with pytest.raises(ValueError, match="atlas"):
        save_mesh_obj(case.verts, case.faces, uv, atlas.astype(np.float32), tmp_path / "bad.obj")


# ---- the analytic sphere ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sphere():
    s = ti.sphere_scene()
    s["depth"], s["face"], _ = rr.render(s["v"], s["f"], s["K"], s["poses"], s["near"], s["H"], s["W"])
    return s


# Measured on the restatement: the largest texel error against the function at the texel's radial projection is
# 34.25 codes (mean 5.51).  Most of it is the bilinear sample of an image whose fine term (amplitude 35, period about
# four pixels) moves up to 35 * 2 pi / 4 = 55 codes per pixel.  The gate is that maximum plus one code for the final
# rounding and one for the half-voxel geometric error, the allowance of the colour section's gate (SPHERE_GATE there).
TEXEL_MAX = 34.25
TEXEL_GATE = TEXEL_MAX + 2


def test_the_texture_comes_closer_to_the_images_than_the_vertex_colours(sphere):
    """The claim of the texture: on a decimated mesh under images with detail inside a face, the textured render is nearer
    to the input images than the colour render of the recoloured vertices.  Mean absolute difference over the drawn
    pixels of the six views.  Measured: 19.78 codes with vertex colours, 7.18 with the texture at N = 8 (DESIGN.md section 8
    "Texture")."""
    s = sphere
    args = (s["K"], s["poses"], s["near"], s["depth"])
    colors = kr.color_views(s["v"], cr.normals(s["v"], s["f"]), s["c"], *args, s["images"], s["voxel"], 0.2, False)[0]
    flat = kr.render_color(s["v"], s["f"], colors, *args, s["face"])
    atlas, uv, n_texels, n_textured = tr.texture(s["v"], s["f"], colors, *args, s["images"], s["voxel"], 0.2, False, 8)
    pic = tr.render_texture(s["v"], s["f"], atlas, *args, s["face"], 8)
    drawn = s["face"] >= 0
    truth = s["images"][..., ::-1].astype(np.float64)

    def distance(p):
        return float(np.abs(p[drawn].astype(np.float64) - truth[drawn]).mean())

    by_vertex, by_texture = distance(flat), distance(pic)
    print(f"decimated sphere, {len(s['f'])} faces, {int(drawn.sum())} drawn pixels: mean absolute difference to the images "
          f"{by_vertex:.2f} codes with vertex colours, {by_texture:.2f} with the texture; {n_textured} of {n_texels} texels from the views")
    assert by_texture < by_vertex
    assert n_textured > 0.9 * n_texels

    # the texels a view reached (those that do not depend on the fall-back colours) against the analytic function
    other = tr.texture(s["v"], s["f"], 255 - colors, *args, s["images"], s["voxel"], 0.2, False, 8)[0]
    tex = tr.face_texels(8)
    F, T = len(s["f"]), len(tex)
    fi = np.repeat(np.arange(F), T)
    i, j = np.tile(tex[:, 0], F), np.tile(tex[:, 1], F)
    X, Y = tr.atlas_position(fi, i, j, 8, tr.layout(F, 8)[0])
    reached = (atlas[Y, X] == other[Y, X]).all(axis=1)
    assert abs(int(reached.sum()) - n_textured) <= 0.001 * n_textured         # a fall-back may equal its complement by chance
    c = s["v"].astype(np.float64)[s["f"]][fi]
    b1, b2 = i / 8.0, j / 8.0
    points = (1 - b1 - b2)[:, None] * c[:, 0] + b1[:, None] * c[:, 1] + b2[:, None] * c[:, 2]
    want = ti.sphere_colour(points)[:, ::-1]
    err = np.abs(atlas[Y, X].astype(np.float64) - np.clip(want, 0, 255))[reached]
    print(f"texels against the function at their radial projection: max {err.max():.2f} codes, mean {err.mean():.3f}")
    assert err.max() <= TEXEL_GATE


def test_reconstruct_mesh_refuses_a_bad_texel_count_before_any_work():
    import amvs
    from amvs.core.mvs_patchmatch import PatchMatchMVS
    camera = amvs.Camera(K=np.array([[30.0, 0, 16.0], [0, 30.0, 12.0], [0, 0, 1]]), dist=np.zeros(5))
    pm = PatchMatchMVS(camera, scale=1.0, patch_size=7, num_iterations=1, num_samples=2, min_views=2, seed=2, device=0)
    for bad in (-1, 65, 1000, 1.5, 8.5, "8", None, True, np.nan, np.inf, [8]):
        with pytest.raises(ValueError, match="texture_texels must be an integer in 0 .. 64"):
            pm.reconstruct_mesh(None, None, None, texture_texels=bad)

#!/usr/bin/env python3
"""Device time of the surface-mesh kernels (csrc/amvs_mesh.hip, csrc/amvs_mesh_fill.hip, csrc/amvs_mesh_clean.hip,
csrc/amvs_mesh_decimate.hip, csrc/amvs_mesh_render.hip, csrc/amvs_mesh_color.hip, csrc/amvs_mesh_texture.hip) at the CLI
operating point (run on the GPU box):
16 views at 1008 x 756, patch 11, the maps of the extended mode (the reference's algorithm leaves too few correct
depths for a surface) resident on the device, a 256^3 TSDF volume around the fused cloud.  Integration and extraction are timed separately with HIP events on the engine's stream (the extraction
includes its two count read-backs); the first-order bounds of DESIGN.md section 8 are printed next to them.
Then the hole filling (amvs_tsdf_fill) at 2 and 8 steps on that volume and on a 256^3 sphere with a tube unobserved, each the
median of 5 after a warm-up on a volume integrated or set again before every call, next to a first-order byte estimate (no
time gate: there is no earlier code to compare with).
Then the clean-up stage on that mesh and on the mesh of a 256^3 sphere: the vertex -> corner index, labelling + filter,
10 Taubin iterations and the normals, each the median of 5 after a warm-up, with a first-order byte estimate; the
decimation of either mesh at a cell of 2 voxels with either placement of the clusters' vertices (the mean, the quadrics),
likewise; the render of either mesh into the views (the scene's cameras; a ring of as many round the sphere) and the
visibility counts against it, before and after that decimation, next to a first-order estimate that prices the 64-bit
minimum atomics at the rate measured for float adds, which nobody has measured for them; the colours from the views
in both combine modes and the colour render against those maps (resident images, so no upload is timed: the scene's
own; noise round the sphere), next to
a first-order byte estimate (no time gate: there is no earlier code to compare with); the texture at 8 texels per leg in
both combine modes (the call alone, the atlas stays on the device) and the textured render, likewise; and
the labelling of a shuffled strip of 100 000 faces next to a sphere of about as many.

    python tools/mesh_time.py [n_views W H dim]
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import amvs  # noqa: E402,F401
from amvs.core.mvs_patchmatch import PatchMatchMVS  # noqa: E402
from amvs.synthetic import make_scene  # noqa: E402

n_views = int(sys.argv[1]) if len(sys.argv) > 1 else 16
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1008, 756)
dim = int(sys.argv[4]) if len(sys.argv) > 4 else 256
REPS = 5

sc = make_scene(n_views, H, W, device="cuda")
images = [{"image": np.ascontiguousarray(c)} for c in sc.colors]
pm = PatchMatchMVS(sc.camera, scale=1.0, patch_size=11, extended=True)
points, _, maps = pm._reconstruct_maps(images, sc.poses)
lo, hi = points.min(axis=0), points.max(axis=0)
side = float((hi - lo).max()) * 1.05
centre = 0.5 * (lo + hi)
voxel = side / (dim - 1)
origin = centre - 0.5 * side
dims = (dim, dim, dim)
trunc = 4.0 * voxel
ids, src = pm._mesh_inputs(maps)
poses = [(sc.poses[i].R, sc.poses[i].t) for i in ids]
eng = pm._engine
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t = time.time()
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), (time.time() - t) * 1e3, out


t_int, t_ext, w_int, w_ext = [], [], [], []
for rep in range(REPS + 1):
    ms, wall, _ = timed(lambda: eng.tsdf_integrate(pm.K_scaled, poses, pm.min_views, origin, voxel, dims, trunc, **src))
    ms2, wall2, mesh = timed(eng.tsdf_extract)
    if rep:                                   # the first round loads the code objects and grows the buffers
        t_int.append(ms); t_ext.append(ms2); w_int.append(wall); w_ext.append(wall2)
verts, faces, _ = mesh
tsdf, weight, _ = eng.tsdf_volume()
n_pts = dim ** 3
voxel_views = n_pts * len(ids)
observed = int((weight > 0).sum())
print(f"mesh_time: {len(ids)} maps {W}x{H}, patch 11 (extended mode), grid {dim}^3 = {n_pts:,} points (voxel {voxel:.4g}), "
      f"{observed:,} observed; mesh {len(verts):,} vertices, {len(faces):,} faces")
print(f"  integrate: median {np.median(t_int):.3f} ms device (min {min(t_int):.3f}, wall median {np.median(w_int):.3f} ms)")
print(f"  extract:   median {np.median(t_ext):.3f} ms device (min {min(t_ext):.3f}, wall median {np.median(w_ext):.3f} ms)")
# first-order bounds (estimates; MI355X peaks: 78.6 T FP32 VALU lane-operations/s (157.3 TFLOP/s counting an FMA as 2),
# 8 TB/s HBM)
valu_ms = voxel_views * 30 / 78.6e12 * 1e3
gather_ms = (voxel_views * 11 + n_pts * 20) / 8e12 * 1e3
ext_bytes = n_pts * (8 + 1 + 4 + 4 + 4) * 2 + n_pts * 8 * 2
print(f"  bounds (estimates): integrate VALU {valu_ms:.3f} ms / bytes {gather_ms:.3f} ms "
      f"({voxel_views:,} voxel-views x 30 VALU ops, x 11 B gathered + 20 B written per point); "
      f"extract streaming {ext_bytes / 8e12 * 1e3:.3f} ms ({ext_bytes / n_pts:.0f} B per point)")


# ---- clean-up (csrc/amvs_mesh_clean.hip) ----
sys.path.insert(0, "tests")
import mesh_clean_inputs as ci  # noqa: E402
import mesh_fill_inputs as fi  # noqa: E402
import mesh_volumes as mv  # noqa: E402


def fill_time(name, restore, n_points):
    """Hole filling (csrc/amvs_mesh_fill.hip) of the volume restore() makes, the whole call: the memset, the generations,
    the steps and the read-back of the counts."""
    for steps in (2, 8):
        ts = []
        for rep in range(REPS + 1):
            restore()
            ms, _, total = timed(lambda: eng.tsdf_fill(steps))
            if rep:
                ts.append(ms)
        frontier = sum(eng.last_fill_counts)
        # first order: the generations written once (4 B of weight in, 1 B out), then per step 1 B per point and about 50 B
        # per point filled (6 neighbour bytes, 5 floats of up to 6 neighbours served mostly by the cache, 21 B out).  An ESTIMATE.
        est = n_points * 5 + steps * n_points + frontier * 50
        print(f"hole filling of {name}, {steps} steps: {total:,} points filled {eng.last_fill_counts}: "
              f"median {np.median(ts):.3f} ms device (min {min(ts):.3f}); first-order bytes (estimate) {est / 1e6:.1f} MB = "
              f"{est / 8e12 * 1e3:.4f} ms at 8 TB/s, {est / 6.29e12 * 1e3:.4f} ms at the 6.29 TB/s a copy reaches")


def restore_scene_volume():
    eng.tsdf_integrate(pm.K_scaled, poses, pm.min_views, origin, voxel, dims, trunc, **src)


fill_time(f"the CLI operating point ({dim}^3)", restore_scene_volume, n_pts)
tube = fi.sphere_with_tube(256)[0]
fill_time("the 256^3 sphere without a tube", lambda: eng.tsdf_set_volume(*tube.arrays()), 256 ** 3)
del tube
restore_scene_volume()


def clean_times(name, restore, min_faces=8):
    """restore() makes the mesh current again (and drops its index).  The index is built by the first call that needs
    it, so its time is that of normals on a fresh topology minus normals with the index in place."""
    t = {k: [] for k in ("index", "label+filter", "pinned+1 it", "10 Taubin", "normals")}
    for rep in range(REPS + 1):
        nv, nf = restore()
        first, _, _ = timed(eng.mesh_normals)
        again, _, _ = timed(eng.mesh_normals)
        one, _, _ = timed(lambda: eng.mesh_smooth(1))
        ten, _, _ = timed(lambda: eng.mesh_smooth(10))
        restore()
        lab, _, counts = timed(lambda: eng.mesh_filter_components(min_faces))
        if rep:
            for k, x in zip(t, (first - again, lab, one, ten, again)):
                t[k].append(x)
    V, F = nv, nf
    est = {"index": 3 * F * 4 * (2 + 4 * 4) + V * 8,                   # counts + keys + ids, 4 radix passes in and out
           "label+filter": F * 12 * 3 + V * 4 * 4 + F * 8,              # hooks, flatten, face counts, keep flags + scan
           "pinned+1 it": 3 * F * (12 + 6 * 12) + 2 * (V * 6 * 2 * 12 + V * 24),
           "10 Taubin": 20 * (V * 6 * 2 * 12 + V * 6 * (4 + 12) + V * 24),  # per half-step: gathered positions, row, in + out
           "normals": F * (12 + 36 + 12) + V * (6 * 16 + 12)}
    print(f"clean-up of {name}: {V:,} vertices, {F:,} faces; filter at {min_faces} faces: {counts[0]:,} components, "
          f"{counts[2]:,} faces kept")
    for k in t:
        print(f"  {k:13s} median {np.median(t[k]):8.3f} ms device (min {min(t[k]):.3f}); first-order bytes (estimate) "
              f"{est[k] / 1e6:7.1f} MB = {est[k] / 8e12 * 1e3:.4f} ms at 8 TB/s")
    return t


def restore_volume():
    v, f, _ = eng.tsdf_extract()
    return len(v), len(f)


def decimate_time(name, restore, grid_origin, cell):
    """Decimation (csrc/amvs_mesh_decimate.hip) of the restored mesh at a cell of 2 voxels on the volume's origin."""
    ts, tq = [], []
    for rep in range(REPS + 1):
        V, F = restore()
        ms, _, counts = timed(lambda: eng.mesh_decimate(grid_origin, cell))
        restore()                                                 # a fresh topology: the quadric call builds its index
        mq, _, qcounts = timed(lambda: eng.mesh_decimate_quadric(grid_origin, cell))
        if rep:
            ts.append(ms); tq.append(mq)
    C, K = counts                                                 # clusters that stay, faces that stay
    live = max(F // 8, K)                                         # faces without a repeated id: first order, an eighth
    bits = max(int(np.ceil(np.log2(max(C, 2)))), 1)
    passes = (bits + 7) // 8
    est = (V * (12 + 12)                                          # positions in, key + id out
           + V * 12 * 2 * 8 + V * 8                               # 63-bit sort: 8 passes of (key, id) in and out, histogram
           + V * (8 + 4) + V * 8 + V * (4 + 4 + 4 + 4)            # heads, scan, cluster map
           + V * (4 + 15) + C * 15                                # representatives
           + F * (12 + 12 + 17) + F * 8 + live * 8                # triples, live flags + scan, live list
           + 3 * live * (8 * 2 * passes + 4 + 8)                  # three sorts of (key, face) and the keys' gathers
           + live * (4 + 13) + F * 4 + F * 8 + K * (12 + 12 + 12)  # decision, keep flags + scan, compaction
           + C * (4 + 4 + 15) + K * 24 + C * 15)                  # unused clusters: flags, scan, move, renumber
    print(f"decimation of {name} at 2 voxels: {V:,} vertices, {F:,} faces -> {C:,} / {K:,}: median {np.median(ts):.3f} ms device "
          f"(min {min(ts):.3f}); first-order bytes of the sorts and passes (estimate) {est / 1e6:.1f} MB = "
          f"{est / 8e12 * 1e3:.4f} ms at 8 TB/s")
    # what the quadric placement adds: the vertex -> corner index (clean_times' estimate), the face normals, the rows
    # walked once with the first vertex, the normal and the mean behind every corner, 36 B per vertex out and in
    extra = 3 * F * 4 * (2 + 4 * 4) + V * 8 + F * (12 + 36 + 12) + 3 * F * (4 + 4 + 12 + 12) + V * (4 + 12 + 36) + V * (4 + 36) + C * 24
    print(f"  with quadric placement ({qcounts[2]:,} of the clusters kept the mean): median {np.median(tq):.3f} ms device "
          f"(min {min(tq):.3f}), {np.median(tq) / np.median(ts):.2f} x the mean placement; first-order bytes it adds (estimate) "
          f"{extra / 1e6:.1f} MB = {extra / 8e12 * 1e3:.4f} ms at 8 TB/s")
    assert qcounts[:2] == counts


def render_time(name, restore, K, cams, near, tolerance, grid_origin, cell, colours):
    """Render (csrc/amvs_mesh_render.hip) of the restored mesh into `cams` and the visibility counts, then the same on
    the mesh decimated at 2 voxels: small faces first, faces of tens of pixels after.  The maps stay on the device."""
    for stage in ("as extracted", "decimated at 2 voxels"):
        tr, tv, tb, tk, tc = [], [], [], [], []
        for rep in range(REPS + 1):
            V, F = restore()
            if stage != "as extracted":
                V, F = eng.mesh_decimate(grid_origin, cell)
            r, _, skipped = timed(lambda: eng.mesh_render(K, cams, near=near, fetch=False))
            v, _, counts = timed(lambda: eng.mesh_visibility(tolerance))
            if rep:
                tr.append(r); tv.append(v)
        # the colours in a loop of their own, on the maps of the last round: the calls keep everything current, and the
        # colour render's 36 MB copy to the host stays out of the rounds that time the render and the counts
        eng.mesh_normals()                                            # keeps the maps
        for rep in range(REPS + 1):
            b, _, n_blend = timed(lambda: eng.mesh_color_views(tolerance, 0.2, False, **colours))
            k, _, n_best = timed(lambda: eng.mesh_color_views(tolerance, 0.2, True, **colours))
            c, _, _ = timed(lambda: eng.mesh_render_color(0, len(cams)))
            if rep:
                tb.append(b); tk.append(k); tc.append(c)
        # the texture likewise, after the colours (which drop it): N = 8, or the largest N whose atlas fits
        N = 8
        while N > 1 and int(np.ceil(np.sqrt((F + 1) // 2))) * (N + 3) > 16384:
            N -= 1
        tt, tu, tp = [], [], []
        for rep in range(REPS + 1):
            b, _, tex_blend = timed(lambda: texture_call(tolerance, N, False, colours))
            k, _, tex_best = timed(lambda: texture_call(tolerance, N, True, colours))
            c, _, _ = timed(lambda: eng.mesh_render_texture(0, len(cams)))
            if rep:
                tt.append(b); tu.append(k); tp.append(c)
        face = eng.mesh_render_fetch(0, len(cams))[1]
        covered = int((face >= 0).sum())
        pixels = face.size
        # first order: every covered pixel is hit by a front and a back face (2 atomics of 8 B) at the chip-wide rate
        # measured for FLOAT adds (about 1.3 TB/s of bytes; NOT measured for 64-bit integer minima), the key clear
        # (8 B per pixel) and the split (8 B in, 8 B out) stream at 8 TB/s
        est = 2 * covered * 8 / 1.3e12 * 1e3 + pixels * 24 / 8e12 * 1e3
        vis = (V * (12 + 4) + V * len(cams) * 4) / 8e12 * 1e3
        print(f"render of {name}, {stage}: {V:,} vertices, {F:,} faces into {len(cams)} views of {W}x{H}, {covered:,} of "
              f"{pixels:,} pixels covered, {int(skipped.sum()):,} (view, face) pairs skipped; {int((counts > 0).sum()):,} vertices seen")
        print(f"  render     median {np.median(tr):8.3f} ms device (min {min(tr):.3f}); first-order estimate {est:.4f} ms "
              f"(atomics at the float-add rate, unmeasured for integer minima): {np.median(tr) / est:.1f} x")
        print(f"  visibility median {np.median(tv):8.3f} ms device (min {min(tv):.3f}); first-order bytes (estimate) {vis:.4f} ms "
              f"at 8 TB/s")
        # first order, per (vertex, view): the projection is arithmetic, four 4-byte depths and twelve colour bytes are
        # read, as if every pair passed every test; per vertex position, normal and colour.  An ESTIMATE at 8 TB/s.
        col = (V * (12 + 12 + 3) + V * len(cams) * (4 * 4 + 12)) / 8e12 * 1e3
        # the colour render: face id and depth in, three corners' positions and colours gathered, 3 bytes out; the
        # picture then crosses to the host (included in the time, not in the estimate)
        pic = (pixels * (4 + 4 + 3) + covered * (12 + 3 * (12 + 3))) / 8e12 * 1e3
        for label, t, n in (("blend", tb, n_blend), ("best view", tk, n_best)):
            print(f"  colours, {label:9s} median {np.median(t):8.3f} ms device (min {min(t):.3f}), {n:,} of {V:,} vertices recoloured; "
                  f"first-order bytes (estimate) {col:.4f} ms at 8 TB/s")
        print(f"  colour render      median {np.median(tc):8.3f} ms device with the copy of {pixels * 3 / 1e6:.1f} MB to the host "
              f"(min {min(tc):.3f}); first-order device bytes (estimate) {pic:.4f} ms at 8 TB/s")
        # first order, per texel: the face's ids, three corner positions and colours (served by the cache within a face, priced
        # as if not) and 3 bytes out; per (texel, view) pair the 28 B the colours count; per atlas slot 3 bytes.  An ESTIMATE.
        wt, ht, T = tex_blend[0], tex_blend[1], tex_blend[2]
        tex = (T * (12 + 3 * (12 + 3) + 3) + T * len(cams) * (4 * 4 + 12) + wt * ht * 3) / 8e12 * 1e3
        # the textured render: face id and depth in, three corners' positions gathered, four texels of 3 bytes, 3 bytes out
        tpic = (pixels * (4 + 4 + 3) + covered * (12 + 3 * 12 + 4 * 3)) / 8e12 * 1e3
        for label, t, r in (("blend", tt, tex_blend), ("best view", tu, tex_best)):
            print(f"  texture N={N}, {label:9s} median {np.median(t):8.3f} ms device (min {min(t):.3f}), atlas {wt} x {ht}, {r[3]:,} of "
                  f"{T:,} texels from the views; first-order bytes (estimate) {tex:.4f} ms at 8 TB/s")
        print(f"  textured render    median {np.median(tp):8.3f} ms device with the copy of {pixels * 3 / 1e6:.1f} MB to the host "
              f"(min {min(tp):.3f}); first-order device bytes (estimate) {tpic:.4f} ms at 8 TB/s")


def texture_call(tolerance, N, best, colours):
    """amvs_mesh_texture alone, from resident images: the atlas and the UVs stay on the device.  Returns (width, height,
    n_texels, n_textured)."""
    import ctypes as C
    ids = np.ascontiguousarray(colours["view_ids"], np.int32)
    wt, ht, total, done = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
    eng._chk(eng._lib.amvs_mesh_texture(eng._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), None, float(np.float32(tolerance)), 0.2,
                                        int(best), N, 0, C.byref(wt), C.byref(ht), C.byref(total), C.byref(done)))
    return wt.value, ht.value, total.value, done.value


def resident_images(images_bgr):
    """The images into the engine's colour slots 0 .. n-1 (outside any timed call): mesh_color_views then reads resident
    images and its time holds no host-to-device copy."""
    for j, img in enumerate(images_bgr):
        eng.set_view_colors(j, img)
    return dict(view_ids=list(range(len(images_bgr))))


def ring_of_cameras(n, distance=3.0):
    """n cameras round the origin looking at it, on a tilted ring: (R, t) with R's rows the camera's axes."""
    out = []
    for a in np.arange(n) * 2 * np.pi / n:
        eye = distance * np.array([np.cos(a) * 0.9, np.sin(a) * 0.9, np.sqrt(1 - 0.81) * np.cos(3 * a)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        out.append((R, -R @ eye))
    return out


clean_times(f"the CLI operating point ({dim}^3)", restore_volume)
decimate_time(f"the CLI operating point ({dim}^3)", restore_volume, origin, 2.0 * voxel)
scene_colours = dict(view_ids=src["view_ids"]) if "view_ids" in src else resident_images(src["colors_bgr"])
render_time(f"the CLI operating point ({dim}^3)", restore_volume, pm.K_scaled, poses, voxel, voxel, origin, 2.0 * voxel, scene_colours)
sphere = mv.sphere_volume(256, radius=0.8)
eng.tsdf_set_volume(*sphere.arrays())
clean_times("the 256^3 sphere", restore_volume)
decimate_time("the 256^3 sphere", restore_volume, sphere.origin, 2.0 * float(sphere.voxel))
K_sphere = np.array([[0.9 * H, 0, W / 2.0], [0, 0.9 * H, H / 2.0], [0, 0, 1]])
noise = resident_images(np.random.default_rng(1).integers(0, 256, (len(poses), H, W, 3), dtype=np.uint8))
render_time("the 256^3 sphere", restore_volume, K_sphere, ring_of_cameras(len(poses)), 0.1, float(sphere.voxel), sphere.origin,
            2.0 * float(sphere.voxel), noise)


def label_time(name, restore):
    ts = []
    for rep in range(REPS + 1):
        nv, nf = restore()
        ms, _, counts = timed(eng.mesh_filter_components)
        if rep:
            ts.append(ms)
    print(f"labelling of {name}: {nf:,} faces, {counts[0]} component(s): median {np.median(ts):.3f} ms (min {min(ts):.3f})")


strip = ci.strip()


def restore_strip():
    eng.mesh_set(*strip.arrays())
    return len(strip.verts), len(strip.faces)


label_time("the shuffled strip", restore_strip)
small_sphere = mv.sphere_volume(76, radius=0.8, trunc=0.1)
eng.tsdf_set_volume(*small_sphere.arrays())
label_time("a 76^3 sphere", restore_volume)
eng.set_stream(None)

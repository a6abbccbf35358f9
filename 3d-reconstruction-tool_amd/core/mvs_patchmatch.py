"""PatchMatch multi-view stereo: host side of the MI355X backend.

Mirrors the call surface of the reference's src/core/mvs_patchmatch.py
(`PatchMatchMVS(camera, scale, patch_size, num_iterations, num_samples, min_views,
depth_min, depth_max).reconstruct(images, poses, sparse_points) -> (points, colors)`,
reference :43-50, :72-74) so `run_reconstruction.py --mvs` can import this class
instead.  The per-pixel sweep (`_patchmatch_cuda`, reference :225-321) runs in the
gfx950 kernels behind libamvs.so; everything kept here is the small float64 host
geometry around it (depth range :141-165, source selection :193-223, fusion :536-570,
filtering :572-588).

Differences a caller can observe, all opt-in or performance-only:
  * every view is uploaded once and all reference views are swept in batches
    (the reference re-uploads per view and loops serially, :104-123, :235-257);
  * `seed` names the RNG streams (the reference is unseeded);
  * `mode` selects the arithmetic of the sweep kernels: "exact" reproduces the reference's float32
    operation sequence (bit-identical to the tests' CPU restatement, which matches torch-CPU up to
    the box filter's summation order; the default), "fast" is the tolerance mode of include/amvs.h
    AMVS_MODE_FAST (what bench.py times) -- measured against the reference's golden vectors it
    agrees exactly as well as "exact" does;
  * under an initialised torch.distributed process group the reference views are
    sharded over ranks and the per-view maps are all-gathered (see ..parallel);
  * with `device_fusion` (default) and torch-ROCm present the per-view maps never leave
    the GPU: the sweep writes them into device tensors, the all-gather (RCCL) and the
    fusion + filter read them there, and only the final cloud is copied to the host.
"""
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from .camera import Camera, CameraPose
from .utils import nearest_map_neighbours, rows_matmul
from .view_cache import ResidentViews
from .. import engine as _engine
from .. import parallel as _parallel


@dataclass
class DepthNormalMap:
    """Per-view result (reference :30-35)."""
    depth: np.ndarray       # (H, W) float32
    normal: np.ndarray      # (H, W, 3) float32
    confidence: np.ndarray  # (H, W) float32, number of photo-consistent source views


@dataclass
class _ResidentMaps:
    """Maps of all swept views kept on the GPU (torch tensors), rows in job order."""
    ref_ids: list            # reference view index per row
    depth: object            # (n, H*W) float32
    normal: object           # (n, H*W*3) float32
    confidence: object       # (n, H*W) float32
    shape: tuple

    def to_host(self):
        H, W = self.shape
        d, n, c = self.depth.cpu().numpy(), self.normal.cpu().numpy(), self.confidence.cpu().numpy()
        return {r: DepthNormalMap(depth=d[i].reshape(H, W), normal=n[i].reshape(H, W, 3),
                                  confidence=c[i].reshape(H, W)) for i, r in enumerate(self.ref_ids)}


def _print_view_progress(cam_indices, ref_idx, valid, per_view):
    print(f"  [{cam_indices.index(ref_idx)+1}/{len(cam_indices)}] Cam {ref_idx}: {int(valid):,} valid pixels ({per_view:.1f}s)")


class PatchMatchMVS(ResidentViews):
    NUM_SOURCES = 4          # reference :108

    def __init__(self, camera: Camera, scale: float = 0.25, patch_size: int = 11,
                 num_iterations: int = 3, num_samples: int = 8, min_views: int = 3,
                 depth_min: float = 0.1, depth_max: float = 100.0, *,
                 seed: int = 0, device: Optional[int] = None, views_per_batch: int = 16,
                 process_group=None, device_fusion: bool = True, mode: str = "exact",
                 device_prep: Optional[bool] = None, extended: bool = False, gather_normals: bool = True,
                 undistort: bool = False):
        super().__init__(device_prep, undistort)     # the resident-view cache, the device_prep default, the lens switch
        self.camera = camera
        if self.undistort:
            self._lens()                         # (an unsupported distortion model is refused here, not at the first call)
        self.scale = scale
        self.patch_size = patch_size
        self.num_iterations = num_iterations
        self.num_samples = num_samples
        self.min_views = min_views
        self.depth_min = depth_min
        self.depth_max = depth_max
        self.seed = seed
        self.views_per_batch = max(1, int(views_per_batch))
        self.process_group = process_group
        self.device_fusion = device_fusion
        # several ranks: also all-gather the normal maps (12 of the 20 B/pixel; north_star's exchange).
        # reconstruct() itself fuses depth and confidence only (reference :536-570).
        self.gather_normals = gather_normals
        # Extended mode (off by default, NO reference counterpart -- the reference's docstring names view
        # propagation and plane normals, :1-13, its code implements neither): slanted-plane cost,
        # red-black propagation, view propagation fed by the other views' maps (all-gathered between
        # iterations on several GPUs), geometric-consistency confidence.  Judged against ground truth.
        self.extended = extended
        if mode not in ("exact", "fast"):
            raise ValueError("mode must be 'exact' or 'fast'")
        self.mode = mode
        self.device_id = _parallel.local_device() if device is None else int(device)
        print(f"PatchMatch MVS using GPU: HIP device {self.device_id} (gfx950 kernels)")
        # scaled intrinsics: first two rows times `scale` (reference :69-70)
        self.K_scaled = camera.K.copy()
        self.K_scaled[:2] *= scale
        self.last_timing = None
        self.last_mesh_grid = None       # (origin, voxel, dims, trunc) of the last reconstruct_mesh
        self.last_mesh_views = None      # ... and the views it fused, in map order
        # run the multi-rank code path -- row groups, second stream, collectives -- on a one-rank process group
        # as well; how the RCCL calls are rehearsed on a one-GPU box
        self.exercise_exchange = False
        self._streams = None             # (device, sweep stream, exchange stream) of _exchange_streams
        self._cloud_resident = False
        self._filter_threshold = None    # filter_min_views while the maps of the last call are the geometric filter's

    def _threshold(self):
        """What a pixel's confidence must reach to be used by the fusion, the TSDF and the normals: min_views, or -- when the
        maps at hand are the (depth, count) of the geometric filter -- its filter_min_views."""
        held = getattr(self, "_filter_threshold", None)
        return self.min_views if held is None else held

    # ------------------------------------------------------------------ public ----
    def reconstruct(self, images: List[dict], poses: Dict[int, CameraPose],
                    sparse_points: np.ndarray = None, *, with_normals: bool = False, normal_radius: int = 2,
                    normal_jump: float = 0.05, normal_depth_tolerance: float = 0.01, geometric_filter: bool = False,
                    filter_px: float = 1.0, filter_rel: float = 0.01, filter_min_views: int = 2, filter_refine: bool = True,
                    filter_neighbours: Optional[int] = None) -> Tuple[np.ndarray, ...]:
        """(points, colors) as the reference returns them.  with_normals=True appends oriented unit normals (N,3) float32
        of the final cloud (csrc/amvs_cloud_normals.hip, include/amvs.h amvs_cloud_normals; no reference counterpart): per
        view a plane is fitted to the inverse depths in a window of normal_radius pixels around every pixel with
        confidence >= min_views, over the neighbours whose depth is within normal_jump of the centre's, and every point
        takes the cosine-weighted mean of the normals of the views that see it within normal_depth_tolerance (relative).
        A point no view gives a normal keeps (0, 0, 0).

        geometric_filter=True (off by default: the call is then exactly what it was) checks the depth maps against each
        other between the sweep and the fusion (csrc/amvs_depth_filter.hip, include/amvs_depth.h amvs_depth_filter; no
        reference counterpart): a pixel with confidence >= min_views keeps its depth only if at least filter_min_views other
        maps agree with it after forward-backward reprojection -- the reprojected pixel within filter_px pixels, the
        reprojected depth within filter_rel (relative) -- and with filter_refine it becomes the mean of its own and the
        agreeing depths.  filter_neighbours: None compares every map with every other one, an int k with the k nearest
        camera centres among the views that have a map (core.utils.nearest_map_neighbours).  The fusion and the normals then
        read the filtered depths and the counts, with filter_min_views as their threshold in place of min_views.  In the
        extended mode the filter runs after that mode's own consistency step, on its maps."""
        if with_normals:
            _, world = _parallel.rank_world(self.process_group)
            if world > 1:
                raise NotImplementedError("with_normals runs on one process: normals with a process group of "
                                          f"{world} ranks are not implemented (call it without a process group)")
        gfilter = self._filter_arguments(geometric_filter, filter_px, filter_rel, filter_min_views, filter_refine, filter_neighbours)
        points, colors, maps = self._reconstruct_maps(images, poses, sparse_points, gfilter)
        if not with_normals:
            return points, colors
        return points, colors, self._cloud_normals(points, colors, maps, poses, normal_radius, normal_jump, normal_depth_tolerance)

    def _filter_arguments(self, geometric_filter, px, rel, min_views, refine, neighbours):
        """None, or (filter_px, filter_rel, filter_min_views, filter_refine, filter_neighbours) of a call with
        geometric_filter=True, which runs on one process."""
        if not geometric_filter:
            return None
        _, world = _parallel.rank_world(self.process_group)
        if world > 1:
            raise NotImplementedError("geometric_filter runs on one process: filtering across a process group of "
                                      f"{world} ranks is not implemented (call it without a process group)")
        if isinstance(min_views, (bool, np.bool_)) or int(min_views) != min_views or min_views < 1:
            raise ValueError("filter_min_views must be an integer of at least 1")
        return float(px), float(rel), int(min_views), bool(refine), neighbours

    def _cloud_normals(self, points, colors, maps, poses, radius, jump, depth_tolerance):
        """Normals of the final cloud from the maps _reconstruct_maps returned.  The cloud is the engine's resident one
        wherever the fusion ran on the device; the host fusion's cloud is uploaded first."""
        if maps is None or len(points) == 0:
            return np.zeros((len(points), 3), np.float32)       # (one row per point, whatever the early exit)
        t0 = time.time()
        kind, data, _ = maps
        if kind == "resident":
            ids = list(data.ref_ids)
            import torch
            torch.cuda.synchronize(data.depth.device)
            where = dict(device_ptrs=(data.depth.data_ptr(), data.confidence.data_ptr()))
        else:
            ids = list(data)
            where = dict(depth=np.stack([data[i].depth for i in ids]), conf=np.stack([data[i].confidence for i in ids])) if ids else {}
        if not ids:
            return np.zeros((len(points), 3), np.float32)
        eng = self._engine
        if not self._cloud_resident:
            eng.cloud_set(points, colors)
        _, n_points = eng.cloud_normals(self.K_scaled, [(poses[i].R, poses[i].t) for i in ids], self._threshold(), radius, jump, 3,
                                        depth_tolerance, 1, **where)
        normals, _ = eng.fetch_cloud_normals(len(points))
        print(f"  Normals: {n_points:,} of {len(points):,} points from {len(ids)} views ({time.time() - t0:.2f}s)")
        return normals

    def reconstruct_mesh(self, images: List[dict], poses: Dict[int, CameraPose], sparse_points: np.ndarray = None, *,
                         voxel_size: Optional[float] = None, bounds=None, trunc_voxels: float = 4.0,
                         max_dim: int = 256, min_component_faces: int = 0, keep_largest: bool = False,
                         smooth_iterations: int = 0, smooth_lambda: float = 0.5, smooth_mu: float = -0.53,
                         fix_boundary: bool = True, with_normals: bool = False,
                         decimate_voxels: float = 0.0, decimate_placement: str = "mean",
                         decimate_regularisation: float = 1e-3, min_visible_views: int = 0,
                         visibility_tolerance_voxels: float = 1.0, color_from_views: bool = False,
                         color_min_cos: float = 0.2, color_best_view: bool = False,
                         texture_texels: int = 0, fill_holes_voxels: int = 0,
                         fill_min_neighbours: int = 1, geometric_filter: bool = False, filter_px: float = 1.0,
                         filter_rel: float = 0.01, filter_min_views: int = 2, filter_refine: bool = True,
                         filter_neighbours: Optional[int] = None) -> Tuple[np.ndarray, ...]:
        """Surface mesh of the scene: reconstruct()'s preparation, sweep and fusion, then the per-view depth maps
        fused into a truncated signed distance volume and its zero level set extracted by marching tetrahedra on
        the GPU (csrc/amvs_mesh.hip; no reference counterpart).  Returns (vertices (V,3) float32, faces (F,3) int32,
        colors (V,3) uint8 RGB); face normals point toward the cameras.

        bounds: ((xmin, ymin, zmin), (xmax, ymax, zmax)) of the volume; default the fused cloud's box padded by the
        truncation distance.  voxel_size: default the longest side / (max_dim - 1).  The truncation distance is
        trunc_voxels * voxel_size.  The volume holds at most AMVS_TSDF_MAX_POINTS grid points (include/amvs.h).

        fill_holes_voxels=N > 0 (an integer up to 64; 2 to 4 is the recommended range) fills holes between the fusion and
        the extraction (csrc/amvs_mesh_fill.hip, Engine.tsdf_fill): in N steps the signed distance and the colour grow from
        the observed grid points into the unobserved ones next to them, each new point the mean of its observed or
        already filled 6-neighbours, and the extraction then meshes them like any other.  It is for the holes that
        unsure pixels leave in a surface that is otherwise seen (glossy or texture-less patches, thin occlusions): it
        closes holes up to about 2 N voxels wide that observed surface surrounds.  It is no surface completion.  It also
        advances every open border of the observed surface by up to N voxels, and where whole sides of an object were
        never seen it invents a closing surface there: a sphere of radius 0.8 seen from three of six axis views is
        closed after 8 steps by a surface with 1 089 vertices more than 2 voxels off the sphere, the worst 0.45 off.
        fill_min_neighbours (1 .. 6, default 1) is the number of observed or filled neighbours a point needs to be
        filled: with 2 a flat front no longer advances while pockets still fill (274 such vertices and 0.31 in that
        scene, which then stays open).  Every clean-up step below sees the filled mesh; min_visible_views removes
        what no view sees of it again.

        Clean-up on the device (csrc/amvs_mesh_clean.hip), in this order and each only when asked for:
        min_visible_views > 0 renders the mesh into the views that were fused (csrc/amvs_mesh_render.hip; near plane one
        voxel), counts for every vertex the views that see it -- in the image and not behind the rendered surface by
        more than float32(visibility_tolerance_voxels) * float32(voxel_size) -- and keeps the faces whose three vertices
        each reach min_visible_views: the inner sheets and back sides behind the observed surface go, and what that
        detaches is left to the component filter that follows;
        min_component_faces > 0 drops the connected components with fewer faces and keep_largest all but the one with
        the most; smooth_iterations > 0 runs that many Taubin lambda | mu iterations (smooth_lambda, smooth_mu;
        fix_boundary keeps the vertices on open edges where they are); decimate_voxels > 0 decimates by vertex
        clustering (csrc/amvs_mesh_decimate.hip) on cells of float32(decimate_voxels) * float32(voxel_size) that sit on
        the volume's origin: one vertex per cell, and the faces that collapse or cancel go (a twelfth stay at 2);
        decimate_placement="mean" puts that vertex at the mean of the cell's vertices, "quadric" where the planes of
        their faces meet best (Engine.mesh_decimate_quadric with decimate_regularisation; same faces and colours, a
        smaller error on curved surfaces and at edges);
        color_from_views=True then colours the final mesh from the images (csrc/amvs_mesh_color.hip): the normals, a
        render into the fused views with near plane one voxel, and for every vertex the bilinear samples of the views that
        see it within float32(visibility_tolerance_voxels) * float32(voxel_size) at a cosine above color_min_cos, blended
        with the cosine as weight or, with color_best_view, taken from the most frontal view; a vertex no view reaches
        keeps the volume's colour;
        texture_texels=N > 0 (an integer up to 64) then textures the final mesh (csrc/amvs_mesh_texture.hip): a render into
        the fused views with near plane one voxel, and a per-face atlas with N texel intervals per triangle leg, every
        texel coloured like a vertex above, with the same tolerance, images, color_min_cos and color_best_view, and from
        the vertex colours where no view reaches it; uv (F,3,2) float32 and atlas (Ht,Wt,3) uint8 RGB are appended to the
        result, after the normals if those were asked for (core.utils.save_mesh_obj writes them);
        with_normals=True appends area-weighted vertex normals (V,3) float32 to the result, a 4-tuple then.  With the
        defaults none of it runs.  geometric_filter and the filter_* keywords are reconstruct()'s: the cloud that sizes the
        volume and the maps the volume fuses are then the filtered ones, with filter_min_views as the TSDF's threshold.
        The grid of the last call is kept in last_mesh_grid (origin, voxel, dims, trunc), the views
        it fused in last_mesh_views."""
        rank, world = _parallel.rank_world(self.process_group)
        if world > 1:
            raise NotImplementedError("reconstruct_mesh runs on one process: meshing with a process group of "
                                      f"{world} ranks is not implemented (call it without a process group)")
        if trunc_voxels <= 0:
            raise ValueError("trunc_voxels must be positive")
        if smooth_iterations < 0:
            raise ValueError("smooth_iterations must not be negative")
        if not (np.isfinite(decimate_voxels) and decimate_voxels >= 0):
            raise ValueError("decimate_voxels must be finite and not negative")
        if decimate_placement not in ("mean", "quadric"):
            raise ValueError(f"decimate_placement must be 'mean' or 'quadric', not {decimate_placement!r}")
        try:
            whole = not isinstance(min_visible_views, bool) and int(min_visible_views) == min_visible_views
        except (TypeError, ValueError, OverflowError):
            whole = False
        if not whole or min_visible_views < 0:
            raise ValueError("min_visible_views must be an integer and not negative")
        if not (np.isfinite(visibility_tolerance_voxels) and visibility_tolerance_voxels >= 0):
            raise ValueError("visibility_tolerance_voxels must be finite and not negative")
        for name, flag in (("color_from_views", color_from_views), ("color_best_view", color_best_view)):
            if not isinstance(flag, (bool, np.bool_)):
                raise ValueError(f"{name} must be a bool")
        try:
            cos_ok = not isinstance(color_min_cos, bool) and 0.0 <= float(color_min_cos) < 1.0
        except (TypeError, ValueError):
            cos_ok = False
        if not cos_ok:
            raise ValueError("color_min_cos must lie in [0, 1)")
        try:
            texels_ok = (not isinstance(texture_texels, (bool, np.bool_)) and int(texture_texels) == texture_texels
                         and 0 <= texture_texels <= 64)
        except (TypeError, ValueError, OverflowError):
            texels_ok = False
        if not texels_ok:
            raise ValueError("texture_texels must be an integer in 0 .. 64")
        texture = int(texture_texels) > 0
        for name, value, lo, hi in (("fill_holes_voxels", fill_holes_voxels, 0, 64),
                                    ("fill_min_neighbours", fill_min_neighbours, 1, 6)):
            try:
                ok = not isinstance(value, (bool, np.bool_)) and int(value) == value and lo <= value <= hi
            except (TypeError, ValueError, OverflowError):
                ok = False
            if not ok:
                raise ValueError(f"{name} must be an integer in {lo} .. {hi}")
        fill = int(fill_holes_voxels)
        gfilter = self._filter_arguments(geometric_filter, filter_px, filter_rel, filter_min_views, filter_refine, filter_neighbours)
        points, _, maps = self._reconstruct_maps(images, poses, sparse_points, gfilter)
        do_filter = min_component_faces > 0 or keep_largest
        empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8))
        if with_normals:
            empty += (np.zeros((0, 3), np.float32),)
        if texture:
            empty += (np.zeros((0, 3, 2), np.float32), np.zeros((0, 0, 3), np.uint8))
        if maps is None or (bounds is None and len(points) == 0):
            return empty
        origin, voxel, dims, trunc = self._mesh_grid(points, bounds, voxel_size, trunc_voxels, max_dim)
        self.last_mesh_grid = (origin, voxel, dims, trunc)
        print(f"\nMeshing: {dims[0]} x {dims[1]} x {dims[2]} TSDF grid, voxel {voxel:.4g}, truncation {trunc:.4g}")
        t0 = time.time()
        ids, src = self._mesh_inputs(maps)
        if not ids:
            return empty
        fused = [(poses[i].R, poses[i].t) for i in ids]
        self.last_mesh_views = None
        if fill > 0:
            self._engine.tsdf_integrate(self.K_scaled, fused, self._threshold(), origin, voxel, dims, trunc, **src)
            n_filled = self._engine.tsdf_fill(fill, int(fill_min_neighbours))
            verts, faces, colors = self._engine.tsdf_extract()
        else:
            verts, faces, colors = self._engine.tsdf_mesh(self.K_scaled, fused, self._threshold(), origin, voxel, dims, trunc, **src)
        self.last_mesh_views = list(ids)
        print(f"  Mesh: {len(verts):,} vertices, {len(faces):,} faces ({time.time() - t0:.2f}s)")
        decimate = decimate_voxels > 0
        cull = min_visible_views > 0
        if not (cull or do_filter or smooth_iterations > 0 or with_normals or decimate or color_from_views or texture):
            if fill > 0:
                print(f"  Clean-up: filled {n_filled:,} grid points in {fill} steps (its time is the mesh's)")
            return verts, faces, colors
        t0 = time.time()
        eng = self._engine
        n_comp, n_faces = 0, len(faces)
        if cull:
            eng.mesh_render(self.K_scaled, fused, near=np.float32(voxel))
            eng.mesh_visibility(np.float32(visibility_tolerance_voxels) * np.float32(voxel))
            n_faces = eng.mesh_filter_visible(int(min_visible_views))[1]
            culled = f"visibility >= {int(min_visible_views)} views: {len(faces):,} faces -> {n_faces:,}"
        if do_filter:
            n_comp, _, n_faces = eng.mesh_filter_components(min_component_faces, keep_largest)
        if smooth_iterations > 0:
            eng.mesh_smooth(smooth_iterations, smooth_lambda, smooth_mu, fix_boundary)
        filtered = None
        if decimate:
            # the labels do not survive the decimation: what the line says of the filter is taken before it
            filtered = (len(np.unique(eng.mesh_fetch(labels=True)[-1])) if do_filter else 0, n_faces)
            cell = np.float32(decimate_voxels) * np.float32(voxel)
            if decimate_placement == "quadric":
                kept_mean = eng.mesh_decimate_quadric(np.asarray(origin, np.float64).astype(np.float32), cell,
                                                      decimate_regularisation)[2]
            else:
                eng.mesh_decimate(np.asarray(origin, np.float64).astype(np.float32), cell)
        if with_normals or color_from_views:
            eng.mesh_normals()
        if color_from_views:
            eng.mesh_render(self.K_scaled, fused, near=np.float32(voxel), fetch=False)
            images_of = {k: src[k] for k in ("view_ids", "colors_bgr") if k in src}
            n_colored = eng.mesh_color_views(np.float32(visibility_tolerance_voxels) * np.float32(voxel), color_min_cos,
                                             color_best_view, **images_of)
        if texture:
            if not color_from_views:
                eng.mesh_render(self.K_scaled, fused, near=np.float32(voxel), fetch=False)
            images_of = {k: src[k] for k in ("view_ids", "colors_bgr") if k in src}
            atlas, uv, n_textured = eng.mesh_texture(np.float32(visibility_tolerance_voxels) * np.float32(voxel), int(texture_texels),
                                                     color_min_cos, color_best_view, **images_of)
        out = eng.mesh_fetch(normals=with_normals, labels=do_filter and not decimate)
        line = [f"filled {n_filled:,} grid points in {fill} steps"] if fill > 0 else []
        if cull:
            line.append(culled)
        if do_filter and decimate:
            line.append(f"{n_comp:,} components -> {filtered[0]:,}, {filtered[1]:,} faces")
        elif do_filter:
            line.append(f"{n_comp:,} components -> {len(np.unique(out[-1])):,}, {len(out[1]):,} faces")
            out = out[:-1]
        if smooth_iterations > 0:
            line.append(f"{smooth_iterations} Taubin iterations")
        if decimate:
            how = f", quadric placement ({kept_mean:,} kept the mean)" if decimate_placement == "quadric" else ""
            line.append(f"decimation at {decimate_voxels:g} voxels{how}: {filtered[1]:,} faces -> {len(out[1]):,}")
        if color_from_views:
            line.append(f"colours from {len(fused)} views: {n_colored:,} of {len(out[0]):,} vertices")
        if texture:
            line.append(f"texture {int(texture_texels)} texels, {atlas.shape[1]} x {atlas.shape[0]}: {n_textured:,} of "
                        f"{eng.last_texture_texels:,} texels from the views")
            out = out + (uv, atlas)
        if with_normals:
            line.append("normals")
        print(f"  Clean-up: {', '.join(line)} ({time.time() - t0:.2f}s)")
        return out

    def _mesh_inputs(self, maps):
        """(view indices, Engine.tsdf_integrate keyword arguments) of the maps _reconstruct_maps returned: the device
        tensors or the host maps, and the resident colour images where the engine holds them."""
        kind, data, proc_images = maps
        if kind == "resident":
            ids = list(data.ref_ids)
            import torch
            torch.cuda.synchronize(data.depth.device)
            src = dict(device_ptrs=(data.depth.data_ptr(), data.confidence.data_ptr(), len(ids)))
        else:
            ids = list(data)
            if not ids:
                return ids, {}
            src = dict(depth=np.stack([data[i].depth for i in ids]), conf=np.stack([data[i].confidence for i in ids]))
        if self._resident_colors and proc_images is self._engine_images:
            src["view_ids"] = [self._slot[i] for i in ids]
        else:
            src["colors_bgr"] = np.stack([proc_images[i]["color"] for i in ids])
        return ids, src

    @staticmethod
    def _mesh_grid(points, bounds, voxel_size, trunc_voxels, max_dim):
        """(origin, voxel, dims (nx, ny, nz), trunc) of reconstruct_mesh's volume."""
        tv = float(trunc_voxels)
        if bounds is None:
            lo, hi = points.min(axis=0).astype(np.float64), points.max(axis=0).astype(np.float64)
            if voxel_size is None:
                # the padded box's longest side (longest + 2 trunc) spans max_dim - 1 voxels
                room = int(max_dim) - 1 - 2.0 * tv
                if room <= 0:
                    raise ValueError(f"max_dim {max_dim} leaves no room inside the {tv}-voxel truncation band")
                voxel = float((hi - lo).max()) / room
            else:
                voxel = float(voxel_size)
            lo, hi = lo - tv * voxel, hi + tv * voxel
        else:
            lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
            if not np.all(hi > lo):
                raise ValueError("bounds must be ((xmin, ymin, zmin), (xmax, ymax, zmax)) with max > min")
            voxel = float((hi - lo).max()) / (int(max_dim) - 1) if voxel_size is None else float(voxel_size)
        if not (voxel > 0 and np.isfinite(voxel)):
            raise ValueError(f"voxel size {voxel} must be positive (a cloud of one point needs voxel_size or bounds)")
        dims = tuple(max(2, int(np.ceil((hi[a] - lo[a]) / voxel - 1e-6)) + 1) for a in range(3))
        return lo, voxel, dims, tv * voxel

    def _reconstruct_maps(self, images: List[dict], poses: Dict[int, CameraPose], sparse_points: np.ndarray = None,
                          gfilter=None):
        """reconstruct(): preparation, sweep, fusion and its progress lines; with gfilter (_filter_arguments) the geometric
        filter between the sweep and the fusion, and its (depth, count) maps in place of the sweep's from there on.  Returns (points, colors, maps) where maps
        is None (fewer than 3 cameras, no views) or (kind, per-view maps, prepared images): kind "resident" with the
        device tensors of _sweep_resident / _sweep_extended, or "host" with the DepthNormalMap dict of _sweep."""
        print("\n" + "=" * 60)
        print("PATCHMATCH MULTI-VIEW STEREO")
        print(f"  Scale: {self.scale}x, Patch: {self.patch_size}, Iters: {self.num_iterations}")
        print("=" * 60)
        t0 = time.time()
        cam_indices = sorted(poses.keys())
        n_cams = len(cam_indices)
        if n_cams < 3:                                   # reference :88-90
            print("Need at least 3 cameras")
            return np.array([]), np.array([]), None

        self._estimate_depth_range(poses, sparse_points)
        print(f"  Depth range: [{self.depth_min:.2f}, {self.depth_max:.2f}]")
        print("\nPreparing images...")
        if self.device_prep:
            proc_images = self._prepare_images_device(images, cam_indices, poses)
        else:
            proc_images = self._prepare_images(images, cam_indices)

        print(f"\nComputing depth maps for {n_cams} views...")
        jobs = []
        for ref_idx in cam_indices:
            src = self._select_source_views(ref_idx, cam_indices, poses, k=self.NUM_SOURCES)
            if len(src) < 2:                             # reference :110-112
                print(f"  [{cam_indices.index(ref_idx)+1}/{n_cams}] Cam {ref_idx}: skipped (not enough neighbors)")
                continue
            jobs.append((ref_idx, src))

        if self.extended and jobs:
            torch = _parallel._torch_cuda()
            if torch is None:
                raise RuntimeError("the extended mode keeps its state in device tensors: PyTorch-ROCm with a GPU is required")
            sweep = self._sweep_extended
        else:
            torch = _parallel._torch_cuda() if self.device_fusion and jobs else None
            sweep = self._sweep_resident
        self._cloud_resident = False     # the engine holds the final cloud (what _cloud_normals works on)
        self._filter_threshold = None
        if torch is not None:
            resident = sweep(torch, jobs, proc_images, poses, cam_indices)
            if gfilter is not None:
                resident = self._geometric_filter_resident(torch, resident, poses, gfilter)
            print("\nFusing depth maps...")
            points, colors, raw = self._fuse_filter_resident(resident, proc_images, poses)
            self._cloud_resident = len(resident.ref_ids) > 0
            maps = ("resident", resident, proc_images)
        else:
            depth_maps = self._sweep(jobs, proc_images, poses, cam_indices)
            if gfilter is not None:
                depth_maps = self._geometric_filter_host(depth_maps, poses, gfilter)
            print("\nFusing depth maps...")
            if self.device_fusion and self._engine is not None and depth_maps:
                points, colors, raw = self._fuse_filter_device(depth_maps, proc_images, poses)
                self._cloud_resident = raw > 0
            else:
                points, colors = self._fuse_depth_maps(depth_maps, proc_images, poses)
                raw = len(points)
                if raw > 0:
                    points, colors = self._filter_points(points, colors)
            maps = ("host", depth_maps, proc_images)
        print(f"  Raw points: {raw:,}")
        if raw > 0:
            print(f"  After filtering: {len(points):,}")
        print(f"\nPatchMatch MVS completed in {time.time() - t0:.1f}s")
        return points, colors, maps

    # ------------------------------------------------------------- host geometry --
    def _estimate_depth_range(self, poses: Dict[int, CameraPose], sparse_points: np.ndarray = None):
        """1st / 99th*1.5 percentile of positive sparse-point depths over all cameras, else a
        camera-spread fallback (reference :141-165)."""
        centers = np.array([poses[i].center for i in poses])
        if sparse_points is not None and len(sparse_points) > 0:
            pooled = []
            for idx in poses:
                z = poses[idx].transform_points(sparse_points)[:, 2]
                z = z[z > 0]
                if z.size:
                    pooled.extend(z)
            if pooled:
                self.depth_min = max(0.1, np.percentile(pooled, 1))
                self.depth_max = np.percentile(pooled, 99) * 1.5
                return
        spread = np.linalg.norm(centers - np.median(centers, axis=0), axis=1)
        scene_scale = np.percentile(spread, 90)
        self.depth_min = max(0.1, scene_scale * 0.05)
        self.depth_max = scene_scale * 10.0

    def _select_source_views(self, ref_idx: int, all_indices: List[int],
                             poses: Dict[int, CameraPose], k: int = 4) -> List[int]:
        """Score = baseline * (1 - |angle-20|/60) for 5 < angle < 60 degrees, else 0; the k best
        in stable descending order (reference :193-223)."""
        c_ref = poses[ref_idx].center
        z_ref = poses[ref_idx].R[2, :]
        scored = []
        for idx in all_indices:
            if idx == ref_idx:
                continue
            baseline = np.linalg.norm(poses[idx].center - c_ref)
            cosang = np.clip(np.dot(z_ref, poses[idx].R[2, :]), -1, 1)
            angle = np.degrees(np.arccos(cosang))
            score = baseline * (1 - abs(angle - 20) / 60) if 5 < angle < 60 else 0
            scored.append((idx, score))
        scored.sort(key=lambda item: item[1], reverse=True)
        return [idx for idx, _ in scored[:k]]

    # ----------------------------------------------------------------- device -----
    def _pm_params(self):
        return _engine.make_pm_params(self.patch_size, self.num_iterations, self.num_samples,
                                      self.depth_min, self.depth_max, mode=self.mode)

    def _run_batch(self, eng, batch):
        """batch: list of (ref_idx, src_indices) with equal source counts -> maps per ref."""
        refs, srcs = self._job_slots(batch, range(len(batch)))
        depth, normal, conf = eng.patchmatch(refs, srcs, self._pm_params(), self.seed_for_stream())
        self.last_timing = eng.timing()
        return depth, normal, conf

    def seed_for_stream(self):
        return int(self.seed)

    def _patchmatch_cuda(self, ref_idx: int, src_indices: List[int], images: Dict,
                         poses: Dict[int, CameraPose]) -> DepthNormalMap:
        """One reference view (reference :225-321).  RNG stream = (seed, engine slot of ref)."""
        eng = self._ensure_engine(images, poses, sorted(images.keys()))
        depth, normal, conf = self._run_batch(eng, [(ref_idx, list(src_indices))])
        return DepthNormalMap(depth=depth[0], normal=normal[0], confidence=conf[0])

    def _sweep(self, jobs, proc_images, poses, cam_indices) -> Dict[int, DepthNormalMap]:
        """All reference views: sharded over ranks when torch.distributed is initialised,
        batched per GPU, one progress line per view (reference :104-123)."""
        rank, world = _parallel.rank_world(self.process_group)
        mine = _parallel.shard(len(jobs), rank, world)
        eng = self._ensure_engine(proc_images, poses, cam_indices)
        local = {}
        by_count = {}
        for j in mine:
            by_count.setdefault(len(jobs[j][1]), []).append(j)
        for _, idxs in sorted(by_count.items()):
            for b in range(0, len(idxs), self.views_per_batch):
                chunk = idxs[b:b + self.views_per_batch]
                t1 = time.time()
                depth, normal, conf = self._run_batch(eng, [jobs[j] for j in chunk])
                per_view = (time.time() - t1) / len(chunk)
                for n, j in enumerate(chunk):
                    local[j] = DepthNormalMap(depth=depth[n], normal=normal[n], confidence=conf[n])
                    _print_view_progress(cam_indices, jobs[j][0], np.sum(conf[n] >= self.min_views), per_view)
        if world > 1:
            local = _parallel.allgather_maps(local, len(jobs), proc_images[cam_indices[0]]["shape"],
                                             self.process_group, DepthNormalMap, device_id=self.device_id)
        return {jobs[j][0]: local[j] for j in sorted(local)}

    def _plan_group_launches(self, jobs, mine, per, base, views_per_batch):
        """The launch / exchange plan of one rank in the several-rank _sweep_resident: its block of `per`
        rows (row = job - base) is cut into row groups that are THE SAME ON EVERY RANK, its jobs into
        launches (consecutive jobs, one source count, at most a group long, never straddling a group
        boundary).  Returns (groups, plan): groups = [(first row, end row)], plan = [(jobs of a launch or
        None, [indices of the groups to all-gather right after it])] -- every group exactly once, in
        order, on every rank (also on a rank without views: the collectives must match)."""
        n_groups = 2 if per >= 2 else 1
        group_rows = (per + n_groups - 1) // n_groups
        groups = [(g * group_rows, min((g + 1) * group_rows, per)) for g in range(n_groups)]
        plan, next_group = [], 0
        for chunk in _parallel.runs_of_one_count(jobs, mine, min(views_per_batch, group_rows)):
            lo = 0
            while lo < len(chunk):
                row = chunk[lo] - base
                room = groups[min(row // group_rows, n_groups - 1)][1] - row
                piece = chunk[lo:lo + room]
                lo += room
                done_rows = piece[-1] - base + 1
                ready = []
                while next_group < n_groups and (done_rows >= groups[next_group][1] or done_rows == len(mine)):
                    ready.append(next_group)
                    next_group += 1
                plan.append((piece, ready))
        if next_group < n_groups:
            plan.append((None, list(range(next_group, n_groups))))
        return groups, plan

    def _sweep_resident(self, torch, jobs, proc_images, poses, cam_indices) -> "_ResidentMaps":
        """_sweep with the maps kept in device tensors: this rank's views are swept straight into
        its block of rows (amvs_patchmatch_device) and the valid-pixel counts of the progress lines are
        reduced on the GPU.

        Several ranks: every rank's block is `per` = ceil(n / world) rows of ONE tensor in job order, cut
        into the same row groups on every rank (at least two, so that a 4-view shard still overlaps);
        the launches are capped at a group, and as soon as the launches covering a group are enqueued its
        all-gather (RCCL: three collectives -- depth, confidence, normals -- on a second stream, ordered
        after the sweep by an event) runs under the sweep of the next group.  Only the last group's
        exchange is exposed.  The host never waits for a collective before the last launch is enqueued (a
        call only waits for the sweep stream while it stages its job table); the progress lines are
        printed afterwards.  The reference loops serially and has no
        exchange (:104-123)."""
        rank, world = _parallel.rank_world(self.process_group)
        mine = _parallel.shard(len(jobs), rank, world)
        eng = self._ensure_engine(proc_images, poses, cam_indices)
        H, W = proc_images[cam_indices[0]]["shape"]
        hw = H * W
        dev = torch.device("cuda", self.device_id)
        n = len(jobs)
        if world == 1 and not (self.exercise_exchange and torch.distributed.is_initialized()):
            depth = torch.empty((n, hw), dtype=torch.float32, device=dev)
            normal = torch.empty((n, 3 * hw), dtype=torch.float32, device=dev)
            conf = torch.empty((n, hw), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            for chunk in _parallel.runs_of_one_count(jobs, mine, self.views_per_batch):
                t1 = time.time()
                r0 = chunk[0]
                refs, srcs = self._job_slots(jobs, chunk)
                eng.patchmatch_device(refs, srcs, self._pm_params(), self.seed_for_stream(),
                                      depth[r0].data_ptr(), normal[r0].data_ptr(), conf[r0].data_ptr())
                eng.sync()
                self.last_timing = eng.timing()
                per_view = (time.time() - t1) / len(chunk)
                valid = (conf[r0:r0 + len(chunk)] >= self.min_views).sum(dim=1).tolist()
                for k, j in enumerate(chunk):
                    _print_view_progress(cam_indices, jobs[j][0], valid[k], per_view)
            return _ResidentMaps(ref_ids=[jobs[j][0] for j in range(n)], depth=depth, normal=normal,
                                 confidence=conf, shape=(H, W))

        dist = torch.distributed
        direct = dist.get_backend(self.process_group) == "nccl"
        per = (n + world - 1) // world                    # rows per rank block (the last block may be short)
        base = rank * per
        groups, plan = self._plan_group_launches(jobs, mine, per, base, self.views_per_batch)
        # Storage rows are laid out [group][rank][row of the group]: what one group's exchange fills is ONE
        # contiguous block, so a group is one all_gather_into_tensor per map, in place (this rank's rows are
        # its own slice of the block) -- no list of output views for ProcessGroupNCCL to assemble through a
        # flattened scratch and copy out.  Job j = r * per + a + i (rank r, group [a, b), i < b - a) lives in
        # storage row world * a + r * (b - a) + i; rows of jobs >= n are padding.
        def store_row(j):
            return self._storage_row(j, per, world, groups)
        depth = torch.zeros((world * per, hw), dtype=torch.float32, device=dev)
        normal = torch.zeros((world * per, 3 * hw), dtype=torch.float32, device=dev)
        conf = torch.zeros((world * per, hw), dtype=torch.float32, device=dev)
        maps = [depth, conf] + ([normal] if self.gather_normals else [])      # fusion reads the first two
        sweep_stream, comm_stream = self._exchange_streams(torch, dev)
        torch.cuda.synchronize(dev)                       # the zero fills ran on torch's current stream
        eng.set_stream(sweep_stream.cuda_stream)
        works = []

        def gather_group(a, b, swept):
            """All-gather rows [a, b) of every rank's block; `swept` = event after the launches that wrote them."""
            blk0, rows = world * a, b - a
            with torch.cuda.stream(comm_stream):
                comm_stream.wait_event(swept)
                for t in maps:
                    block = t[blk0: blk0 + world * rows]              # [rank][row], contiguous
                    own = block[rank * rows: (rank + 1) * rows]
                    if direct:
                        works.append(dist.all_gather_into_tensor(block, own, group=self.process_group, async_op=True))
                    else:                                 # gloo (tests): staged through the host
                        swept.synchronize()
                        host = torch.empty((world * rows, t.shape[1]), dtype=torch.float32)
                        dist.all_gather_into_tensor(host, own.cpu(), group=self.process_group)
                        for r in range(world):
                            if r != rank:
                                block[r * rows: (r + 1) * rows].copy_(host[r * rows: (r + 1) * rows])

        t1 = time.time()
        try:
            for piece, ready in plan:
                if piece is not None:
                    r0 = store_row(piece[0])              # (a launch never straddles a group: consecutive storage rows)
                    refs, srcs = self._job_slots(jobs, piece)
                    eng.patchmatch_device(refs, srcs, self._pm_params(), self.seed_for_stream(),
                                          depth[r0].data_ptr(), normal[r0].data_ptr(), conf[r0].data_ptr())
                for g in ready:                           # (a rank without views still takes part in every collective)
                    swept = torch.cuda.Event()
                    swept.record(sweep_stream)
                    gather_group(*groups[g], swept)
            for w in works:
                w.wait()                                  # torch's current stream waits for the collective
            eng.sync()
            self.last_timing = eng.timing()
            comm_stream.synchronize()
            torch.cuda.synchronize(dev)
        finally:
            eng.set_stream(None)
        per_view = (time.time() - t1) / max(len(mine), 1)
        # back to job order (the fusion walks the maps view by view: the cloud's point order depends on it)
        order = torch.tensor([store_row(j) for j in range(n)], dtype=torch.long, device=dev)
        identity = all(store_row(j) == j for j in range(n))
        depth, conf = (depth[:n], conf[:n]) if identity else (depth.index_select(0, order), conf.index_select(0, order))
        normal = normal[:n] if identity else normal.index_select(0, order)
        valid = (conf >= self.min_views).sum(dim=1).tolist()
        for j in mine:
            _print_view_progress(cam_indices, jobs[j][0], valid[j], per_view)
        return _ResidentMaps(ref_ids=[jobs[j][0] for j in range(n)], depth=depth, normal=normal,
                             confidence=conf, shape=(H, W))

    @staticmethod
    def _storage_row(j, per, world, groups):
        """Storage row of job j in the several-rank _sweep_resident: rows are laid out [group][rank][row of the
        group], so that the rows one group's exchange fills are ONE contiguous block (one all_gather_into_tensor
        per map).  Job j = r * per + k belongs to rank r; k lies in group [a, b)."""
        r, k = divmod(j, per)
        a, b = next(g for g in groups if g[0] <= k < g[1])
        return world * a + r * (b - a) + (k - a)

    def _exchange_streams(self, torch, dev):
        """The sweep / exchange streams of the several-rank path, created once per device and reused by every
        later reconstruct of this object."""
        cached = self._streams
        if cached is None or cached[0] != dev:
            cached = (dev, torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
            self._streams = cached
        return cached[1], cached[2]

    def _sweep_extended(self, torch, jobs, proc_images, poses, cam_indices) -> "_ResidentMaps":
        """The extended mode (csrc/amvs_extended.hip): the state of ALL views lives in device tensors;
        this rank iterates its shard of the reference views, and after every iteration the ranks
        all-gather the depth / normal / cost maps -- the exchange `north_star` places between the
        propagation sweeps, feeding the next iteration's view propagation and the final geometric
        consistency.  Confidence = number of geometrically consistent source views."""
        rank, world = _parallel.rank_world(self.process_group)
        mine = _parallel.shard(len(jobs), rank, world)
        eng = self._ensure_engine(proc_images, poses, cam_indices)
        H, W = proc_images[cam_indices[0]]["shape"]
        hw = H * W
        dev = torch.device("cuda", self.device_id)
        n_views = len(cam_indices)
        depth = torch.zeros((n_views, hw), dtype=torch.float32, device=dev)
        normal = torch.zeros((n_views, 3 * hw), dtype=torch.float32, device=dev)
        cost = torch.full((n_views, hw), float("inf"), dtype=torch.float32, device=dev)
        params = _engine.make_xpm_params(self.patch_size, self.depth_min, self.depth_max,
                                         window_stride=2 if self.patch_size >= 7 else 1, num_refine=2)
        groups = {}
        for j in mine:                                     # one call has one source count
            groups.setdefault(len(jobs[j][1]), []).append(j)
        calls = [(*self._job_slots(jobs, js), js) for _, js in sorted(groups.items())]
        slots_all = torch.tensor([self._slot[jobs[j][0]] for j in range(len(jobs))], dtype=torch.long, device=dev)
        slots_mine = torch.tensor([self._slot[jobs[j][0]] for j in mine], dtype=torch.long, device=dev)
        direct = world > 1 and torch.distributed.get_backend(self.process_group) == "nccl"

        def exchange():
            if world == 1:
                return
            for t, width in ((depth, hw), (normal, 3 * hw), (cost, hw)):
                local = t[slots_mine]
                full = _parallel.allgather_packed(local if direct else local.cpu(), len(jobs), width, self.process_group)
                t[slots_all] = full if direct else full.to(dev)
            # the scatter above runs on torch's stream; the engine launches on its own (non-blocking)
            # stream, which nothing else orders after it
            torch.cuda.synchronize(dev)

        ptrs = (depth.data_ptr(), normal.data_ptr(), cost.data_ptr())
        torch.cuda.synchronize(dev)
        t1 = time.time()
        for refs, srcs, _ in calls:
            eng.xpm_init(refs, srcs, params, self.seed_for_stream(), *ptrs)
        eng.sync()
        exchange()
        for it in range(self.num_iterations):
            # several calls per iteration (jobs with different source counts): their view candidates
            # read a copy of the maps taken before the first call writes, so that the result does not
            # depend on the grouping (nor on the rank layout)
            snap = (depth.clone(), normal.clone()) if len(calls) > 1 else None
            if snap is not None:
                torch.cuda.synchronize(dev)
            for refs, srcs, _ in calls:
                eng.xpm_iterate(refs, srcs, params, it, self.seed_for_stream(), *ptrs,
                                snapshot_depth_ptr=snap[0].data_ptr() if snap else 0,
                                snapshot_normal_ptr=snap[1].data_ptr() if snap else 0)
            eng.sync()
            exchange()
        conf = torch.zeros((len(jobs), hw), dtype=torch.float32, device=dev)
        row = {j: n for n, j in enumerate(mine)}
        conf_mine = torch.zeros((len(mine), hw), dtype=torch.float32, device=dev)
        for refs, srcs, js in calls:
            block = torch.empty((len(js), hw), dtype=torch.float32, device=dev)
            eng.xpm_consistency(refs, srcs, params, *ptrs, block.data_ptr())
            eng.sync()
            for n, j in enumerate(js):
                conf_mine[row[j]] = block[n]
        if world > 1:
            full = _parallel.allgather_packed(conf_mine if direct else conf_mine.cpu(), len(jobs), hw, self.process_group)
            conf = full if direct else full.to(dev)
        else:
            conf = conf_mine
        per_view = (time.time() - t1) / max(len(mine), 1)
        valid = (conf >= self.min_views).sum(dim=1).tolist()
        for j in range(len(jobs)):
            _print_view_progress(cam_indices, jobs[j][0], valid[j], per_view)
        return _ResidentMaps(ref_ids=[jobs[j][0] for j in range(len(jobs))], depth=depth[slots_all].contiguous(),
                             normal=normal[slots_all].contiguous(), confidence=conf.contiguous(), shape=(H, W))

    # ------------------------------------------------------------ geometric filter --
    def _filter_rows(self, ids, poses, gfilter):
        return nearest_map_neighbours([poses[i].center for i in ids], gfilter[4])

    def _geometric_filter_resident(self, torch, maps: "_ResidentMaps", poses, gfilter) -> "_ResidentMaps":
        """The maps of _sweep_resident / _sweep_extended through Engine.depth_filter, device to device: new tensors take
        the filtered depths and the counts (the normal maps are the sweep's)."""
        ids = list(maps.ref_ids)
        if not ids:
            return maps
        t0 = time.time()
        px, rel, min_views, refine, _ = gfilter
        depth, count = torch.empty_like(maps.depth), torch.empty_like(maps.confidence)
        torch.cuda.synchronize(maps.depth.device)
        n_valid, n_kept = self._engine.depth_filter(self.K_scaled, [(poses[i].R, poses[i].t) for i in ids], self.min_views, px, rel,
                                                    min_views, refine, neighbours=self._filter_rows(ids, poses, gfilter),
                                                    device_ptrs=(maps.depth.data_ptr(), maps.confidence.data_ptr()),
                                                    out_ptrs=(depth.data_ptr(), count.data_ptr()))
        self._filter_threshold = min_views
        print(f"\nGeometric filter: {n_kept:,} of {n_valid:,} valid pixels agree with {min_views} views or more ({time.time() - t0:.2f}s)")
        return _ResidentMaps(ref_ids=ids, depth=depth, normal=maps.normal, confidence=count, shape=maps.shape)

    def _geometric_filter_host(self, depth_maps: Dict[int, DepthNormalMap], poses, gfilter) -> Dict[int, DepthNormalMap]:
        """The host maps of _sweep through Engine.depth_filter."""
        ids = list(depth_maps)
        if not ids:
            return depth_maps
        t0 = time.time()
        px, rel, min_views, refine, _ = gfilter
        depth, count, (n_valid, n_kept) = self._engine.depth_filter(
            self.K_scaled, [(poses[i].R, poses[i].t) for i in ids], self.min_views, px, rel, min_views, refine,
            neighbours=self._filter_rows(ids, poses, gfilter), depth=np.stack([depth_maps[i].depth for i in ids]),
            conf=np.stack([depth_maps[i].confidence for i in ids]))
        self._filter_threshold = min_views
        print(f"\nGeometric filter: {n_kept:,} of {n_valid:,} valid pixels agree with {min_views} views or more ({time.time() - t0:.2f}s)")
        return {i: DepthNormalMap(depth=depth[n], normal=depth_maps[i].normal, confidence=count[n]) for n, i in enumerate(ids)}

    # ------------------------------------------------------------ fusion / filter --
    def _fuse_filter_resident(self, maps: "_ResidentMaps", images: Dict, poses: Dict[int, CameraPose]):
        """Fusion + filter straight from the device tensors of _sweep_resident."""
        import torch
        n = len(maps.ref_ids)
        if n == 0:
            return np.array([]).reshape(0, 3), np.array([]).reshape(0, 3), 0
        K_inv = np.linalg.inv(self.K_scaled)
        torch.cuda.synchronize(maps.depth.device)
        if self._resident_colors and images is self._engine_images:
            return self._engine.fuse_filter_views([self._slot[i] for i in maps.ref_ids], maps.depth.data_ptr(),
                                                  maps.confidence.data_ptr(), K_inv,
                                                  [(poses[i].R, poses[i].t) for i in maps.ref_ids], self._threshold(),
                                                  do_filter=True)
        cols = np.stack([images[i]["color"] for i in maps.ref_ids])
        return self._engine.fuse_filter(None, None, cols, K_inv, [(poses[i].R, poses[i].t) for i in maps.ref_ids],
                                        self._threshold(), do_filter=True,
                                        device_ptrs=(maps.depth.data_ptr(), maps.confidence.data_ptr(), n))

    def _fuse_filter_device(self, depth_maps: Dict[int, "DepthNormalMap"], images: Dict,
                            poses: Dict[int, CameraPose]):
        """_fuse_depth_maps + _filter_points on the GPU (amvs_fuse_filter): float64, same order,
        bit-identical clouds; returns (points, colors, raw point count)."""
        ids = [idx for idx, dm in depth_maps.items() if np.any(dm.confidence >= self._threshold())]
        if not ids:
            return np.array([]).reshape(0, 3), np.array([]).reshape(0, 3), 0
        depth = np.stack([depth_maps[i].depth for i in ids])
        conf = np.stack([depth_maps[i].confidence for i in ids])
        cols = np.stack([images[i]["color"] for i in ids])
        K_inv = np.linalg.inv(self.K_scaled)
        return self._engine.fuse_filter(depth, conf, cols, K_inv, [(poses[i].R, poses[i].t) for i in ids],
                                        self._threshold(), do_filter=True)


    def _fuse_depth_maps(self, depth_maps: Dict[int, DepthNormalMap], images: Dict,
                         poses: Dict[int, CameraPose]) -> Tuple[np.ndarray, np.ndarray]:
        """Back-project pixels with confidence >= min_views to world space (reference :536-570)."""
        K_inv = np.linalg.inv(self.K_scaled)
        clouds, cloud_colors = [], []
        for idx, dm in depth_maps.items():
            keep = dm.confidence >= self._threshold()
            if not np.any(keep):
                continue
            ys, xs = np.where(keep)
            pix = np.stack([xs, ys, np.ones_like(xs)], axis=-1)
            cam_pts = rows_matmul(pix, K_inv.T) * dm.depth[keep][:, np.newaxis]
            clouds.append(rows_matmul(cam_pts - poses[idx].t, poses[idx].R))
            cloud_colors.append(images[idx]["color"][ys, xs][:, ::-1])      # BGR -> RGB
        if not clouds:
            return np.array([]).reshape(0, 3), np.array([]).reshape(0, 3)
        return np.vstack(clouds), np.vstack(cloud_colors)

    def _filter_points(self, points: np.ndarray, colors: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """95th-percentile radius cut around the median, then 1 cm voxel de-duplication keeping
        the first point of every voxel in key order (reference :572-588)."""
        dist = np.linalg.norm(points - np.median(points, axis=0), axis=1)
        keep = dist < np.percentile(dist, 95)
        points, colors = points[keep], colors[keep]
        cell = np.floor(points / 0.01).astype(np.int64)
        keys = cell[:, 0] * 1000000000 + cell[:, 1] * 1000000 + cell[:, 2]
        _, first = np.unique(keys, return_index=True)
        return points[first], colors[first]

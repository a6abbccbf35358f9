"""The dense-SIFT mode without a GPU: the fourth header against its binding table, the refusal of a NULL context, the
restatement of tests/match_restatement.py against independent yardsticks (a loop, an SVD), the input family of
tests/match_inputs.py against the edges the GPU comparison relies on, and the host logic of core/dense.py (the pair list,
the descriptor checks, the missing-cv2 error).  tests/test_hip_match.py and tests/test_hip_pair_cloud.py compare the device
with the same restatement."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_inputs as mi  # noqa: E402
import match_restatement as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_METHODS = ("set_descriptors", "knn2", "match_descriptors", "pair_cloud_begin", "pair_triangulate", "pair_cloud_finish",
                  "cloud_bounds", "cloud_voxel_downsample_grid")


# ----------------------------------------------------------------------------------------- header and table ---
def test_fourth_header_matches_its_table_and_every_symbol_is_exported():
    from amvs import _lib
    header = open(os.path.join(ROOT, "include", "amvs_match.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(amvs_\w+)\(", header, re.M))
    assert declared == set(_lib.MATCH_SIGNATURES) and len(declared) == 9
    for table in (_lib.SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.LENS_SIGNATURES):
        assert not declared & set(table)
    for other in ("amvs.h", "amvs_depth.h", "amvs_lens.h"):
        assert not declared & set(re.findall(r"^(?:int|const char \*)\s*(amvs_\w+)\(",
                                             open(os.path.join(ROOT, "include", other)).read(), re.M))
    assert '#include "amvs.h"' in header
    lib = _lib.load()
    for name, (res, args) in _lib.MATCH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    from amvs.engine import Engine
    for m in ENGINE_METHODS:
        assert callable(getattr(Engine, m)), m
    for name, value in (("AMVS_DESC_TILE", mi.TILE), ("AMVS_DESC_CHUNK", mi.CHUNK), ("AMVS_DESC_QUERY_BLOCK", mi.QBLOCK),
                        ("AMVS_JACOBI_SWEEPS", mr.JACOBI_SWEEPS), ("AMVS_DESC_DIM", 128)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, header).group(1)) == value
    assert int(re.search(r"#define AMVS_DESC_MAX_ROWS\s+(\d+)", header).group(1)) >= 262144
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", makefile, re.M).group(1).split()
    assert {"amvs_match.o", "amvs_triangulate.o", "amvs_capi_match.o"} <= set(objs)
    assert "../../include/amvs_match.h" in re.search(r"^%\.o:(.*)$", makefile, re.M).group(1)


def test_a_null_context_is_refused_by_every_entry_point_without_a_device():
    from amvs import _lib
    lib = _lib.load()
    d9, d3 = (C.c_double * 9)(), (C.c_double * 3)()
    f2, u8 = (C.c_float * 2)(), (C.c_uint8 * 128)()
    i2, n64 = (C.c_int32 * 2)(), C.c_int64(0)
    calls = {
        "amvs_desc_set": (None, 0, u8, 1, 128),
        "amvs_desc_knn2": (None, 0, 1, i2, i2),
        "amvs_desc_match": (None, 0, 1, 0.85, 0, i2, i2, i2, C.byref(n64)),
        "amvs_pair_cloud_begin": (None,),
        "amvs_pair_triangulate": (None, d9, d9, d3, d9, d3, f2, f2, u8, 1, 0.1, 50.0, 0.99, 6.0, C.byref(n64)),
        "amvs_pair_cloud_finish": (None, C.byref(n64)),
        "amvs_cloud_bounds": (None, None, d3, d3),
        "amvs_cloud_voxel_downsample_grid": (None, None, d3, 0.1, C.byref(n64)),
        "amvs_match_selftest_sqrt": (None, d3, 3, d3),
    }
    assert set(calls) == set(_lib.MATCH_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
    assert lib.amvs_desc_set(None, -5, None, -1, 7) == -1          # whatever the other arguments


# ------------------------------------------------------------------------------------------ the restatement ---
def knn2_loop(q, t):
    """The definition, one pair at a time, in Python integers."""
    out_i, out_s = [], []
    for a in q.astype(np.int64):
        s = [(int(((a - b) ** 2).sum()), j) for j, b in enumerate(t.astype(np.int64))]
        s.sort()
        out_i.append([s[0][1], s[1][1]])
        out_s.append([s[0][0], s[1][0]])
    return np.array(out_i, np.int32), np.array(out_s, np.int32)


@pytest.mark.parametrize("shape", [(1, 2), (31, 33), (33, 31), (64, 257)])
def test_knn2_restatement_is_the_definition(shape):
    q, t = mi.knn_shape_case(*shape)
    idx, d2 = mr.knn2(q, t)
    li, ls = knn2_loop(q, t)
    assert np.array_equal(idx, li) and np.array_equal(d2, ls)


def test_knn2_restatement_on_the_planted_cases():
    q, t = mi.far_case()
    idx, d2 = mr.knn2(q, t)
    assert idx.tolist() == [[0, 1]] and d2.tolist() == [[8323200, 8323200]]
    q, t = mi.identical_case()
    idx, d2 = mr.knn2(q, t)
    assert idx[:, 0].tolist() == [3, 40, 69, 0] and not d2[:, 0].any() and d2[:, 1].all()
    q, t, rows = mi.duplicate_case()
    idx, d2 = mr.knn2(q, t)
    assert idx.tolist() == [rows[:2]] * 3 and (d2[:, 0] == d2[:, 1]).all() and d2[0, 0] == 0
    # rows of different tiles (32), chunks (256) and splits
    assert len({r // mi.TILE for r in rows}) >= 4 and len({r // mi.CHUNK for r in rows}) == 3
    q, t, planted = mi.split_case()
    idx, _ = mr.knn2(q, t)
    assert np.array_equal(idx, planted) and (planted[:, 0] // mi.CHUNK != planted[:, 1] // mi.CHUNK).all()
    assert mi.splits(len(q), len(t)) >= 3


def test_restatement_by_minima_is_the_sorted_one():
    for case in (mi.knn_shape_case(300, 1000), mi.duplicate_case()[:2], mi.far_case(), mi.identical_case(), mi.split_case()[:2]):
        a, b = mr.knn2(*case), mr.knn2_by_minima(*case)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


_MULTI = {}


def multi_chunk_restated():
    if not _MULTI:
        q, t, planted = mi.multi_chunk_case()
        _MULTI["v"] = (q, t, planted) + mr.knn2_by_minima(q, t)
    return _MULTI["v"]


def test_multi_chunk_case_walks_the_chunk_loop_and_plants_across_its_boundaries():
    n_q, n_t = mi.MULTI_CHUNK_SHAPE
    cps, chunks = mi.chunks_per_split(n_q, n_t), -(-n_t // mi.CHUNK)
    assert cps == 2 and chunks % cps == 1 and n_t % mi.TILE != 0        # more than one chunk a workgroup; an uneven last share
    # no other shape of the family does: this case is the one that runs the chunk loop more than once
    assert all(mi.chunks_per_split(*s) == 1 for s in mi.KNN_SHAPES + [(40, 1000), (4096, 5003), (300, 400)])
    q, t, planted, idx, d2 = multi_chunk_restated()
    assert np.array_equal(idx[:600], planted)
    share, chunk = planted // (cps * mi.CHUNK), planted // mi.CHUNK
    kind = np.arange(600) % 6
    for k in (0, 1):            # best and second best in different chunks of one share, both orders
        assert (share[kind == k, 0] == share[kind == k, 1]).all() and (chunk[kind == k, 0] != chunk[kind == k, 1]).all()
    assert (planted[kind == 0, 0] < planted[kind == 0, 1]).all() and (planted[kind == 1, 0] > planted[kind == 1, 1]).all()
    assert (share[kind == 2, 0] != share[kind == 2, 1]).all()
    for k, same_share in ((3, True), (4, False)):      # exact copies astride a chunk boundary: inside a share, between two
        sel = kind == k
        assert (planted[sel, 1] == planted[sel, 0] + 1).all() and (planted[sel, 1] % mi.CHUNK == 0).all()
        assert ((share[sel, 0] == share[sel, 1]) == same_share).all() and not d2[:600][sel].any()
    assert (share[kind == 5] == mi.splits(n_q, n_t) - 1).all() and not d2[:600][kind == 5].any()


def test_shapes_reach_the_edges_of_the_launch_shape():
    nq = {s[0] for s in mi.KNN_SHAPES}
    nt = {s[1] for s in mi.KNN_SHAPES}
    for T in (mi.TILE, mi.QBLOCK // 4, mi.QBLOCK, mi.CHUNK):
        assert {T - 1, T, T + 1} <= nq, T
    for T in (mi.TILE, mi.CHUNK, 2 * mi.CHUNK):
        assert {T - 1, T, T + 1} <= nt, T
    assert {(1, 2), (2, 2), (31, 33), (33, 31), (64, 257), (129, 127), (300, 1000)} <= set(mi.KNN_SHAPES)


def test_match_restatement_ratio_and_cross_check():
    q, t = mi.ratio_case()
    idx, d2 = mr.knn2(q, t)
    for ratio in (0.85, 0.8):
        qi, ti, s = mr.match(q, t, ratio)
        r = np.float64(np.float32(ratio))
        expect = [i for i in range(len(q)) if float(d2[i, 0]) < (r * r) * float(d2[i, 1])]
        assert qi.tolist() == expect and np.array_equal(ti, idx[qi, 0]) and np.array_equal(s, d2[qi, 0])
        assert 90 <= len(qi) < 200                       # the clear matches pass, the ambiguous ones do not
        qx, tx, _ = mr.match(q, t, ratio, cross_check=True)
        assert set(zip(qx.tolist(), tx.tolist())) < set(zip(qi.tolist(), ti.tolist()))
        assert len(set(tx.tolist())) == len(tx)          # the cross check leaves a train row to one query
        assert np.all(np.diff(qx) > 0)


TRI = {}


def tri_case(beta):
    if beta not in TRI:
        c = mi.triangulation_case(beta)
        X, keep, margin = mr.triangulate(c["K"], c["R1"], c["t1"], c["R2"], c["t2"], c["pts1"], c["pts2"])
        TRI[beta] = (c, X, keep, margin)
    return TRI[beta]


@pytest.mark.parametrize("beta", mi.BASELINES_DEG)
def test_jacobi_route_stays_close_to_the_svd(beta):
    c, X, keep, margin = tri_case(beta)
    n = c["n_noisy"]
    Xs = mr.triangulate_svd(c["K"], c["R1"], c["t1"], c["R2"], c["t2"], c["pts1"][:n], c["pts2"][:n])
    rel = np.linalg.norm(X[:n] - Xs, axis=1) / np.linalg.norm(Xs, axis=1)
    print(f"baseline {beta} deg: Jacobi on A^T A against the SVD of A, largest relative difference in X {rel.max():.3e}")
    assert rel.max() < 1e-9


@pytest.mark.parametrize("beta", mi.BASELINES_DEG)
def test_planted_candidates_fall_on_their_side_and_no_decision_is_marginal(beta):
    c, X, keep, margin = tri_case(beta)
    for name, (row, expect) in c["planted"].items():
        assert bool(keep[row]) == expect, (name, X[row])
    # seeded continuous inputs: no decision of the restatement is within 1e-6 relative of its threshold
    assert margin.min() > 1e-6, margin.min()
    n = c["n_noisy"]
    assert 0.5 * n < keep[:n].sum() <= n
    names = set(c["planted"])
    assert {"reproj1_in", "reproj1_out", "reproj2_in", "reproj2_out", "parallax_in"} <= names
    if beta == 40.0:
        assert {"near1_in", "near1_out", "near2_in", "near2_out", "far1_in", "far1_out", "far2_in", "far2_out"} <= names
    if beta <= 2.0:
        assert "parallax_out" in names


def test_triangulation_of_exact_projections_returns_the_point():
    R2, t2 = mi.second_view(10.0)
    X = np.array([[0.3, -0.2, 5.5], [-1.0, 0.4, 4.0]])
    p1 = mi.project(mi.K_TRI, np.eye(3), np.zeros(3), X)
    p2 = mi.project(mi.K_TRI, R2, t2, X)
    Y, keep, _ = mr.triangulate(mi.K_TRI, np.eye(3), np.zeros(3), R2, t2, p1, p2)
    assert keep.all() and np.abs(Y - X).max() < 1e-3          # (float32 keypoints)


def test_grid_restatement_against_a_dictionary():
    for name, (p, c, keep, origin, voxel) in mi.grid_cases().items():
        if len(p) > 5000:
            continue
        gp, gc = mr.voxel_grid(p, c, origin, voxel, keep)
        first = {}
        for i in range(len(p)):
            if keep is not None and not keep[i]:
                continue
            first.setdefault(tuple(np.floor((p[i] - origin) / voxel).astype(np.int64)), i)
        order = [first[k] for k in sorted(first)]
        assert np.array_equal(gp, p[order]) and np.array_equal(gc, c[order]), name
    p, c, keep, origin, voxel = mi.grid_cases()["one_voxel"]
    assert len(mr.voxel_grid(p, c, origin, voxel)[0]) == 1
    p, c, keep, origin, voxel = mi.grid_cases()["on_faces"]
    assert len(mr.voxel_grid(p, c, origin, voxel)[0]) == len(np.unique(p, axis=0))


# ----------------------------------------------------------------------------------------------- host logic ---
@pytest.mark.parametrize("n", [2, 3, 9, 40])
@pytest.mark.parametrize("window", [1, 8, 20])
def test_pair_list_against_a_literal_double_loop(n, window):
    from amvs.core.dense import camera_pairs
    literal = []
    for i in range(n):
        for j in range(n):
            if j <= i:
                continue
            if abs(i - j) <= window or abs(i - j) >= n - window:
                literal.append((i, j))
    assert camera_pairs(n, window) == literal == mr.pair_list(n, window)


def test_descriptor_dtype_and_range_checks():
    from amvs.core.dense import descriptors_u8
    rng = np.random.default_rng(0)
    d = mi.random_desc(rng, 7)
    assert descriptors_u8(d) is not None and np.array_equal(descriptors_u8(d), d)
    assert np.array_equal(descriptors_u8(d.astype(np.float32)), d)
    for bad in (d.astype(np.float32) / 512.0, d.astype(np.float32) + 0.5, d.astype(np.float32) - 300.0,
                d.astype(np.float64), d.astype(np.int32), d[:, :64]):
        with pytest.raises(ValueError) as e:
            descriptors_u8(bad)
        if np.asarray(bad).shape[1] == 128:
            assert "RootSIFT" in str(e.value) and "learned" in str(e.value)


def test_reconstruct_without_cv2_points_to_reconstruct_from_features(monkeypatch):
    from amvs.core import DenseReconstructor, reconstruct_from_features
    from amvs.core.camera import Camera
    assert reconstruct_from_features is DenseReconstructor.reconstruct_from_features
    monkeypatch.setitem(sys.modules, "cv2", None)                  # import cv2 then raises ImportError
    rec = DenseReconstructor(Camera(K=np.eye(3), dist=np.zeros(5)))
    assert (rec.min_parallax, rec.max_reproj_error) == (0.3, 6.0)
    with pytest.raises(ImportError, match="reconstruct_from_features"):
        rec.reconstruct([], {})
    with pytest.raises(ValueError, match="with_normals"):
        rec.reconstruct_from_features({}, [], {}, with_normals=True)


SCENE = {}


def scene_restated():
    """The end-to-end scene through the chained restatement, once (the brute-force neighbour statistic stands in for
    the pinned device one)."""
    if not SCENE:
        cam, poses, features, images, planted = mi.dense_scene()
        rp = {i: (p.R, np.ravel(p.t)) for i, p in poses.items()}
        SCENE["out"] = mr.reconstruct(cam.K, features, images, rp, window=20)
        SCENE["planted"] = planted
    return SCENE["out"], SCENE["planted"]


def test_the_chained_restatement_recovers_the_planted_points():
    (points, colors), planted = scene_restated()
    assert len(points) > 600 and colors.shape == points.shape and colors.dtype == np.uint8
    d = np.sqrt(((points[:, None, :] - planted[None, :, :]) ** 2).sum(2)).min(1)
    good = (d < 0.01 * 5.0).mean()                                 # 1 % of the scene's depth (the arc's radius)
    print(f"{len(points)} points, {100 * good:.1f} % within 1 % of the depth of a planted point")
    assert good >= 0.95

"""Inputs of the dense-SIFT tests (CPU and GPU): descriptor sets aimed at the edges of the matcher's launch shape, the
triangulation family with candidates planted on either side of every threshold, clouds for the bounds and the grid, and
the synthetic end-to-end scene.  Everything is seeded; nothing here reads the library."""
import math

import numpy as np

TILE, CHUNK, QBLOCK = 32, 256, 512        # include/amvs_match.h: AMVS_DESC_TILE, AMVS_DESC_CHUNK, AMVS_DESC_QUERY_BLOCK


def chunks_per_split(n_q, n_t):
    """The header's split rule: how many 256-row chunks one workgroup walks."""
    q_blocks, chunks = -(-n_q // QBLOCK), -(-n_t // CHUNK)
    want = max(1, min(chunks, 2048 // q_blocks))
    return -(-chunks // want)


def splits(n_q, n_t):
    """... and how many workgroups share the train set of one query block."""
    return -(-(-(-n_t // CHUNK)) // chunks_per_split(n_q, n_t))


# ---- descriptors ---------------------------------------------------------------------------------------------------------
def random_desc(rng, n):
    return rng.integers(0, 256, (n, 128), dtype=np.uint8)


# the issue's shapes, then one less / exactly / one more than the tile (32), a wave's queries (128), the query block (512)
# and the chunk (256)
KNN_SHAPES = [(1, 2), (2, 2), (31, 33), (33, 31), (64, 257), (129, 127), (300, 1000),
              (32, 32), (127, 255), (128, 256), (31, 31), (33, 33), (32, 2), (255, 513), (257, 512), (256, 511),
              (511, 40), (512, 300), (513, 64), (97, 600)]


def knn_shape_case(n_q, n_t):
    rng = np.random.default_rng(1000 * n_q + n_t)
    return random_desc(rng, n_q), random_desc(rng, n_t)


def near(rng, row, amount):
    return np.clip(row.astype(np.int64) + rng.integers(-amount, amount + 1, row.shape), 0, 255).astype(np.uint8)


def split_case():
    """40 queries, 1000 train rows: 4 chunks, one workgroup each; query i has its best in one chunk and its second best
    in another."""
    rng = np.random.default_rng(77)
    q, t = random_desc(rng, 40), random_desc(rng, 1000)
    assert splits(len(q), len(t)) == 4
    planted = np.empty((40, 2), np.int64)
    for i in range(40):
        cb, cs = i % 4, (i + 1 + i // 4 % 3) % 4
        assert cb != cs
        planted[i] = (cb * CHUNK + i, cs * CHUNK + 100 + i)                # (no row is planted twice)
        t[planted[i, 0]] = near(rng, q[i], 1)
        t[planted[i, 1]] = near(rng, q[i], 4)
    return q, t, planted


def far_case():
    """All 255 against two rows of zeros: s = 8 323 200 twice -- the case unmasked padding (value 128) would win."""
    return np.full((1, 128), 255, np.uint8), np.zeros((2, 128), np.uint8)


def identical_case():
    rng = np.random.default_rng(5)
    t = random_desc(rng, 70)
    return t[[3, 40, 69, 0]].copy(), t


def duplicate_case():
    """One descriptor at train rows of different tiles, chunks and splits; the queries are that descriptor and a
    neighbour of it."""
    rng = np.random.default_rng(6)
    t = random_desc(rng, 1000)
    rows = [5, 37, 300, 301, 999]
    t[rows] = t[5]
    q = np.stack([t[5], near(rng, t[5], 2), t[999]])
    return q, t, rows


def full_case():
    """4096 x 5003 random rows with 500 planted near-duplicates."""
    rng = np.random.default_rng(2024)
    q, t = random_desc(rng, 4096), random_desc(rng, 5003)
    qi = rng.choice(4096, 500, replace=False)
    ti = rng.choice(5003, 500, replace=False)
    for a, b in zip(qi, ti):
        t[b] = near(rng, q[a], 3)
    return q, t


MULTI_CHUNK_SHAPE = (4096, 66100)


def multi_chunk_case():
    """4096 x 66 100: 259 chunks dealt two to a workgroup (130 shares, the last of one chunk, its last tile of 4 rows), so
    every workgroup walks the chunk loop twice.  Planted, for the first 600 queries: the best and the second best in the
    two chunks of ONE share (in either order), in two shares, and -- as exact copies of the query -- on the two sides of
    the chunk boundary inside a share, on the two sides of a boundary between shares, and in the lone last chunk.
    Returns (q, t, planted [600][2] train rows: best, second)."""
    rng = np.random.default_rng(4242)
    n_q, n_t = MULTI_CHUNK_SHAPE
    assert chunks_per_split(n_q, n_t) == 2 and splits(n_q, n_t) == 130 and -(-n_t // CHUNK) % 2 == 1
    q, t = random_desc(rng, n_q), random_desc(rng, n_t)
    planted = np.empty((600, 2), np.int64)
    for i in range(600):
        share = 3 + (i * 7) % 120                               # chunks 2 share and 2 share + 1
        lo, hi = 2 * share * CHUNK, (2 * share + 1) * CHUNK
        kind = i % 6
        if kind == 0:                                           # best in the first chunk of the share, second in its second
            rows, exact = (lo + 20 + i % 200, hi + 30 + i % 200), False
        elif kind == 1:                                         # the other way round
            rows, exact = (hi + 10 + i % 200, lo + 40 + i % 200), False
        elif kind == 2:                                         # two shares
            rows, exact = (lo + 50 + i % 200, hi + CHUNK + 5 + i % 200), False
        elif kind == 3:                                         # copies astride the chunk boundary inside the share
            rows, exact = (hi - 1, hi), True
        elif kind == 4:                                         # copies astride the boundary between two shares
            rows, exact = (hi + CHUNK - 1, hi + CHUNK), True
        else:                                                   # the lone chunk of the last share: its last two rows
            rows, exact = (n_t - 2, n_t - 1), True
        planted[i] = rows
    # (a boundary row serves every query that names it: those queries are made copies of one descriptor)
    owner = {}
    for i in range(600):
        if i % 6 >= 3:
            key = tuple(planted[i])
            if key in owner:
                q[i] = q[owner[key]]
            else:
                owner[key] = i
                t[planted[i, 0]] = q[i]
                t[planted[i, 1]] = q[i]
        else:
            assert planted[i, 0] not in owner and planted[i, 1] not in owner
            t[planted[i, 0]] = near(rng, q[i], 1)
            t[planted[i, 1]] = near(rng, q[i], 4)
    return q, t, planted


def ratio_case():
    """300 x 400: a third of the queries with a clear match, a third with two equally good ones, the rest random; some
    train rows are claimed by two queries, which the cross check has to resolve."""
    rng = np.random.default_rng(31)
    q, t = random_desc(rng, 300), random_desc(rng, 400)
    for i in range(0, 100):
        t[i] = near(rng, q[i], 3)
    for i in range(100, 200):
        t[i] = near(rng, q[i], 3)
        t[i + 100] = near(rng, q[i], 3)
    for i in range(0, 20):
        q[280 + i] = near(rng, t[i], 5)           # a second claimant of train row i
    return q, t


# ---- triangulation ---------------------------------------------------------------------------------------------------------
F_PX, CENTRE, DEPTH = 3000.0, 1500.0, 5.0
K_TRI = np.array([[F_PX, 0.0, CENTRE], [0.0, F_PX, CENTRE], [0.0, 0.0, 1.0]])
BASELINES_DEG = (0.5, 2.0, 10.0, 40.0)


def second_view(beta_deg):
    """(R, t) of a camera on the circle of radius DEPTH about the point (0, 0, DEPTH), beta away from the first camera
    (identity at the origin), looking at that point."""
    b = math.radians(beta_deg)
    C = np.array([DEPTH * math.sin(b), 0.0, DEPTH - DEPTH * math.cos(b)])
    fwd = np.array([0.0, 0.0, DEPTH]) - C
    fwd /= np.linalg.norm(fwd)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return R, -R @ C


def project(K, R, t, X):
    pc = X @ R.T + t
    h = pc @ K.T
    return h[:, :2] / h[:, 2:3]


def triangulation_case(beta_deg, n=300, noise=0.7):
    """dict(K, R1, t1, R2, t2, pts1, pts2, rgb, planted): n noisy candidates at depth about 5, then noise-free candidates
    well on either side of each threshold; planted[name] = (row, expected decision)."""
    rng = np.random.default_rng(int(beta_deg * 10) + 9)
    R1, t1 = np.eye(3), np.zeros(3)
    R2, t2 = second_view(beta_deg)
    C2 = -R2.T @ t2
    fwd2 = R2[2]
    X = np.array([0.0, 0.0, DEPTH]) + rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.5, 1.5, 1.0])
    p1 = project(K_TRI, R1, t1, X) + rng.normal(0.0, noise, (n, 2))
    p2 = project(K_TRI, R2, t2, X) + rng.normal(0.0, noise, (n, 2))
    extra, e1, e2, planted = [], [], [], {}

    def plant(name, Xp, expect, d1=(0.0, 0.0), d2=(0.0, 0.0)):
        Xp = np.asarray(Xp, np.float64).reshape(1, 3)
        planted[name] = (n + len(extra), expect)
        extra.append(Xp[0])
        e1.append(project(K_TRI, R1, t1, Xp)[0] + np.asarray(d1))
        e2.append(project(K_TRI, R2, t2, Xp)[0] + np.asarray(d2))

    base = float(np.linalg.norm(C2))
    if beta_deg >= 10.0:
        # depth limits, per view: near view 1 only / view 2 only, and beyond 50 in view 1 only / view 2 only
        plant("near1_out", [0.01, 0.0, 0.05], False)
        plant("near1_in", [0.01, 0.0, 0.2], True)
        plant("far1_out", [0.0, 0.0, 60.0], False)
        plant("far1_in", [0.0, 0.0, 40.0], True)
    if beta_deg >= 30.0:
        plant("near2_out", C2 + 0.05 * fwd2 + 0.005 * R2[0], False)
        plant("near2_in", C2 + 0.2 * fwd2 + 0.005 * R2[0], True)
        plant("far2_out", C2 + 60.0 * fwd2, False)               # depth 60 in view 2, about 47 in view 1
        plant("far2_in", C2 + 45.0 * fwd2, True)
    # parallax: the angle is about baseline / depth; 0.3 degrees is 5.236e-3 rad
    z_floor = base / math.radians(0.3)
    if 1.45 * z_floor < 49.0:
        plant("parallax_out", [0.0, 0.0, 1.45 * z_floor], False)
        plant("parallax_in", [0.0, 0.0, 0.6 * z_floor], True)
    else:
        plant("parallax_in", [0.0, 0.0, min(0.6 * z_floor, 30.0)], True)
    # reprojection: a keypoint moved across the epipolar line by d leaves about d / 2 in each view
    plant("reproj1_in", [0.2, 0.1, DEPTH], True, d1=(0.0, 8.0))
    plant("reproj1_out", [0.2, 0.1, DEPTH], False, d1=(0.0, 20.0))
    plant("reproj2_in", [-0.2, 0.1, DEPTH], True, d2=(0.0, 8.0))
    plant("reproj2_out", [-0.2, 0.1, DEPTH], False, d2=(0.0, 20.0))
    p1 = np.vstack([p1, np.array(e1)]).astype(np.float32)
    p2 = np.vstack([p2, np.array(e2)]).astype(np.float32)
    rgb = rng.integers(0, 256, (len(p1), 3), dtype=np.uint8)
    return dict(K=K_TRI, R1=R1, t1=t1, R2=R2, t2=t2, pts1=p1, pts2=p2, rgb=rgb, planted=planted, n_noisy=n)


# ---- clouds for the bounds and the grid ------------------------------------------------------------------------------------
def grid_cases():
    """name -> (points, colors, keep or None, origin, voxel)."""
    rng = np.random.default_rng(404)
    out = {}
    out["one_point"] = (np.array([[0.25, -1.5, 3.0]]), np.array([[1, 2, 3]], np.uint8), None, np.array([0.25, -1.5, 3.0]), 0.1)
    p = rng.uniform(0.0, 0.0999, (500, 3)) + np.array([2.0, -3.0, 1.0])
    out["one_voxel"] = (p, rng.integers(0, 256, (500, 3), dtype=np.uint8), None, np.array([2.0, -3.0, 1.0]), 0.1)
    # exactly on voxel faces: multiples of a power of two from an origin that is one as well
    g = rng.integers(-6, 7, (400, 3)).astype(np.float64) * 0.25 + np.array([1.0, -2.0, 0.5])
    out["on_faces"] = (g, rng.integers(0, 256, (400, 3), dtype=np.uint8), None, np.array([1.0, -2.0, 0.5]), 0.25)
    p = rng.normal(0.0, 1.0, (3000, 3))
    keep = np.ones(3000, bool)
    for a in range(3):
        keep[np.argmin(p[:, a])] = keep[np.argmax(p[:, a])] = False
    keep[rng.choice(3000, 700, replace=False)] = False
    mn = p[keep].min(0)
    out["mask_removes_extremes"] = (p, rng.integers(0, 256, (3000, 3), dtype=np.uint8), keep, mn,
                                    float(np.linalg.norm(p[keep].max(0) - mn) / 40.0))
    p = rng.normal(0.0, 2.0, (50000, 3))
    mn = p.min(0)
    out["random_50000"] = (p, rng.integers(0, 256, (50000, 3), dtype=np.uint8), None, mn,
                           float(np.linalg.norm(p.max(0) - mn) / 1200.0))
    return out


# ---- the end-to-end scene ----------------------------------------------------------------------------------------------------
def dense_scene(n_views=6, n_points=600, n_distractors=200, H=480, W=640, seed=12):
    """(camera, poses {i: CameraPose}, features {i: {'descriptors', 'points'}}, images [{'image'}], planted (n, 3)):
    amvs.synthetic's arc of cameras around the origin, planted points projected to float32 keypoints with 0.3 px of noise,
    one random descriptor per point perturbed by +-3 per view, unmatched distractors, every view's features shuffled."""
    from amvs.core.camera import Camera
    from amvs.synthetic import arc_poses
    rng = np.random.default_rng(seed)
    f = 0.8 * W
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    poses = arc_poses(n_views, radius=5.0, arc_step_deg=10.0)
    planted = rng.uniform(-1.0, 1.0, (n_points, 3)) * np.array([1.2, 0.9, 0.6])
    desc = random_desc(rng, n_points)
    features, images = {}, []
    for i in range(n_views):
        uv = project(K, poses[i].R, np.ravel(poses[i].t), planted) + rng.normal(0.0, 0.3, (n_points, 2))
        d = near(rng, desc, 3)
        uv = np.vstack([uv, rng.uniform(0.0, 1.0, (n_distractors, 2)) * np.array([W - 1.0, H - 1.0])])
        d = np.vstack([d, random_desc(rng, n_distractors)])
        order = rng.permutation(len(uv))
        features[i] = {"descriptors": d[order], "points": uv[order].astype(np.float32)}
        images.append({"image": rng.integers(0, 256, (H, W, 3), dtype=np.uint8)})
    return Camera(K=K, dist=np.zeros(5)), poses, features, images, planted

"""Inputs of the track-state tests (include/amvs_sfm.h): planted scenes small enough to read, hand-built match tables whose
rows aim at one rule each, a seeded random generator, and SCRIPTS -- lists of (method, arguments) that a test plays on the
restatement (tests/sfm_state_restatement.py) and on the device alike and whose every result it compares.

A point exists only once amvs_sfm_triangulate has made it, so every state starts the same way: views 0 and 1 enter with
their planted poses and no observations, and the rows of pair (0, 1) become points.  With exact projections every such
row is valid, so point id == row number there; the CPU tests assert that for the restatement before anything leans on it."""
import numpy as np

K = np.array([[800.0, 0.0, 320.0], [0.0, 800.0, 240.0], [0.0, 0.0, 1.0]])
B = 256                                              # AMVS_SFM_BLOCK


def look_at(c, target=(0.0, 0.0, 6.0)):
    z = np.asarray(target, np.float64) - c
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ c


def cameras(V):
    """V poses on an arc in front of the scene, about one unit apart."""
    return [look_at(np.array([1.0 * (v - (V - 1) / 2), 0.1 * (v % 2), 0.0])) for v in range(V)]


def project(pose, X):
    R, t = pose
    pc = X @ R.T + t
    return ((pc[:, :2] / pc[:, 2:3]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)


def planted(V, N, seed, noise=0.0):
    """N points in front of V cameras, every view sees every point: keypoint k of every view is point k.  Returns
    (poses, keypoints per view, X)."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(4.5, 7.5, N)])
    poses = cameras(V)
    kps = [project(p, X) + rng.normal(0, noise, (N, 2)).astype(np.float32) if noise else project(p, X) for p in poses]
    return poses, kps, X


def identity_rows(ks):
    ks = np.asarray(list(ks), np.int32)
    return np.stack([ks, ks], 1)


def start(poses):
    """The first steps of every script: the two initial views, then the points of pair (0, 1)."""
    return [("register", (0, poses[0][0], poses[0][1])), ("register", (1, poses[1][0], poses[1][1])), ("triangulate", (1, K))]


QUERIES = [("counts", ()), ("scores", ()), ("observations", ()), ("points", ())]


# ---- hand-built: scores and correspondences, V = 4, 12 keypoints --------------------------------------------------------
def rules_case(variant="full"):
    """Views 0, 1 (and 2, unless variant == "two") are registered, view 3 is the one asked about.  Points 0 .. 11 come from
    pair (0, 1), so owner[0][k] = owner[1][k] = k; view 2 observes point 8 + k with its keypoint k for k < 4 except that its
    keypoint 3 stays un-owned (the mask).  Then point 6 dies.  The rows of view 3, in rank order:
        pair (0, 3): (5, 0)  keypoint 0 <- point 5                     (its lower rank: wins over point 7 below)
                     (3, 1)  keypoint 1 <- point 3                     (the lower rank for point 3: keeps it)
                     (6, 4)  keypoint 4 <- a keypoint whose point died: nothing
                     (2, 6)  keypoint 6 <- point 2                     (an ordinary correspondence)
        pair (1, 3): (7, 0)  keypoint 0 <- point 7                     (a second candidate, from another point: loses)
                     (3, 2)  keypoint 2 <- point 3                     (claimed by keypoint 1 already: keypoint 2 loses ...)
                     (2, 5)  keypoint 5 <- point 2                     (rank above (2, 6): keypoint 5 loses point 2)
        pair (2, 3): (1, 2)  keypoint 2 <- point 9                     (... and gets nothing, though this candidate is free)
                     (3, 3)  keypoint 3 <- registered but un-owned: nothing
                     (0, 7)  keypoint 7 <- point 8
    pair (0, 2) has no rows; pair (1, 2) is absent.  Expected for view 3 with "full": keypoints 0, 1, 6, 7 with points 5, 3, 2, 8,
    and the score 6 (keypoints 0, 1, 2, 5, 6, 7).  Variants: "two" leaves view 2 unregistered, "empty_view" gives view 3 no
    keypoint, "no_rows" is M = 0, "all_registered" registers view 3 at the end."""
    poses, kps, _ = planted(4, 12, seed=11)
    n3 = 0 if variant == "empty_view" else 12
    kps[3] = kps[3][:n3]
    pairs = [((0, 1), identity_rows(range(12))), ((0, 2), np.zeros((0, 2), np.int32))]
    if variant == "empty_view":
        pairs += [((0, 3), np.zeros((0, 2), np.int32))]
    elif variant == "no_rows":
        pairs = [((0, 1), np.zeros((0, 2), np.int32))]
    else:
        pairs += [((0, 3), np.array([[5, 0], [3, 1], [6, 4], [2, 6]], np.int32)),
                  ((1, 3), np.array([[7, 0], [3, 2], [2, 5]], np.int32)),
                  ((2, 3), np.array([[1, 2], [3, 3], [0, 7]], np.int32))]
    script = start(poses) + list(QUERIES)
    if variant != "two":
        script += [("register", (2, poses[2][0], poses[2][1], [0, 1, 2, 3], [8, 9, 10, 11], [1, 1, 1, 0]))]
    if variant not in ("no_rows",):
        script += [("kill", ([6],))]
    script += QUERIES + [("correspondences", (3,)), ("correspondences", (2,))]
    if variant == "all_registered":
        script += [("register", (3, poses[3][0], poses[3][1])), ("scores", ()), ("correspondences", (3,))]
    return kps, pairs, script


RULES_VARIANTS = ("full", "two", "empty_view", "no_rows", "all_registered")


# ---- launch edges ----------------------------------------------------------------------------------------------------------
def edges_case(N):
    """N keypoints a view, N points from pair (0, 1); views 2 and 3 are unregistered and their N rows with the registered
    views are spread over three pairs, so that the walk of amvs_sfm_scores and of amvs_sfm_correspondences(2) crosses a pair
    boundary inside a workgroup: N = B - 1, B, B + 1, 2 B + 1.  Every third point is killed first, every fifth row of (0, 2)
    names a keypoint the pair (1, 2) names too."""
    poses, kps, _ = planted(4, N, seed=N)
    a, b = N // 3, 2 * (N // 3)
    r02 = identity_rows(range(0, a))
    r12 = np.stack([np.arange(a, b), np.arange(a, b)], 1).astype(np.int32)
    r12[::5, 1] = r02[: len(r12[::5]), 1]                           # the same keypoints of view 2 as (0, 2): two candidates
    r12 = r12[np.unique(r12[:, 1], return_index=True)[1]]
    r12 = r12[np.argsort(r12[:, 0], kind="stable")]
    r03 = identity_rows(range(b, N))
    pairs = [((0, 1), identity_rows(range(N))), ((0, 2), r02), ((0, 3), r03), ((1, 2), r12)]
    script = start(poses) + [("kill", (list(range(0, N, 3)),))] + QUERIES + [("correspondences", (2,)), ("correspondences", (3,))]
    kp2 = list(range(0, N, 2))
    script += [("register", (2, poses[2][0], poses[2][1], kp2, kp2, [k % 3 != 1 for k in kp2])), ("triangulate", (2, K))] + QUERIES
    script += [("correspondences", (3,)), ("drop", ([2] * len(kp2[::4]), kp2[::4], 2))] + QUERIES
    return kps, pairs, script


# ---- triangulation -----------------------------------------------------------------------------------------------------------
def triangulate_case(variant):
    """Three registered views.  Tracks 0 .. 5 are rows of pair (0, 1); tracks 6 .. 11 are rows of (0, 2) AND of (1, 2): pair
    r = 0 makes their points and pair r = 1 must skip them; tracks 12 .. 15 are rows of (1, 2) alone.  Keypoint 16 of views 0
    and 2 is the image of a point BEHIND both cameras (row (16, 16) of (0, 2): never valid).  "same_pose": view 2 enters
    with the pose of view 1 (zero baseline with it: depth_max = 0, nothing valid there, and the DLT of identical rays).
    "boundary": B + 40 tracks in pair (0, 1), every seventh row a wrong match, valid rows on both sides of the workgroup
    boundary."""
    if variant == "boundary":
        N = B + 40
        poses, kps, _ = planted(3, N, seed=5)
        rows = identity_rows(range(N))
        rows[::7, 1] = rows[::7, 1][::-1]                                      # wrong matches: a permutation, still one-to-one
        pairs = [((0, 1), rows), ((0, 2), identity_rows(range(0, N, 2))), ((1, 2), identity_rows(range(1, N, 2)))]
        script = start(poses) + QUERIES + [("register", (2, poses[2][0], poses[2][1])), ("triangulate", (2, K))] + QUERIES
        return kps, pairs, script
    poses, kps, _ = planted(3, 16, seed=7)
    behind = np.array([[0.3, 0.2, -5.0]])
    for v in (0, 1, 2):
        kps[v] = np.concatenate([kps[v], project(poses[v], behind)])
    pairs = [((0, 1), identity_rows(range(6))), ((0, 2), identity_rows(list(range(6, 12)) + [16])),
             ((1, 2), identity_rows(range(6, 16)))]
    pose2 = poses[1] if variant == "same_pose" else poses[2]
    script = start(poses) + QUERIES + [("register", (2, pose2[0], pose2[1])), ("triangulate", (2, K))] + QUERIES
    return kps, pairs, script


TRIANGULATE_VARIANTS = ("plain", "same_pose", "boundary")


# ---- observations and drop -----------------------------------------------------------------------------------------------
def drop_case():
    """Points 0 .. 9 from pair (0, 1); view 2 observes points 0 .. 4.  Dropping (1, 7) leaves point 7 one observation: it dies and
    keypoint 7 of view 0 is free again; dropping (2, 3) leaves point 3 two.  Pair (0, 2) holds row (7, 7): the following
    triangulation of view 2 owns keypoint 7 of view 0 again, under id 10."""
    poses, kps, _ = planted(3, 10, seed=3)
    pairs = [((0, 1), identity_rows(range(10))), ((0, 2), identity_rows([7])), ((1, 2), identity_rows([8]))]
    script = start(poses) + QUERIES + [("register", (2, poses[2][0], poses[2][1], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4])), ("kill", ([9],))]
    script += QUERIES + [("drop", ([1, 2, 1, 0], [7, 3, 7, 9], 2))] + QUERIES + [("triangulate", (2, K))] + QUERIES
    script += [("drop", ([], [], 3))] + QUERIES
    return kps, pairs, script


# ---- refusals of amvs_sfm_register -----------------------------------------------------------------------------------------
def register_refusals():
    """(kps, pairs, script, refused): `refused` are calls that must each be refused and leave the state as it was."""
    poses, kps, _ = planted(3, 8, seed=2)
    pairs = [((0, 1), identity_rows(range(8)))]
    R, t = poses[2]
    refused = [("register", (0, R, t)), ("register", (3, R, t)), ("register", (-1, R, t)),
               ("register", (2, R, t, [0, 0], [1, 2])), ("register", (2, R, t, [0, 1], [2, 2])),
               ("register", (2, R, t, [8], [0])), ("register", (2, R, t, [-1], [0])), ("register", (2, R, t, [0], [8])),
               ("register", (2, R, t, [0], [-1]))]
    script = start(poses) + [("kill", ([4],))]
    after = [("register", (2, R, t, [0, 0, 3, 5, 7], [1, 1, 4, 5, 8], [1, 0, 1, 1, 0]))] + QUERIES     # masked rows are not checked
    return kps, pairs, script, refused, after


# ---- seeded random states ----------------------------------------------------------------------------------------------------
def random_case(seed):
    """V = 5, up to 40 keypoints a view in a random order, one-to-one rows between the views' common tracks with a few wrong
    matches, pixel noise of half a pixel, and a script that walks the whole interface: the views enter in a random order with
    a random mask over their correspondences, points die, observations are dropped."""
    rng = np.random.default_rng(1000 + seed)
    V, N = 5, 40
    poses, full, _ = planted(V, N, seed=2000 + seed, noise=0.5)
    tracks = [rng.permutation(N)[: rng.integers(25, N + 1)] for _ in range(V)]          # tracks[v][k] = the track of keypoint k
    kps = [full[v][tracks[v]] for v in range(V)]
    pairs = []
    for i in range(V):
        for j in range(i + 1, V):
            if (i, j) != (0, 1) and rng.random() < 0.15:
                continue
            where_j = {int(tr): k for k, tr in enumerate(tracks[j])}
            rows = [(k, where_j[int(tr)]) for k, tr in enumerate(tracks[i]) if int(tr) in where_j and rng.random() < 0.8]
            rows = np.array(rows, np.int32).reshape(-1, 2)
            if len(rows) > 4:                                                               # wrong matches, still one-to-one
                sel = rng.choice(len(rows), 3, replace=False)
                rows[sel, 1] = rows[np.roll(sel, 1), 1]
            rows = rows[rng.permutation(len(rows))]
            pairs.append(((i, j), rows))
    order = [int(v) for v in rng.permutation(np.arange(2, V))]
    script = start(poses) + list(QUERIES)
    for n, v in enumerate(order):
        script += [("correspondences", (v,)), ("register_from", (v, poses[v][0], poses[v][1], int(rng.integers(1 << 30)))),
                   ("triangulate", (v, K)), ("counts", ()), ("scores", ())]
        if n == 0:
            script += [("kill_random", (int(rng.integers(1 << 30)), 0.2))]
        script += [("drop_random", (int(rng.integers(1 << 30)), 0.15, 2))] + QUERIES
    return kps, pairs, script


# ---- playing a script ----------------------------------------------------------------------------------------------------------
def play(backend, script, refusals):
    """Every step's result, in order; "refused" for a step the backend refuses with one of `refusals`.  A backend has the
    methods of tests/sfm_state_restatement.py's State."""
    log = []
    for name, args in script:
        try:
            if name == "kill":
                X, alive = backend.points()
                alive = alive.copy()
                alive[list(args[0])] = False
                out = backend.set_points(X, alive)
            elif name == "kill_random":
                X, alive = backend.points()
                alive = alive & (np.random.default_rng(args[0]).random(len(alive)) >= args[1])
                out = backend.set_points(X, alive)
            elif name == "register_from":
                v, R, t, seed = args
                kp, pid, _, _ = backend.correspondences(v)
                out = backend.register(v, R, t, kp, pid, np.random.default_rng(seed).random(len(kp)) < 0.8)
            elif name == "drop_random":
                cam, pt, _ = backend.observations()
                sel = np.random.default_rng(args[0]).random(len(cam)) < args[1]
                out = backend.drop(cam[sel], pt[sel], args[2])
            else:
                out = getattr(backend, name)(*args)
        except refusals:
            out = "refused"
        log.append((name, out))
    return log


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(a, b):
    """Integers equal, floating-point arrays bit for bit, tuples entry by entry."""
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(same_result(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            return same_bits(a, b)
        return a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))
    return a == b


def first_difference(log_a, log_b):
    """None, or (step number, step name) of the first step whose results differ."""
    if len(log_a) != len(log_b):
        return (min(len(log_a), len(log_b)), "length")
    for n, ((name, a), (_, b)) in enumerate(zip(log_a, log_b)):
        if not same_result(a, b):
            return (n, name)
    return None

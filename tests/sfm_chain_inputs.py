"""Planted scenes for the chain of the sparse-reconstruction stages (tests/sfm_chain.py), shared by
tests/test_sfm_chain_cpu.py and tests/test_hip_sfm_chain.py: true poses, 160 points, per view a list of keypoints and
per pair of views a list of matches, some of them false.  The cameras, the cloud and the projection are those of
tests/bundle_inputs.py.  Everything is a function of the scene's name; nothing is random between runs, and every view
and every pair draws from a generator of its own, so the views and pairs that two scenes share are the same in both.

A scene is a dict:
    K (3, 3); R (V, 9), t (V, 3): the true poses, Xc = R X + t; X (160, 3)
    keypoints[v] (n_v, 2) float32 pixels; track[v] (n_v,) the planted track id of every keypoint, for the checks only:
        the index of its point in X, or -1 for a keypoint planted off every track (FALSE_TRACK)
    matches[(i, j)], i < j: (m, 2) int32 keypoint indices of view i and view j, in a shuffled order."""
import numpy as np

import bundle_inputs as bi

K = bi.K
N_POINTS = 160
P_SEEN, MIN_VIEWS = 0.7, 3
FALSE_FRACTION = 0.2                      # false matches per pair, relative to the true ones
NOISE_PX = 0.5
REPLACED_FRACTION = 0.1                   # noisy: true matches replaced by an epipolar-consistent false one
LAMBDA_RANGES = ((0.6, 0.8), (1.3, 1.6))  # where along the ray of view i the replaced match's point lies
FALSE_TRACK = -1
SEED = 6                                  # (see tests/test_sfm_chain_cpu.py for what was asked of it)
ROTATION_ONLY_DEG = 4.0                   # edges: view 6 is view 2 turned about its own y axis
FAR_VIEW_CENTRE = (1.0, 1.5, -6.5)        # edges: view 7
FAR_VIEW_KEYPOINTS = 5
NAMES = ("clean", "noisy", "edges")


def centre(R, t):
    return -(np.asarray(R).reshape(3, 3).T @ np.asarray(t).reshape(3))


def _poses(name):
    R, t = bi.cameras(6)
    if name != "edges":
        return R, t
    a = np.deg2rad(ROTATION_ONLY_DEG)
    turn = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    R6 = turn @ R[2].reshape(3, 3)
    t6 = -R6 @ centre(R[2], t[2])                                   # the centre of view 2: no baseline between the two
    R7, t7 = bi.look_at(FAR_VIEW_CENTRE)
    return np.concatenate([R, [R6.reshape(9), R7.reshape(9)]]), np.concatenate([t, [t6, t7]])


def _visibility(name):
    """vis (160, V) bool.  The first six columns are the same in every scene."""
    rng = np.random.default_rng([SEED, 0])
    vis = rng.random((N_POINTS, 6)) < P_SEEN
    for p in range(N_POINTS):
        while vis[p].sum() < MIN_VIEWS:
            vis[p, rng.integers(6)] = True
    if name == "edges":
        more = np.random.default_rng([SEED, 0, 1])
        v6 = more.random(N_POINTS) < P_SEEN
        v7 = np.zeros(N_POINTS, bool)
        v7[more.choice(N_POINTS, FAR_VIEW_KEYPOINTS, replace=False)] = True
        vis = np.concatenate([vis, v6[:, None], v7[:, None]], axis=1)
    return vis


def _pixels(R, t, v, X):
    """The exact pixels (n, 2) float64 of the points X (n, 3) in view v."""
    n = len(X)
    return bi.project(R, t, X, np.full(n, v), np.arange(n))


def scene(name):
    assert name in NAMES
    noise = 0.0 if name == "clean" else NOISE_PX
    R, t = _poses(name)
    V = len(R)
    X = bi.cloud(N_POINTS, np.random.default_rng([SEED, 3]))
    vis = _visibility(name)
    keypoints, track, at = [], [], []
    for v in range(V):
        rng = np.random.default_rng([SEED, 1, v])
        ids = rng.permutation(np.flatnonzero(vis[:, v]))             # (a keypoint's index says nothing about its track)
        uv = _pixels(R, t, v, X[ids])
        if noise:
            uv = uv + noise * rng.standard_normal(uv.shape)
        keypoints.append([row for row in uv.astype(np.float32)])
        track.append(list(ids))
        at.append({int(p): k for k, p in enumerate(ids)})            # track id -> keypoint index
    matches = {}
    for i in range(V):
        for j in range(i + 1, V):
            rng = np.random.default_rng([SEED, 2, i, j])
            both = np.flatnonzero(vis[:, i] & vis[:, j])
            rows = [(at[i][p], at[j][p]) for p in both]
            if noise:
                Ci = centre(R[i], t[i])
                for r in rng.choice(len(rows), int(round(REPLACED_FRACTION * len(rows))), replace=False):
                    lo, hi = LAMBDA_RANGES[rng.integers(2)]
                    Y = Ci + rng.uniform(lo, hi) * (X[both[r]] - Ci)
                    keypoints[j].append(_pixels(R, t, j, Y[None])[0].astype(np.float32))
                    # (seen from the centre of view i itself the point hides behind the track's own: no false keypoint)
                    track[j].append(FALSE_TRACK if np.linalg.norm(centre(R[j], t[j]) - Ci) > 1e-9 else both[r])
                    rows[r] = (rows[r][0], len(keypoints[j]) - 1)
            only_i, only_j = np.flatnonzero(vis[:, i] & ~vis[:, j]), np.flatnonzero(vis[:, j] & ~vis[:, i])
            n_false = min(int(round(FALSE_FRACTION * len(both))), len(only_i), len(only_j))
            for a, b in zip(rng.choice(only_i, n_false, replace=False), rng.choice(only_j, n_false, replace=False)):
                rows.append((at[i][a], at[j][b]))
            if rows:
                matches[(i, j)] = np.array(rows, np.int32)[rng.permutation(len(rows))]
    return {"name": name, "K": K, "R": R, "t": t, "X": X,
            "keypoints": [np.array(k, np.float32).reshape(-1, 2) for k in keypoints],
            "track": [np.array(k, np.int64) for k in track], "matches": matches}


def true_match(sc, pair, row):
    """Whether a match of the pair joins two keypoints of one planted track."""
    i, j = pair
    a, b = sc["track"][i][row[0]], sc["track"][j][row[1]]
    return a == b and a != FALSE_TRACK


def false_pair(m=60, seed=5):
    """(pts1, pts2) (m, 2) float32: the keypoints of m different tracks in view 0 against those of m other tracks in view 3
    of the clean scene; no match is true."""
    sc = scene("clean")
    rng = np.random.default_rng([SEED, 4, seed])
    k0 = rng.permutation(len(sc["keypoints"][0]))
    k3 = rng.permutation(len(sc["keypoints"][3]))
    rows = []
    for a in k0:
        for b in k3:
            if sc["track"][0][a] != sc["track"][3][b] and all(b != r[1] for r in rows):
                rows.append((a, b))
                break
        if len(rows) == m:
            break
    rows = np.array(rows)
    return sc["keypoints"][0][rows[:, 0]], sc["keypoints"][3][rows[:, 1]]

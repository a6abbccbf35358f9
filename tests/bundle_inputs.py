"""Planted scenes for the bundle adjustment (include/amvs_bundle.h), shared by tests/test_bundle_cpu.py and
tests/test_hip_bundle.py: cameras on an arc in front of a cloud (and, on request, one on the far side looking back), a
visibility matrix, pixels with or without noise, and perturbed starting states.  Everything is a function of its
arguments; nothing is random between runs."""
import numpy as np

K = np.array([[1500.0, 0.0, 960.0], [0.0, 1500.0, 540.0], [0.0, 0.0, 1.0]])
FLIP = np.diag([-1.0, 1.0, -1.0])          # a pose composed with it has every point behind it that was in front


def look_at(centre, target=(0.0, 0.0, 0.0)):
    """(R (3, 3), t (3,)) of a camera at `centre` looking at `target`, y down as far as it can be."""
    c = np.asarray(centre, np.float64)
    z = np.asarray(target, np.float64) - c
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ c


def cameras(C, back=False):
    """R (C, 9), t (C, 3): cameras on an arc at z = -6 looking at the origin; with back, the last one sits at z = +12 and
    looks back at it."""
    Rs, ts = [], []
    for c in range(C):
        a = (c - 0.5 * (C - 1)) * (1.2 / max(C - 1, 1))
        centre = (6.0 * np.sin(a), 0.3 * ((c % 3) - 1), -6.0 * np.cos(a))
        if back and c == C - 1:
            centre = (0.5, -0.2, 12.0)
        R, t = look_at(centre)
        Rs.append(R.reshape(9))
        ts.append(t)
    return np.array(Rs), np.array(ts)


def project(R, t, X, cam, pt):
    """Pixels (N, 2) float64 of the observations (cam[k], pt[k]); no test of the depth."""
    Rm = R.reshape(-1, 3, 3)[cam]
    Xc = np.einsum("nij,nj->ni", Rm, X[pt]) + t[cam]
    with np.errstate(all="ignore"):
        return np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1)


def observations(vis):
    """(cam, pt) int32 of a visibility matrix vis (P, C), strictly ascending in (pt, cam)."""
    pt, cam = np.nonzero(vis)
    return cam.astype(np.int32), pt.astype(np.int32)


def random_visibility(C, P, rng, mean_track=4):
    """vis (P, C): every point seen by at least two cameras, about mean_track on average; point 0 by every camera."""
    vis = rng.random((P, C)) < (mean_track / C)
    for p in range(P):
        while vis[p].sum() < min(2, C):
            vis[p, rng.integers(C)] = True
    vis[0, :] = True                                # (one point that every camera sees)
    return vis


def cloud(P, rng):
    return rng.uniform(-1.5, 1.5, (P, 3))


def make(R, t, X, vis, noise=0.0, seed=0):
    """A scene dict from the true state and a visibility matrix: pixels are the projections plus Gaussian noise, as float32."""
    cam, pt = observations(vis)
    uv = project(R, t, X, cam, pt)
    if noise:
        uv = uv + noise * np.random.default_rng(seed + 77).standard_normal(uv.shape)
    uv = np.where(np.isfinite(uv), uv, 0.0)
    return {"R": R.copy(), "t": t.copy(), "X": X.copy(), "cam": cam, "pt": pt, "uv": uv.astype(np.float32), "C": len(R), "P": len(X)}


def scene(C, P, seed=0, noise=0.0, mean_track=4):
    rng = np.random.default_rng(seed)
    R, t = cameras(C)
    X = cloud(P, rng)
    return make(R, t, X, random_visibility(C, P, rng, mean_track), noise, seed)


def small_rotation(w):
    """exp of the skew matrix of w, by Rodrigues' formula."""
    a = np.linalg.norm(w)
    if a == 0.0:
        return np.eye(3)
    k = np.asarray(w) / a
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)


def perturbed(sc, keep, rot=0.01, trans=0.02, pts=0.02, seed=1):
    """(R, t, X) of a start near the truth: the cameras of the mask `keep` stay at the truth."""
    rng = np.random.default_rng(seed)
    R, t, X = sc["R"].copy(), sc["t"].copy(), sc["X"].copy()
    for c in range(sc["C"]):
        if keep[c]:
            continue
        R[c] = (small_rotation(rot * rng.standard_normal(3)) @ R[c].reshape(3, 3)).reshape(9)
        t[c] = t[c] + trans * rng.standard_normal(3)
    return R, t, X + pts * rng.standard_normal(X.shape)


def fixed_mask(C, *which):
    m = np.zeros(C, np.uint8)
    m[list(which)] = 1
    return m


# ---- the scene of list lengths and point kinds -------------------------------------------------------------------------------
LIST_LENGTHS = (129, 1, 63, 64, 65, 129, 29)       # camera 6 sees points 100 .. 128 only: it shares nothing with camera 2


def lists_scene(noise=0.3):
    """Eight cameras.  The lists of cameras 1 .. 5 have exactly the lengths LIST_LENGTHS[1:6]: camera c < 6 sees points
    0 .. length - 1; camera 6 sees points 100 .. 128 and camera 7, on the far side looking back, points 0 .. 39.  So the
    pair segments of free cameras have the lengths 0 (cameras 1 or 2 and 6), 1 (camera 1 and cameras 2 .. 5), 63, 64
    (cameras 3 and 4, 3 and 5), 65 (cameras 4 and 5) and 29.  Then four special points, seen by cameras 0, 6 and 7 only:
        129: seen by camera 6 alone (one observation: held)
        130: behind cameras 0 and 6, its only ones (no active observation)
        131: in front of camera 6, behind camera 7 (one active and one inactive observation: held)
        132: seen by cameras 0 and 7 (with both of them fixed: observed only by fixed cameras)."""
    rng = np.random.default_rng(5)
    C, P = 8, 133
    R, t = cameras(C, back=True)
    X = cloud(P, rng)
    X[130] = (0.2, 0.1, -20.0)
    X[131] = (0.1, -0.3, 20.0)
    vis = np.zeros((P, C), bool)
    for c, n in enumerate(LIST_LENGTHS[:6]):
        vis[:n, c] = True
    vis[100:129, 6] = True
    vis[:40, 7] = True
    vis[129, 6] = True
    vis[130, [0, 6]] = True
    vis[131, [6, 7]] = True
    vis[132, [0, 7]] = True
    return make(R, t, X, vis, noise, 5)


def with_idle(sc, c):
    """(R, t) of the scene with camera c turned round: every observation of it is inactive."""
    R, t = sc["R"].copy(), sc["t"].copy()
    R[c] = (FLIP @ R[c].reshape(3, 3)).reshape(9)
    t[c] = FLIP @ t[c]
    return R, t


def with_outliers(sc, n=2, shift=120.0):
    """The scene with the pixels of n observations moved by `shift` pixels."""
    out = dict(sc)
    uv = sc["uv"].astype(np.float64).copy()
    at = np.linspace(3, len(uv) - 4, n).astype(int)
    uv[at] += shift
    out["uv"] = uv.astype(np.float32)
    return out, at

"""include/amvs_sfm.h restated in plain Python / NumPy, from the header's text alone: sequential loops over dictionaries and
lists, no launch shape, no atomics, no sort but sorted().  The triangulation is tests/twoview_restatement.py's.  The
device is compared with this: integers exactly, points bit for bit (tests/test_hip_sfm_state.py); its own properties are
checked in tests/test_sfm_state_cpu.py."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twoview_restatement as tv  # noqa: E402

BLOCK = 256
MAX_VIEWS, MAX_KEYPOINTS, MAX_ROWS, MAX_POINTS = 4096, 1 << 28, 1 << 28, 1 << 22
MIN_SCORE, MIN_OBS = 12, 2


class Refused(ValueError):
    """An AMVS_EINVAL of the header."""


class State:
    def __init__(self, keypoints, pairs):
        """amvs_sfm_begin.  keypoints: per view (n_v, 2) pixels; pairs: a list of ((i, j), rows (m, 2)) in the caller's order."""
        V = len(keypoints)
        if V < 1 or V > MAX_VIEWS:
            raise Refused("V")
        self.kp = [np.asarray(k, np.float32).reshape(-1, 2) for k in keypoints]
        self.pairs, last = [], None
        for (i, j), rows in pairs:
            rows = np.asarray(rows, np.int64).reshape(-1, 2)
            if not (0 <= i < j < V):
                raise Refused("pair")
            if last is not None and not (last < (i, j)):
                raise Refused("order")
            last = (i, j)
            for side, view in ((0, i), (1, j)):
                col = [int(k) for k in rows[:, side]]
                if any(k < 0 or k >= len(self.kp[view]) for k in col):
                    raise Refused("range")
                if len(set(col)) != len(col):
                    raise Refused("twice")
            self.pairs.append(((i, j), rows))
        # rank of a row = its position in the concatenation
        self.rank0, m = [], 0
        for _, rows in self.pairs:
            self.rank0.append(m)
            m += len(rows)
        self.V = V
        self.owner = [[-1] * len(k) for k in self.kp]
        self.registered = [False] * V
        self.pose = [None] * V
        self.X, self.alive = [], []

    # ---- helpers -----------------------------------------------------------------------------------------------------
    def n_points(self):
        return len(self.X)

    def candidates(self, view):
        """(rank, k of view, point) for every row of a pair of `view` with a registered view whose keypoint there is owned."""
        out = []
        for p, ((i, j), rows) in enumerate(self.pairs):
            if view not in (i, j):
                continue
            r = j if view == i else i
            if not self.registered[r]:
                continue
            for n, (ki, kj) in enumerate(rows):
                k, kr = (int(ki), int(kj)) if view == i else (int(kj), int(ki))
                if self.owner[r][kr] >= 0:
                    out.append((self.rank0[p] + n, k, self.owner[r][kr]))
        return out

    # ---- the entry points --------------------------------------------------------------------------------------------
    def register(self, view, R, t, kp=(), pid=(), mask=None):
        if not (0 <= view < self.V) or self.registered[view]:
            raise Refused("view")
        rows = [(int(k), int(p)) for n, (k, p) in enumerate(zip(kp, pid)) if mask is None or mask[n]]
        for k, p in rows:
            if not (0 <= k < len(self.kp[view])) or not (0 <= p < self.n_points()):
                raise Refused("range")
        if len({k for k, _ in rows}) != len(rows) or len({p for _, p in rows}) != len(rows):
            raise Refused("repeated")
        self.registered[view] = True
        self.pose[view] = (np.asarray(R, np.float64).reshape(3, 3).copy(), np.asarray(t, np.float64).reshape(3).copy())
        n_set = 0
        for k, p in rows:
            if self.alive[p]:
                self.owner[view][k] = p
                n_set += 1
        return n_set

    def scores(self):
        out = np.zeros(self.V, np.int32)
        for v in range(self.V):
            out[v] = -1 if self.registered[v] else len({k for _, k, _ in self.candidates(v)})
        return out

    def correspondences(self, view):
        if not (0 <= view < self.V) or self.registered[view]:
            raise Refused("view")
        a, p_of = {}, {}
        for rank, k, p in self.candidates(view):                 # stage A
            if k not in a or rank < a[k]:
                a[k], p_of[k] = rank, p
        b = {}
        for k, rank in a.items():                                # stage B
            if p_of[k] not in b or rank < b[p_of[k]]:
                b[p_of[k]] = rank
        kept = [k for k in sorted(a) if a[k] == b[p_of[k]]]
        kp = np.array(kept, np.int32)
        pid = np.array([p_of[k] for k in kept], np.int32)
        X = np.array([self.X[p] for p in pid], np.float64).reshape(-1, 3).astype(np.float32)
        x = self.kp[view][kp] if kept else np.zeros((0, 2), np.float32)
        return kp, pid, X, x

    @staticmethod
    def baseline(pose1, pose2):
        C = []
        for R, t in (pose1, pose2):
            C.append([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])
        d = [C[1][i] - C[0][i] for i in range(3)]
        return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])

    def triangulate(self, view, K, depth_min=tv.DEPTH_MIN, depth_baselines=tv.DEPTH_BASELINES, cos_max_parallax=None,
                    max_reproj=tv.MAX_REPROJ):
        if not (0 <= view < self.V) or not self.registered[view]:
            raise Refused("view")
        if self.n_points() + len(self.kp[view]) > MAX_POINTS:
            raise Refused("limit")
        if cos_max_parallax is None:
            cos_max_parallax = float(np.cos(np.deg2rad(tv.MIN_PARALLAX_DEG)))
        per = np.zeros(self.V, np.int32)
        for r in range(self.V):
            if r == view or not self.registered[r]:
                continue
            lo, hi = min(view, r), max(view, r)
            found = [rows for (pair, rows) in self.pairs if pair == (lo, hi)]
            if not found:
                continue
            cand = [(int(ki), int(kj)) for ki, kj in found[0] if self.owner[lo][int(ki)] < 0 and self.owner[hi][int(kj)] < 0]
            if not cand:
                continue
            (R1, t1), (R2, t2) = self.pose[lo], self.pose[hi]
            with np.errstate(all="ignore"):
                depth_max = np.float64(self.baseline(self.pose[lo], self.pose[hi])) * np.float64(depth_baselines)
            p1 = np.array([self.kp[lo][ki] for ki, _ in cand], np.float32)
            p2 = np.array([self.kp[hi][kj] for _, kj in cand], np.float32)
            X, valid, _ = tv.triangulate(K, R1, t1, R2, t2, p1, p2, depth_min, float(depth_max), cos_max_parallax, max_reproj)
            for n, (ki, kj) in enumerate(cand):
                if valid[n]:
                    self.owner[lo][ki] = self.owner[hi][kj] = self.n_points()
                    self.X.append(np.array(X[n], np.float64))
                    self.alive.append(True)
                    per[r] += 1
        return int(per.sum()), per

    def counts(self):
        return self.n_points(), int(sum(self.alive)), sum(1 for o in self.owner for p in o if p >= 0)

    def observations(self):
        obs = sorted((p, v, k) for v, o in enumerate(self.owner) for k, p in enumerate(o) if p >= 0)
        cam = np.array([v for _, v, _ in obs], np.int32)
        pt = np.array([p for p, _, _ in obs], np.int32)
        uv = np.array([self.kp[v][k] for _, v, k in obs], np.float32).reshape(-1, 2)
        return cam, pt, uv

    def points(self):
        return np.array(self.X, np.float64).reshape(-1, 3), np.array(self.alive, bool)

    def unown_dead(self):
        for o in self.owner:
            for k, p in enumerate(o):
                if p >= 0 and not self.alive[p]:
                    o[k] = -1

    def set_points(self, X, alive):
        X, alive = np.asarray(X, np.float64).reshape(-1, 3), [bool(a) for a in alive]
        if len(X) != self.n_points() or len(alive) != self.n_points():
            raise Refused("n")
        if any(a and not b for a, b in zip(alive, self.alive)):
            raise Refused("back")
        self.X, self.alive = [x.copy() for x in X], alive
        self.unown_dead()

    def set_pose(self, view, R, t):
        if not (0 <= view < self.V) or not self.registered[view]:
            raise Refused("view")
        self.pose[view] = (np.asarray(R, np.float64).reshape(3, 3).copy(), np.asarray(t, np.float64).reshape(3).copy())

    def drop(self, cam, pt, min_obs=MIN_OBS):
        named = [(int(c), int(p)) for c, p in zip(cam, pt)]
        if min_obs < 0 or any(not (0 <= c < self.V) or not (0 <= p < self.n_points()) for c, p in named):
            raise Refused("range")
        obs_dropped = 0
        for c, p in named:
            for k, o in enumerate(self.owner[c]):
                if o == p:
                    self.owner[c][k] = -1
                    obs_dropped += 1
        left = [0] * self.n_points()
        for o in self.owner:
            for p in o:
                if p >= 0:
                    left[p] += 1
        points_dropped = 0
        for p in range(self.n_points()):
            if self.alive[p] and left[p] < min_obs:
                self.alive[p] = False
                points_dropped += 1
        self.unown_dead()
        return obs_dropped, points_dropped

    # ---- what the tests compare ----------------------------------------------------------------------------------------
    def owners(self):
        return [list(o) for o in self.owner]

"""CPU restatement (NumPy, float32) of the EXTENDED PatchMatch mode's kernels
(3d-reconstruction-tool_amd/csrc/amvs_extended.hip): the slanted-plane window cost `xcost_t`, the
view-propagation candidates and one red-black half sweep.

TEST INFRASTRUCTURE ONLY (imported by tests/test_extended_oracle.py).  The extended mode has NO
reference counterpart -- the reference's docstring names plane normals and view propagation
(mvs_patchmatch.py:1-13), its code implements neither (:323-390, :415-457) -- so this file is not pinned
against reference outputs: it is an independent second implementation of the same specification,
written from the kernel's documented arithmetic, against which the HIP kernels are compared with a
STATED TOLERANCE (the kernels use v_rcp_f32 / v_rsq_f32, exp / log of the device library and real
FMAs; this file uses IEEE division / sqrt, NumPy's exp / log and FMAs emulated in float64).

Ref64 (below) is the float64 reference of every extended-mode kernel -- window cost in both samplings and
both window loops, half sweep, consistency, initial state -- with per-pixel decision margins
(tests/test_extended_paths.py).

Conventions: images are 8-bit codes (H, W) uint8; gray = code / 255 in float32; state maps depth
(H, W), normal (H, W, 3), cost (H, W) float32; K, K_inv float32 3x3 (K_inv as the engine forms it:
the float32 inverse); poses (R, t) world -> camera.
"""
import numpy as np

F = np.float32
INF = F(np.inf)


def fma(a, b, c):
    """fmaf emulated through float64 (the product of two float32 is exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def compose(K, Rr, tr, Rs, ts):
    """fast_compose (csrc/amvs_kernels_fast.hip): M = K R_s R_ref^T K^-1, b = K (t_s - R_s R_ref^T t_ref) in
    double on the float32 operands, sums left to right, K^-1 by cofactors, one rounding at the end."""
    Kd = np.asarray(K, np.float32).astype(np.float64).reshape(9)
    Rr = np.asarray(Rr, np.float32).astype(np.float64).reshape(9)
    Rs = np.asarray(Rs, np.float32).astype(np.float64).reshape(9)
    tr = np.asarray(tr, np.float32).astype(np.float64).reshape(3)
    ts = np.asarray(ts, np.float32).astype(np.float64).reshape(3)
    det = Kd[0] * (Kd[4] * Kd[8] - Kd[5] * Kd[7]) - Kd[1] * (Kd[3] * Kd[8] - Kd[5] * Kd[6]) + Kd[2] * (Kd[3] * Kd[7] - Kd[4] * Kd[6])
    Ki = np.array([(Kd[4] * Kd[8] - Kd[5] * Kd[7]) / det, (Kd[2] * Kd[7] - Kd[1] * Kd[8]) / det, (Kd[1] * Kd[5] - Kd[2] * Kd[4]) / det,
                   (Kd[5] * Kd[6] - Kd[3] * Kd[8]) / det, (Kd[0] * Kd[8] - Kd[2] * Kd[6]) / det, (Kd[2] * Kd[3] - Kd[0] * Kd[5]) / det,
                   (Kd[3] * Kd[7] - Kd[4] * Kd[6]) / det, (Kd[1] * Kd[6] - Kd[0] * Kd[7]) / det, (Kd[0] * Kd[4] - Kd[1] * Kd[3]) / det])
    Rrel = np.empty(9)
    for i in range(3):
        for j in range(3):
            Rrel[3 * i + j] = (Rs[3 * i] * Rr[3 * j] + Rs[3 * i + 1] * Rr[3 * j + 1]) + Rs[3 * i + 2] * Rr[3 * j + 2]
    trel = np.array([ts[i] - ((Rrel[3 * i] * tr[0] + Rrel[3 * i + 1] * tr[1]) + Rrel[3 * i + 2] * tr[2]) for i in range(3)])
    A = np.empty(9)
    for i in range(3):
        for j in range(3):
            A[3 * i + j] = (Kd[3 * i] * Rrel[j] + Kd[3 * i + 1] * Rrel[3 + j]) + Kd[3 * i + 2] * Rrel[6 + j]
    M = np.empty(9, np.float32)
    b = np.empty(3, np.float32)
    for i in range(3):
        for j in range(3):
            M[3 * i + j] = np.float32((A[3 * i] * Ki[j] + A[3 * i + 1] * Ki[3 + j]) + A[3 * i + 2] * Ki[6 + j])
        b[i] = np.float32((Kd[3 * i] * trel[0] + Kd[3 * i + 1] * trel[1]) + Kd[3 * i + 2] * trel[2])
    return M, b


def normalise_facing(nx, ny, nz):
    """xnormalise_facing: unit length; planes that do not face the camera become fronto-parallel."""
    l = np.sqrt(nx * nx + ny * ny + nz * nz)
    with np.errstate(divide="ignore", invalid="ignore"):
        il = np.where(l > F(1e-12), F(1.0) / l, F(0.0)).astype(np.float32)
    nx, ny, nz = nx * il, ny * il, nz * il
    bad = ~(nz < F(-0.05))
    return (np.where(bad, F(0), nx).astype(np.float32), np.where(bad, F(0), ny).astype(np.float32),
            np.where(bad, F(-1), nz).astype(np.float32))


class View:
    """One reference view of a scene with its source views (a Job of the device job table)."""

    def __init__(self, K, K_inv, codes, poses, ref, srcs, patch, stride):
        self.K = np.asarray(K, np.float32).reshape(3, 3)
        self.Ki = np.asarray(K_inv, np.float32).reshape(9)
        self.codes = [np.asarray(c, np.uint8) for c in codes]
        self.poses = [(np.asarray(R, np.float64).astype(np.float32).reshape(9), np.asarray(t, np.float64).astype(np.float32).reshape(3))
                      for R, t in poses]
        self.ref, self.srcs = int(ref), [int(s) for s in srcs]
        self.H, self.W = self.codes[0].shape
        self.patch, self.stride = int(patch), int(stride)
        self.N = (self.patch - 1) // self.stride + 1
        assert (self.N - 1) * self.stride + 1 == self.patch, "restated for N x N tap windows only"
        Rr, tr = self.poses[self.ref]
        self.Mb = [compose(self.K, Rr, tr, *self.poses[s]) for s in self.srcs]
        self.gray = self.codes[self.ref].astype(np.float32) / F(255.0)
        self.padded = {v: np.pad(self.codes[v], 3) for v in set(self.srcs)}    # zero border (2 texels + the pair's +1)
        ys, xs = np.meshgrid(np.arange(self.H), np.arange(self.W), indexing="ij")
        self.xs, self.ys = xs.ravel(), ys.ravel()

    # ---------------------------------------------------------------- cost -----
    def _ray(self, x, y):
        k = self.Ki
        fx, fy = x.astype(np.float32), y.astype(np.float32)
        return fma(k[1], fy, fma(k[0], fx, k[2])), fma(k[4], fy, fma(k[3], fx, k[5]))

    def cost(self, x, y, d, nx, ny, nz):
        """xcost_t<N, U8 = true> for the pixels (x[i], y[i]) with hypotheses (d[i], n[i])."""
        H, W, N, st, half = self.H, self.W, self.N, self.stride, self.patch // 2
        k = self.Ki
        P = x.shape[0]
        out = np.full(P, INF, np.float32)
        inside = (x - half >= 0) & (y - half >= 0) & (x - half + (N - 1) * st < W) & (y - half + (N - 1) * st < H)
        rpx, rpy = self._ray(x, y)
        ndr_p = fma(nx, rpx, fma(ny, rpy, nz))
        live = inside & (ndr_p < F(-1e-6))
        delta = d * ndr_p
        w0 = fma(ny, k[3], nx * k[0])
        w1 = fma(ny, k[4], nx * k[1])
        w2 = fma(ny, k[5], fma(nx, k[2], nz))
        stf = F(st)
        x0 = (x - half).astype(np.float32)
        y0 = (y - half).astype(np.float32)
        cx = [x0, x0 + F(N - 1) * stf]
        cy = [y0, y0 + F(N - 1) * stf]
        ndr_c = [fma(w0, cx[c & 1], fma(w1, cy[c >> 1], w2)) for c in range(4)]
        live &= np.maximum(np.maximum(ndr_c[0], ndr_c[1]), np.maximum(ndr_c[2], ndr_c[3])) < F(-1e-6)
        # reference taps (xref_load): sums in tap order
        xi = np.clip(x - half, 0, W - 1 - (N - 1) * st)
        yi = np.clip(y - half, 0, H - 1 - (N - 1) * st)
        taps = [[self.gray[yi + j * st, xi + i * st] for i in range(N)] for j in range(N)]
        sr = np.zeros(P, np.float32)
        srr = np.zeros(P, np.float32)
        for j in range(N):
            for i in range(N):
                sr = sr + taps[j][i]
                srr = fma(taps[j][i], taps[j][i], srr)
        INV = F(1.0 / float(N * N))
        vr = srr - sr * sr * INV
        fw, fh = F(W - 1), F(H - 1)
        costs = np.full((6, P), INF, np.float32)
        n_valid = np.zeros(P, np.int32)
        with np.errstate(all="ignore"):
            for s, (M, b) in zip(self.srcs, self.Mb):
                img = self.padded[s]
                Hm = [fma(b[r], (w0, w1, w2)[c], delta * M[3 * r + c]) for r in range(3) for c in range(3)]
                ok = live.copy()
                for c in range(4):
                    qx, qy = cx[c & 1], cy[c >> 1]
                    p0 = fma(Hm[0], qx, fma(Hm[1], qy, Hm[2]))
                    p1 = fma(Hm[3], qx, fma(Hm[4], qy, Hm[5]))
                    p2 = fma(Hm[6], qx, fma(Hm[7], qy, Hm[8]))
                    ok &= p2 < F(0.1) * ndr_c[c]
                    rz = F(1.0) / p2
                    u, v = p0 * rz, p1 * rz
                    ok &= (u >= 0) & (v >= 0) & (u < fw) & (v < fh)
                sv = np.zeros(P, np.float32)
                svv = np.zeros(P, np.float32)
                srv = np.zeros(P, np.float32)
                for j in range(N):
                    qy = y0 + F(j) * stf
                    p0 = fma(Hm[0], x0, fma(Hm[1], qy, Hm[2]))
                    p1 = fma(Hm[3], x0, fma(Hm[4], qy, Hm[5]))
                    p2 = fma(Hm[6], x0, fma(Hm[7], qy, Hm[8]))
                    for i in range(N):
                        rz = F(1.0) / p2                       # (v_rcp_f32 on the device: 1 ulp)
                        u, v = p0 * rz, p1 * rz
                        x0f, y0f = np.floor(u), np.floor(v)
                        # no clamp: the packed maps carry a zero border of 2 texels (pixels whose corner
                        # tests failed are masked below; their indices are only kept inside the array)
                        xq = np.clip(np.nan_to_num(x0f, nan=0.0, posinf=0.0, neginf=0.0), -2, W).astype(np.int64) + 3
                        yq = np.clip(np.nan_to_num(y0f, nan=0.0, posinf=0.0, neginf=0.0), -2, H).astype(np.int64) + 3
                        fx, fy = u - x0f, v - y0f
                        t00 = img[yq, xq].astype(np.float32)
                        t10 = img[yq + 1, xq].astype(np.float32)
                        t01 = img[yq, xq + 1].astype(np.float32)
                        t11 = img[yq + 1, xq + 1].astype(np.float32)
                        top = fma(fx, t01 - t00, t00)
                        bot = fma(fx, t11 - t10, t10)
                        sval = fma(fy, bot - top, top)
                        sv = sv + sval
                        svv = fma(sval, sval, svv)
                        srv = fma(taps[j][i], sval, srv)
                        p0 = fma(stf, Hm[0], p0)
                        p1 = fma(stf, Hm[3], p1)
                        p2 = fma(stf, Hm[6], p2)
                sv = sv * F(1.0 / 255.0)
                srv = srv * F(1.0 / 255.0)
                svv = svv * F(1.0 / 65025.0)
                cov = srv - sr * sv * INV
                vs = svv - sv * sv * INV
                den = vr * vs
                ncc = np.where(den > F(1e-12), cov * (F(1.0) / np.sqrt(den)), F(0.0)).astype(np.float32)
                c = np.where(ok, F(1.0) - ncc, INF).astype(np.float32)
                # xsorted_insert for the pixels whose source is valid
                for j in range(6):
                    lo, hi = np.minimum(costs[j], c), np.maximum(costs[j], c)
                    costs[j] = np.where(ok, lo, costs[j])
                    c = np.where(ok, hi, c)
                n_valid += ok
        keep = np.maximum((n_valid + 1) // 2, 2)
        tot = np.zeros(P, np.float32)
        with np.errstate(all="ignore"):
            for j in range(6):
                tot = tot + np.where(j < keep, costs[j], F(0.0)).astype(np.float32)
            res = tot / keep.astype(np.float32)
        good = live & (n_valid >= 2)
        out[good] = res[good]
        return out

    def cost_map(self, depth, normal):
        """Cost of every pixel's plane (amvs_xpm_step, AMVS_XPM_PHASE_EVAL)."""
        n = normal.reshape(-1, 3)
        return self.cost(self.xs, self.ys, depth.ravel().astype(np.float32), n[:, 0].copy(), n[:, 1].copy(),
                         n[:, 2].copy()).reshape(self.H, self.W)

    # ---------------------------------------------------------- view propagation --
    def view_candidates(self, depth_all, normal_all, s_index, depth_min, depth_max):
        """xpm_view_candidates_kernel for source index s_index: (cand_depth (H, W) with 0 = none, cand_normal)."""
        H, W = self.H, self.W
        M, b = self.Mb[s_index]
        sv = self.srcs[s_index]
        Rr, tr = self.poses[self.ref]
        Rs, ts = self.poses[sv]
        k = self.Ki
        x, y = self.xs, self.ys
        fx, fy = x.astype(np.float32), y.astype(np.float32)
        d = depth_all[self.ref].ravel()
        q0 = fma(M[1], fy, fma(M[0], fx, M[2]))
        q1 = fma(M[4], fy, fma(M[3], fx, M[5]))
        q2 = fma(M[7], fy, fma(M[6], fx, M[8]))
        p2 = fma(d, q2, b[2])
        cd = np.zeros(H * W, np.float32)
        cn = np.tile(np.array([0, 0, -1], np.float32), (H * W, 1))
        with np.errstate(all="ignore"):
            front = p2 > F(0.1)
            px = np.rint(fma(d, q0, b[0]) / p2)
            py = np.rint(fma(d, q1, b[1]) / p2)
            inb = front & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            pxi = np.where(inb, px, 0).astype(np.int64)
            pyi = np.where(inb, py, 0).astype(np.int64)
            d2 = depth_all[sv][pyi, pxi]
            n0, n1, n2 = (normal_all[sv][pyi, pxi, c] for c in range(3))
            pxf, pyf = pxi.astype(np.float32), pyi.astype(np.float32)
            r0 = fma(k[1], pyf, fma(k[0], pxf, k[2]))
            r1 = fma(k[4], pyf, fma(k[3], pxf, k[5]))
            dl = d2 * (n0 * r0 + n1 * r1 + n2)
            nw = [Rs[c] * n0 + Rs[3 + c] * n1 + Rs[6 + c] * n2 for c in range(3)]
            dw = dl - (n0 * ts[0] + n1 * ts[1] + n2 * ts[2])
            nr = [Rr[3 * c] * nw[0] + Rr[3 * c + 1] * nw[1] + Rr[3 * c + 2] * nw[2] for c in range(3)]
            drf = dw + (nr[0] * tr[0] + nr[1] * tr[1] + nr[2] * tr[2])
            rpx = fma(k[1], fy, fma(k[0], fx, k[2]))
            rpy = fma(k[4], fy, fma(k[3], fx, k[5]))
            ndr = nr[0] * rpx + nr[1] * rpy + nr[2]
            t = drf / ndr
            okc = inb & (ndr < F(-1e-6)) & (t >= F(depth_min)) & (t <= F(depth_max))
            fnx, fny, fnz = normalise_facing(nr[0], nr[1], nr[2])
        cd[okc] = t[okc]
        cn[okc, 0], cn[okc, 1], cn[okc, 2] = fnx[okc], fny[okc], fnz[okc]
        return cd.reshape(H, W), cn.reshape(H, W, 3)

    # ---------------------------------------------------------------- half sweep --
    def half_sweep(self, depth, normal, cost, cand_d, cand_n, colour, iteration, seed, rng_fill, depth_min, depth_max,
                   num_refine=2, view_propagation=True):
        """xpm_sweep_kernel for one checkerboard colour, in place semantics: returns new (depth, normal, cost).
        rng_fill(seed, view, draw, n) -> (uniform (n,), normals (n, 3)) of the build's counter-hash generator."""
        H, W = self.H, self.W
        D, Nn, C = depth.copy(), normal.copy(), cost.copy()
        sel = ((self.xs + self.ys + colour) & 1) == 0               # x = 2 k + ((y + colour) & 1)
        x, y = self.xs[sel], self.ys[sel]
        idx = y * W + x
        bd = D.ravel()[idx].copy()
        bn = [Nn.reshape(-1, 3)[idx, c].copy() for c in range(3)]
        bc = C.ravel()[idx].copy()
        rpx, rpy = self._ray(x, y)
        shrink = 0.5 ** iteration
        rel_range, nrm_range = F(max(0.2 * shrink, 0.004)), F(max(0.4 * shrink, 0.01))
        with_random = iteration < 2
        draw = 1 + 2 * iteration + colour
        n_hyp = 6 + num_refine + (1 if with_random else 0)
        dmin, dmax = F(depth_min), F(depth_max)
        for hyp in range(n_hyp):
            d, nx, ny, nz = bd.copy(), bn[0].copy(), bn[1].copy(), bn[2].copy()
            have = np.ones(x.shape[0], bool)
            with np.errstate(all="ignore"):
                if hyp == 0:
                    have = ~(bc < INF)
                elif hyp <= 4:
                    k = hyp - 1
                    xx = x + (-1 if k == 0 else (1 if k == 1 else 0))
                    yy = y + (-1 if k == 2 else (1 if k == 3 else 0))
                    have = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                    j = np.where(have, yy * W + xx, 0)
                    nd = depth.ravel()[j]
                    nx, ny, nz = (normal.reshape(-1, 3)[j, c] for c in range(3))
                    rqx, rqy = self._ray(np.where(have, xx, 0), np.where(have, yy, 0))
                    dl = nd * (nx * rqx + ny * rqy + nz)
                    ndr = nx * rpx + ny * rpy + nz
                    have = have & (ndr < F(-1e-6))
                    d = dl / ndr
                elif hyp == 5:
                    have = np.full(x.shape[0], bool(view_propagation))
                    d = cand_d.ravel()[idx]
                    have = have & (d > 0)
                    nx, ny, nz = (cand_n.reshape(-1, 3)[idx, c] for c in range(3))
                elif hyp < 6 + num_refine:
                    r = hyp - 6
                    u, g = rng_fill(seed, self.ref, draw * 8 + r, H * W)
                    u, g = u[idx], g[idx]
                    scale = F(1.0 if r == 0 else 0.25)
                    d = bd * (F(1.0) + (u * F(2.0) - F(1.0)) * rel_range * scale)
                    nx = bn[0] + g[:, 0] * nrm_range * scale
                    ny = bn[1] + g[:, 1] * nrm_range * scale
                    nz = bn[2] + g[:, 2] * nrm_range * scale
                    nx, ny, nz = normalise_facing(nx, ny, nz)
                else:
                    u, g = rng_fill(seed, self.ref, draw * 8 + 7, H * W)
                    u, g = u[idx], g[idx]
                    lmin, lmax = np.log(dmin), np.log(dmax)
                    nx, ny, nz = normalise_facing(g[:, 0] * F(0.3), g[:, 1] * F(0.3), np.full(x.shape[0], F(-1.0)))
                    d = np.exp(lmin + u * (lmax - lmin)).astype(np.float32)
                if hyp > 0:
                    have = have & (d >= dmin) & (d <= dmax)
            d = d.astype(np.float32)
            c = self.cost(x, y, np.where(have, d, F(1.0)).astype(np.float32), np.asarray(nx, np.float32),
                          np.asarray(ny, np.float32), np.asarray(nz, np.float32))
            take = have & ((hyp == 0) | (c < bc))
            bc = np.where(take, c, bc).astype(np.float32)
            bd = np.where(take, d, bd).astype(np.float32)
            bn = [np.where(take, v, o).astype(np.float32) for v, o in zip((nx, ny, nz), bn)]
        D.ravel()[idx] = bd
        for c3 in range(3):
            Nn.reshape(-1, 3)[idx, c3] = bn[c3]
        C.ravel()[idx] = bc
        return D, Nn, C


# =====================================================================================================
# float64 reference with decision margins (tests/test_extended_paths.py)
#
# Written from the specification (the kernel header, DESIGN.md section 7 "Extended mode"), not from the
# kernels' operation order: float64 throughout, IEEE division / sqrt, NumPy exp / log.  Its inputs are the
# job table's float32 values (K, K^-1, poses, the composed M, b of `compose`) and the float32 state maps.
#
# Every kernel decision is a float comparison against a threshold; where the exact value lies close to
# the threshold the kernel's float32 rounding may decide the other way.  Each function therefore also
# returns a DECISION MARGIN per pixel: the distance of the closest decision from its threshold, in pixels
# for the u / v bounds of the footprint (and the rint of the consistency projection), relative (to the
# unit normal or to the threshold) for the depth tests, n.r < -1e-6 and the normal's facing test.  A
# decision that holds is limited by its smallest margin; a test that fails is limited by the LARGEST
# margin among the failing tests (one clear failure decides it).
#
# The window.  The taps run -half, -half + stride, ... and stop at or before +half on both axes (the
# generic loop `xcost`); for the (patch, stride) pairs the product uses, (patch - 1) is a multiple of
# stride and this is the centred N x N window of `xcost_t`.  For a pair that does not fit, e.g. (9, 3),
# the window is -4, -1, +2: NOT centred -- this is the specification (only C-ABI callers can ask for it).
# Every tap must pass every test (n.r_q < -1e-6 along its ray, source depth > 0.1, 0 <= u < W - 1,
# 0 <= v < H - 1); `taps="corners"` tests the four window corners only (what the N x N path does --
# equivalent in exact arithmetic because each test is affine or projective in the tap position).
# =====================================================================================================
D = np.float64
EPS32 = 2.0 ** -24


def _and_margin(oks, ms):
    """Conjunction of tests over the last axis: ok = all; margin = min of all margins if ok, else the largest
    margin among the failing tests."""
    ok = oks.all(axis=-1)
    m_ok = ms.min(axis=-1)
    m_fail = np.where(~oks, ms, -np.inf).max(axis=-1)
    return ok, np.where(ok, m_ok, m_fail)


def _rel(a, thr):
    return np.abs(a - thr) / abs(thr)


def normalise_facing64(nx, ny, nz):
    """xnormalise_facing in float64: (nx, ny, nz, margin of the facing test nz < -0.05, relative to 0.05)."""
    nx, ny, nz = (np.asarray(v, D) for v in (nx, ny, nz))
    l = np.sqrt(nx * nx + ny * ny + nz * nz)
    with np.errstate(divide="ignore", invalid="ignore"):
        il = np.where(l > 1e-12, 1.0 / l, 0.0)
    nx, ny, nz = nx * il, ny * il, nz * il
    m = _rel(nz, -0.05)
    bad = ~(nz < -0.05)
    return np.where(bad, 0.0, nx), np.where(bad, 0.0, ny), np.where(bad, -1.0, nz), m


def init_state(seed, view, H, W, log_scale, log_min, rng_fill):
    """xpm_init_kernel: depth = exp(u * log_scale + log_min) (log-uniform over [depth_min, depth_max]),
    normal = normalise_facing(0.3 g0, 0.3 g1, -1), cost = +inf, from draw 0 of the view's stream."""
    u, g = rng_fill(seed, view, 0, H * W)
    d = np.exp(u.astype(D) * D(np.float32(log_scale)) + D(np.float32(log_min)))
    nx, ny, nz, _ = normalise_facing64(g[:, 0].astype(D) * 0.3, g[:, 1].astype(D) * 0.3, np.full(H * W, -1.0))
    return d.reshape(H, W), np.stack([nx, ny, nz], -1).reshape(H, W, 3)


class Ref64:
    """One reference view with its sources, float64.  grays: list of (H, W) float images of all views (the
    float maps; 8-bit views are code / 255, for which the packed 8-bit sampling is exact)."""

    def __init__(self, K, K_inv, grays, poses, ref, srcs, patch, stride, taps="all"):
        self.Kf = np.asarray(K, np.float32).reshape(9)
        self.K = self.Kf.astype(D)
        self.Ki = np.asarray(K_inv, np.float32).reshape(9).astype(D)
        self.grays = [np.asarray(g, np.float32).astype(D) for g in grays]
        self.poses32 = [(np.asarray(R, np.float64).astype(np.float32).reshape(9), np.asarray(t, np.float64).astype(np.float32).reshape(3))
                        for R, t in poses]
        self.ref, self.srcs = int(ref), [int(s) for s in srcs]
        self.H, self.W = self.grays[0].shape
        self.patch, self.stride = int(patch), int(stride)
        half = self.patch // 2
        self.offs = np.arange(-half, half + 1, self.stride)
        assert taps in ("all", "corners")
        self.taps = taps
        Rr, tr = self.poses32[self.ref]
        self.Mb = [tuple(v.astype(D) for v in compose(self.Kf, Rr, tr, *self.poses32[s])) for s in self.srcs]
        ys, xs = np.meshgrid(np.arange(self.H), np.arange(self.W), indexing="ij")
        self.xs, self.ys = xs.ravel(), ys.ravel()

    def _ray(self, x, y):
        k = self.Ki
        return k[0] * x + k[1] * y + k[2], k[3] * x + k[4] * y + k[5]

    @staticmethod
    def _bilinear(img, u, v):
        H, W = img.shape
        with np.errstate(invalid="ignore"):
            x0 = np.clip(np.nan_to_num(np.floor(u), nan=0.0), 0, W - 2).astype(np.int64)
            y0 = np.clip(np.nan_to_num(np.floor(v), nan=0.0), 0, H - 2).astype(np.int64)
        fx, fy = u - x0, v - y0
        top = img[y0, x0] + fx * (img[y0, x0 + 1] - img[y0, x0])
        bot = img[y0 + 1, x0] + fx * (img[y0 + 1, x0 + 1] - img[y0 + 1, x0])
        return top + fy * (bot - top)

    # ---------------------------------------------------------------- cost -----
    def cost(self, x, y, d, nx, ny, nz, edge_tol=0.0):
        """Window cost of hypotheses (d[i], n[i]) at pixels (x[i], y[i]): (cost, margin, kappa).  kappa is the
        conditioning of the per-source NCC (max over the valid sources of sum r^2 / var r + sum v^2 / var v):
        a float32 evaluation of the sums loses about kappa * 2^-24 of the cost.  edge_tol > 0 widens the
        footprint bounds to -edge_tol <= u < W - 1 + edge_tol (same for v) -- the samples themselves stay
        exact (u = W - 1 reads column W - 1) -- to value windows whose validity is a rounding decision."""
        H, W, offs = self.H, self.W, self.offs
        x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
        d, nx, ny, nz = (np.asarray(v, D) for v in (d, nx, ny, nz))
        P = x.shape[0]
        cost = np.full(P, np.inf)
        margin = np.full(P, np.inf)
        kappa = np.zeros(P)
        win = (x + offs[0] >= 0) & (y + offs[0] >= 0) & (x + offs[-1] < W) & (y + offs[-1] < H)
        rpx, rpy = self._ray(x, y)
        ndr_p = nx * rpx + ny * rpy + nz
        idx = np.nonzero(win)[0]
        if idx.size == 0:
            return cost, margin, kappa
        oy, ox = (a.ravel() for a in np.meshgrid(offs, offs, indexing="ij"))
        if self.taps == "corners":
            n = offs.size
            sel = np.array([0, n - 1, n * (n - 1), n * n - 1])
            oy_t, ox_t = oy[sel], ox[sel]
        else:
            oy_t, ox_t = oy, ox
        xi, yi = x[idx], y[idx]
        dd, ax, ay, az = d[idx], nx[idx], ny[idx], nz[idx]
        ndp = ndr_p[idx]
        delta = dd * ndp

        def geom(oxs, oys):
            qx, qy = (xi[:, None] + oxs[None]).astype(D), (yi[:, None] + oys[None]).astype(D)
            rqx, rqy = self._ray(qx, qy)
            ndr = ax[:, None] * rqx + ay[:, None] * rqy + az[:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = delta[:, None] / ndr
            return qx, qy, ndr, t

        # the plane faces the camera at the pixel and along every tested ray (source independent)
        qxt, qyt, ndr_t, tt = geom(ox_t, oy_t)
        nd_all = np.concatenate([ndp[:, None], ndr_t], axis=1)
        face_ok, face_m = _and_margin(nd_all < -1e-6, np.abs(nd_all + 1e-6))
        qx, qy, _, t = geom(ox, oy)
        rv = self.grays[self.ref][yi[:, None] + oy[None], xi[:, None] + ox[None]]
        n_t = ox.size
        sr, srr = rv.sum(1), (rv * rv).sum(1)
        vr = srr - sr * sr / n_t
        src_cost, src_ok, src_m, src_k = [], [], [], []
        with np.errstate(all="ignore"):
            for s, (M, b) in zip(self.srcs, self.Mb):
                def project(qx_, qy_, t_):
                    X = [t_ * (M[3 * r] * qx_ + M[3 * r + 1] * qy_ + M[3 * r + 2]) + b[r] for r in range(3)]
                    return X[0] / X[2], X[1] / X[2], X[2]
                u, v, p2 = project(qxt, qyt, tt)
                e = edge_tol
                oks = np.concatenate([p2 > 0.1, u >= -e, u < W - 1 + e, v >= -e, v < H - 1 + e], axis=1)
                ms = np.concatenate([_rel(p2, 0.1), np.abs(u), np.abs(W - 1 - u), np.abs(v), np.abs(H - 1 - v)], axis=1)
                ms = np.where(np.isfinite(ms), ms, np.inf)
                ok, m = _and_margin(oks, ms)
                u, v, _ = project(qx, qy, t)
                sv = self._bilinear(self.grays[s], np.where(ok[:, None], u, 0.0), np.where(ok[:, None], v, 0.0))
                ssv, svv, srv = sv.sum(1), (sv * sv).sum(1), (rv * sv).sum(1)
                vs = svv - ssv * ssv / n_t
                cov = srv - sr * ssv / n_t
                den = vr * vs
                ncc = np.where(den > 1e-12, cov / np.sqrt(np.where(den > 0, den, 1.0)), 0.0)
                m = np.where(ok, np.minimum(m, _rel(den, 1e-12)), m)
                src_cost.append(np.where(ok, 1.0 - ncc, np.inf))
                src_ok.append(ok)
                src_m.append(m)
                src_k.append(np.where(ok & (den > 1e-12), srr / np.maximum(vr, 1e-300) + svv / np.maximum(vs, 1e-300), 0.0))
        sc = np.sort(np.stack(src_cost, 1), axis=1)
        n_valid = np.stack(src_ok, 1).sum(1)
        keep = np.maximum((n_valid + 1) // 2, 2)
        with np.errstate(invalid="ignore"):
            tot = np.where(np.arange(sc.shape[1])[None] < keep[:, None], sc, 0.0).sum(1)
            c = np.where(n_valid >= 2, tot / keep, np.inf)
        c = np.where(face_ok, c, np.inf)
        m = np.where(face_ok, np.minimum(face_m, np.stack(src_m, 1).min(1)), face_m)
        cost[idx], margin[idx], kappa[idx] = c, m, np.where(face_ok, np.stack(src_k, 1).max(1), 0.0)
        return cost, margin, kappa

    def cost_map(self, depth, normal, edge_tol=0.0):
        """(cost, margin, kappa) maps of every pixel's current plane (AMVS_XPM_PHASE_EVAL)."""
        n = np.asarray(normal).reshape(-1, 3)
        res = self.cost(self.xs, self.ys, np.asarray(depth).ravel(), n[:, 0], n[:, 1], n[:, 2], edge_tol)
        return tuple(r.reshape(self.H, self.W) for r in res)

    # ---------------------------------------------------------------- half sweep --
    def half_sweep(self, depth, normal, cost, cand_d, cand_n, colour, iteration, seed, rng_fill, depth_min, depth_max,
                   num_refine=2, view_propagation=True, cost_tol=None):
        """One red (colour 0) or black (colour 1) half sweep from the float32 state (depth, normal, cost) of
        this view and its view candidates.  Returns (depth, normal, cost, kappa, margin, gap): the new maps
        (the swept colour changed), the conditioning of the winning cost, the smallest margin of any decision
        taken for the pixel (hypothesis validity, range and facing tests, the validity of every cost
        evaluated) and the smallest cost gap of any comparison `c < best` with a finite side between two
        planes that differ by more than 5e-6 -- the gap between the winner and the runner-up when they met.  cost_tol(kappa): the error bound of a
        cost; when given, each gap is divided by the sum of the bounds of its two sides (decided if > 1)."""
        H, W = self.H, self.W
        Dm, Nm, Cm = (np.asarray(a).astype(D).copy() for a in (depth, normal, cost))
        sel = ((self.xs + self.ys + colour) & 1) == 0
        x, y = self.xs[sel], self.ys[sel]
        P = x.shape[0]
        idx = y * W + x
        bd = Dm.ravel()[idx].copy()
        bn = [Nm.reshape(-1, 3)[idx, c].copy() for c in range(3)]
        bc = Cm.ravel()[idx].copy()
        bk = self.cost(x, y, bd, *bn)[2]                  # conditioning of the current plane's cost
        margin = np.full(P, np.inf)
        gap = np.full(P, np.inf)
        rpx, rpy = self._ray(x.astype(D), y.astype(D))
        shrink = 0.5 ** iteration
        rel_range, nrm_range = D(np.float32(max(0.2 * shrink, 0.004))), D(np.float32(max(0.4 * shrink, 0.01)))
        with_random = iteration < 2
        draw = 1 + 2 * iteration + colour
        n_ref = max(0, min(6, num_refine))
        n_hyp = 6 + n_ref + (1 if with_random else 0)
        dmin, dmax = D(np.float32(depth_min)), D(np.float32(depth_max))
        d0, n0 = np.asarray(depth).astype(D), np.asarray(normal).astype(D).reshape(-1, 3)
        for hyp in range(n_hyp):
            d, nx, ny, nz = bd.copy(), bn[0].copy(), bn[1].copy(), bn[2].copy()
            have = np.ones(P, bool)
            hm = np.full(P, np.inf)
            with np.errstate(all="ignore"):
                if hyp == 0:
                    have = ~(bc < np.inf)
                elif hyp <= 4:
                    k = hyp - 1
                    xx = x + (-1 if k == 0 else (1 if k == 1 else 0))
                    yy = y + (-1 if k == 2 else (1 if k == 3 else 0))
                    have = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                    j = np.where(have, yy * W + xx, 0)
                    nx, ny, nz = (n0[j, c] for c in range(3))
                    rqx, rqy = self._ray(np.where(have, xx, 0).astype(D), np.where(have, yy, 0).astype(D))
                    dl = d0.ravel()[j] * (nx * rqx + ny * rqy + nz)
                    ndr = nx * rpx + ny * rpy + nz
                    hm = np.where(have, np.abs(ndr + 1e-6), np.inf)
                    have = have & (ndr < -1e-6)
                    d = dl / ndr
                elif hyp == 5:
                    d = np.asarray(cand_d).astype(D).ravel()[idx]
                    have = np.full(P, bool(view_propagation)) & (d > 0)
                    nx, ny, nz = (np.asarray(cand_n).astype(D).reshape(-1, 3)[idx, c] for c in range(3))
                elif hyp < 6 + n_ref:
                    r = hyp - 6
                    u, g = rng_fill(seed, self.ref, draw * 8 + r, H * W)
                    u, g = u[idx].astype(D), g[idx].astype(D)
                    scale = 1.0 if r == 0 else 0.25
                    d = bd * (1.0 + (u * 2.0 - 1.0) * rel_range * scale)
                    nx, ny, nz, hm = normalise_facing64(bn[0] + g[:, 0] * nrm_range * scale, bn[1] + g[:, 1] * nrm_range * scale,
                                                        bn[2] + g[:, 2] * nrm_range * scale)
                else:
                    u, g = rng_fill(seed, self.ref, draw * 8 + 7, H * W)
                    u, g = u[idx].astype(D), g[idx].astype(D)
                    nx, ny, nz, hm = normalise_facing64(g[:, 0] * 0.3, g[:, 1] * 0.3, np.full(P, -1.0))
                    lmin, lmax = np.log(dmin), np.log(dmax)
                    d = np.exp(lmin + u * (lmax - lmin))
                if hyp > 0:
                    hm = np.minimum(hm, np.where(have, np.minimum(_rel(d, dmin), _rel(d, dmax)), np.inf))
                    have = have & (d >= dmin) & (d <= dmax)
            c, cm, ck = self.cost(x, y, np.where(have, d, 1.0), np.where(have, nx, 0.0), np.where(have, ny, 0.0),
                                  np.where(have, nz, -1.0))
            margin = np.minimum(margin, hm)
            margin = np.where(have, np.minimum(margin, cm), margin)
            if hyp > 0:
                with np.errstate(invalid="ignore"):
                    # a near-tie between two planes that agree to 5e-6 decides nothing
                    differ = (np.abs(d - bd) > 5e-6 * np.abs(bd)) | (np.abs(nx - bn[0]) > 5e-6) | (np.abs(ny - bn[1]) > 5e-6) \
                        | (np.abs(nz - bn[2]) > 5e-6)
                    g_ = np.where(have & differ & (np.isfinite(c) | np.isfinite(bc)), np.abs(c - bc), np.inf)
                    if cost_tol is not None:
                        g_ = g_ / (cost_tol(ck) + cost_tol(bk))
                gap = np.minimum(gap, np.where(np.isnan(g_), np.inf, g_))
            take = have & ((hyp == 0) | (c < bc))
            bc = np.where(take, c, bc)
            bd = np.where(take, d, bd)
            bk = np.where(take, ck, bk)
            bn = [np.where(take, v, o) for v, o in zip((nx, ny, nz), bn)]
        out_k, out_m, out_g = np.zeros(H * W), np.full(H * W, np.inf), np.full(H * W, np.inf)
        Dm.ravel()[idx] = bd
        for c3 in range(3):
            Nm.reshape(-1, 3)[idx, c3] = bn[c3]
        Cm.ravel()[idx] = bc
        out_k[idx], out_m[idx], out_g[idx] = bk, margin, gap
        return Dm, Nm, Cm, out_k.reshape(H, W), out_m.reshape(H, W), out_g.reshape(H, W)

    # ---------------------------------------------------------------- consistency --
    def consistency(self, depth_all, cost_ref, consistency_px=1.0, consistency_rel=0.01):
        """xpm_consistency_kernel: per pixel of the reference view whose cost is below 0.6, the number of
        sources in which its point (depth d) lands in front of the source (depth > 0.1), on a pixel (rounded
        to the nearest) inside the image whose own depth d2 lifts to a point that, seen from the reference,
        is in front of it (> 0.1), re-projects within consistency_px of the pixel and has a depth within
        consistency_rel * d of d.  Returns (count, margin): the margin is in pixels for the rounding and the
        re-projection error, relative for the depth tests (to 0.1 and to consistency_rel * d)."""
        H, W = self.H, self.W
        K, Ki = self.K, self.Ki
        Rr, tr = (v.astype(D) for v in self.poses32[self.ref])
        x, y = self.xs.astype(D), self.ys.astype(D)
        d = np.asarray(depth_all[self.ref], np.float32).astype(D).ravel()
        live = np.asarray(cost_ref, np.float32).ravel() < np.float32(0.6)
        cnt = np.zeros(H * W, np.int64)
        margin = np.full(H * W, np.inf)
        rx, ry = self._ray(x, y)
        with np.errstate(all="ignore"):
            for s, (M, b) in zip(self.srcs, self.Mb):
                Rs, ts = (v.astype(D) for v in self.poses32[s])
                X = [d * (M[3 * r] * x + M[3 * r + 1] * y + M[3 * r + 2]) + b[r] for r in range(3)]
                p2 = X[2]
                u, v = X[0] / p2, X[1] / p2
                px, py = np.rint(u), np.rint(v)
                m_round = np.minimum(np.abs(np.abs(u - np.floor(u)) - 0.5), np.abs(np.abs(v - np.floor(v)) - 0.5))
                inb = (p2 > 0.1) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
                # the decisions up to here: in front of the source (margin relative), the rounding (pixels)
                m1 = np.where(p2 > 0.1, np.minimum(_rel(p2, 0.1), m_round), _rel(p2, 0.1))
                pxi, pyi = np.where(inb, px, 0).astype(np.int64), np.where(inb, py, 0).astype(np.int64)
                d2 = np.asarray(depth_all[s], np.float32).astype(D)[pyi, pxi]
                Y = np.stack([(Ki[0] * pxi + Ki[1] * pyi + Ki[2]) * d2, (Ki[3] * pxi + Ki[4] * pyi + Ki[5]) * d2, d2])
                Xw = Rs.reshape(3, 3).T @ (Y - ts[:, None])
                Xr = Rr.reshape(3, 3) @ Xw + tr[:, None]
                uu = (K[0] * Xr[0] + K[1] * Xr[1]) / Xr[2] + K[2]
                vv = (K[3] * Xr[0] + K[4] * Xr[1]) / Xr[2] + K[5]
                e = np.sqrt((uu - x) ** 2 + (vv - y) ** 2)
                rel_err = np.abs(Xr[2] - d) / d
                tests = np.stack([Xr[2] > 0.1, e < consistency_px, rel_err < consistency_rel], 1)
                ms = np.stack([_rel(Xr[2], 0.1), np.abs(e - consistency_px), _rel(rel_err, consistency_rel)], 1)
                ms = np.where(np.isfinite(ms), ms, np.inf)
                ok2, m2 = _and_margin(tests, ms)
                agree = live & inb & ok2
                cnt += agree
                m = np.where(inb, np.minimum(m1, m2), m1)
                margin = np.where(live, np.minimum(margin, m), margin)
        return cnt.reshape(H, W), margin.reshape(H, W)

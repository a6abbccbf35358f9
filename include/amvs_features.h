/* amvs_features.h -- the SIFT feature extractor of libamvs.so (csrc/amvs_clahe.hip, csrc/amvs_sift.hip,
 * csrc/amvs_sift_keypoints.hip, csrc/amvs_capi_features.hip): CLAHE on a gray 8-bit image, the Gaussian /
 * difference-of-Gaussian scale space of Lowe's SIFT (IJCV 2004), resident on the device and fetched level by level, and
 * on it the keypoints (extrema, refinement, contrast and edge tests), their orientations, their 128-byte descriptors,
 * a canonical order and the selection of the strongest.
 *
 * Why a header of its own: existing tests hold every other header to its table of _lib.py, and existing tests do not
 * change.  What is declared here is bound from an eleventh table, _lib.FEATURE_SIGNATURES; _lib.load() binds all of them.
 * The library, the context and the error codes are those of amvs.h.
 *
 * ---- the definition -----------------------------------------------------------------------------------------------------
 * The structure and the parameters are those OpenCV's createCLAHE and SIFT_create expose.  OpenCV is not a dependency of
 * this library, so the text below IS the definition; parity with cv2 itself is UNPINNED, as it is
 * for the image preparation and the RANSACs.  The device is judged against tests/features_restatement.py, written from
 * this text, bit for bit.
 *
 * Arithmetic.  Integer stages are exact.  Where the text says float32, every operation is one float32 operation with one
 * rounding (to nearest, ties to even), nothing is contracted, and the order is the written one; a * b + c is a product and
 * a sum, two roundings.  Where it says float64, the same holds in float64.
 * Division and sqrt are correctly rounded.  rint rounds to the nearest integer, halves to even.  (int)v truncates.
 * Nothing on the device depends on a library's exp, log, pow, atan2, sin or cos: the Gaussian taps are made on the host
 * (below), and the keypoint stages use the float32 functions expf, atan2deg and sincosdeg stated below
 * (csrc/amvs_sift_math.h).  No fused operation occurs anywhere in this text.
 *
 * fold(i, n), the reflect-101 border folded as often as needed, for any integer i and n >= 1:
 *     n == 1: 0.       Else p = 2 * (n - 1), m = i mod p taken into 0 .. p - 1, and fold = m < n ? m : p - m.
 * (fold(-1, n) = 1, fold(n, n) = n - 2; for n = 3: ... 2 1 | 0 1 2 | 1 0 | 1 2 ...)
 *
 * ---- CLAHE: amvs_clahe_u8 --------------------------------------------------------------------------------------------
 * Input gray [h][w] uint8, clip_limit (float32), grid_x and grid_y tiles across and down.
 *  1. Padding.  Wp = ceil(w / grid_x) * grid_x, Hp = ceil(h / grid_y) * grid_y.  The padded image is
 *     P[y][x] = gray[fold(y, h)][fold(x, w)] for 0 <= y < Hp, 0 <= x < Wp (nothing is added where the side divides).
 *     tw = Wp / grid_x, th = Hp / grid_y, area = tw * th.
 *  2. Histograms.  Tile (ty, tx) covers rows ty * th .. ty * th + th - 1 and columns tx * tw .. tx * tw + tw - 1 of P;
 *     hist[v] = the number of its pixels of value v, v = 0 .. 255.
 *  3. Clip limit.  clip_limit == 0 switches the clipping off.  Else t = (clip_limit * (float)area) / 256.0f in float32;
 *     if t >= (float)area the clipping is off too (no bin can exceed it), else limit = max(1, (int)t).
 *  4. Clipping and redistribution, per tile, when the clipping is on:
 *         excess = sum over v of max(0, hist[v] - limit);      hist[v] = min(hist[v], limit)
 *         batch = excess / 256 (integer division);  residual = excess - 256 * batch;  hist[v] += batch for every v
 *         if residual > 0: step = max(256 / residual, 1) (integer division), and hist[k * step] += 1 for
 *         k = 0 .. residual - 1   (k * step < 256 always holds).
 *  5. LUT.  scale = 255.0f / (float)area (float32 division).  With c[v] = hist[0] + .. + hist[v] (exact integers),
 *         lut[v] = min(255, (int)rint((float)c[v] * scale))       ((float)c[v] rounds to nearest even above 2^24)
 *  6. Interpolation.  For the output pixel at row y < h and column x < w with value v = gray[y][x], in float32:
 *         fy = (float)y * (1.0f / (float)th) - 0.5f;   y1 = floor(fy);   ya = fy - (float)y1;   ya1 = 1.0f - ya
 *         fx = (float)x * (1.0f / (float)tw) - 0.5f;   x1 = floor(fx);   xa = fx - (float)x1;   xa1 = 1.0f - xa
 *         y2 = min(y1 + 1, grid_y - 1);  y1 = max(y1, 0);      x2 = min(x1 + 1, grid_x - 1);  x1 = max(x1, 0)
 *         (ya, ya1, xa, xa1 are taken before the clamps)
 *         r = ((float)lut[y1][x1][v] * xa1 + (float)lut[y1][x2][v] * xa) * ya1
 *           + ((float)lut[y2][x1][v] * xa1 + (float)lut[y2][x2][v] * xa) * ya
 *         out[y][x] = min(255, max(0, (int)rint(r)))
 *     where lut[ty][tx] is the LUT of tile (ty, tx).
 * The result is returned (out_host, which may be NULL) and stays RESIDENT in the context with its size, for
 * amvs_sift_scale_space, until the next amvs_clahe_u8.
 *
 * ---- scale space: amvs_sift_scale_space --------------------------------------------------------------------------------
 * Input gray [h][w] uint8 and sigma (float64; SIFT_create's default is 1.6).  n_layers = 3 intervals per octave,
 * AMVS_SIFT_GAUSS = n_layers + 3 = 6 Gaussian images and AMVS_SIFT_DOG = 5 difference images per octave.
 *
 * Octave count.  m = min(h, w), L = floor(log2(m * m)) (the position of the highest set bit of the integer m * m),
 *     n_octaves = floor((L - 3) / 2) + 1.
 * This is rint(log2(m) - 2) + 1, OpenCV's count with the doubled first octave, without a logarithm: 24 gives 4, 45 gives
 * 4, 46 gives 5, 64 gives 5.  m >= AMVS_SIFT_MIN_SIDE = 3 makes it at least 1, and the last octave at least 5 pixels wide.
 *
 * Octave 0 is twice the input's size (Lowe's octave -1): H0 = 2 h, W0 = 2 w.  Octave o + 1 has Ho+1 = floor(Ho / 2) rows
 * and Wo+1 = floor(Wo / 2) columns.
 *
 * Upsampling.  g[y][x] = (float)gray[y][x].  For a destination index d = 2 k or 2 k + 1 along an axis of source length
 * n, near(d) = k, and far(d) = max(k - 1, 0) for even d, min(k + 1, n - 1) for odd d.  In float32:
 *     row(yy, x) = 0.75f * g[yy][near(x)] + 0.25f * g[yy][far(x)]
 *     U[y][x]    = 0.75f * row(near(y), x) + 0.25f * row(far(y), x)
 * (the linear resize to the doubled size with sample centres at (d + 0.5) / 2 - 0.5 and a replicated border).
 *
 * Sigmas, on the host in float64.  K3 = 1.2599210498948732 (the float64 nearest to 2^(1/3)).
 *     s_base = sqrt(max(sigma * sigma - 1.0, 0.01))             (the doubled input is taken to have blur 2 * 0.5 = 1)
 *     prev_1 = sigma;  for i = 1 .. 5:  total = prev_i * K3;  s_i = sqrt(total * total - prev_i * prev_i);
 *     prev_(i+1) = total
 *
 * Taps of a blur of sigma s, on the host in float64.  n_taps = ((int)rint(8.0 * s + 1.0)) | 1, radius r = n_taps / 2
 * (integer division); r <= AMVS_SIFT_MAX_RADIUS = 32 is guaranteed by sigma <= AMVS_SIFT_MAX_SIGMA = 4.
 *     d = 2.0 * s * s;     e_j = exp64(-((double)((j - r) * (j - r))) / d) for j = 0 .. 2 r
 *     total = e_0 + e_1 + .. + e_2r  (a serial sum from j = 0 upwards);     tap[j] = (float)(e_j / total)
 * exp64(x) for x <= 0, in float64 (no library's exp is called, so the host and the restatement agree to the bit):
 *     n = rint(x * 1.4426950408889634);
 *     t = (x - n * 0.693147180369123816490) - n * 1.90821492927058770002e-10
 *     q = 1/13!;  then for k = 12 down to 0:  q = q * t + 1/k!        (1/k! = 1.0 divided by the exact integer k!)
 *     exp64 = ldexp(q, (int)n)                 (x >= -745 * 0.69 here always: (2 r)^2 / (2 s^2) <= 40)
 *
 * Blur of an image I [H][W] with taps of radius r, in float32, two passes, each pixel one serial sum in tap order:
 *     T[y][x] = sum over j = 0 .. 2 r of tap[j] * I[y][fold(x - r + j, W)]
 *     B[y][x] = sum over j = 0 .. 2 r of tap[j] * T[fold(y - r + j, H)][x]
 * where "sum" is acc = tap[0] * v_0, then acc = acc + tap[j] * v_j for j = 1, 2, ... .  The radius may exceed the side
 * (the smallest octaves): fold then reflects more than once.
 *
 * Per octave.  G[0][0] = blur of U by s_base.  G[o][i] = blur of G[o][i - 1] by s_i, i = 1 .. 5.
 *     D[o][i] = G[o][i + 1] - G[o][i], i = 0 .. 4 (float32).
 *     G[o + 1][0][y][x] = G[o][3][2 y][2 x]                      (3 = n_layers: the image with twice the octave's sigma)
 * The scale space stays RESIDENT in the context until the next amvs_sift_scale_space.
 *
 * ---- keypoints: amvs_sift_extract ---------------------------------------------------------------------------------------
 * Parameters: n_features (0: all), contrast_threshold ct and edge_threshold (float32; SIFT_create's defaults 0.04, 10)
 * and sigma, of which the keypoint stages use sf = (float)sigma.  Everything below is float32 unless it says otherwise.
 *
 * The float32 functions (Horner steps q = q * t + c, a product and a sum each; a / b written as a constant is the
 * float32 quotient of the two float32 numbers):
 *   expf(x), -80 <= x <= 80 (x < -80 gives 0):  n = rint(x * 1.44269504f);
 *       t = (x - n * 0.693359375f) - n * (-2.12194440e-4f);
 *       q = 1/720; then q = q * t + c for c = 1/120, 1/24, 1/6, 1/2, 1, 1;     expf = q * 2^n (exact).
 *   atan2deg(y, x), degrees in 0 .. 360:  ax = |x|, ay = |y|, mx = max(ax, ay), mn = min(ax, ay); mx == 0 gives 0.  Else
 *       a = mn / mx;  s = a * a;  p = -0.01172120f; then p = p * s + c for c = 0.05265332f, -0.11643287f, 0.19354346f,
 *       -0.33262347f, 0.99997726f;  r = (p * a) * 57.29578f;  if ay > ax: r = 90 - r;  then if x < 0: r = 180 - r;  then
 *       if y < 0: r = 360 - r.
 *   sinp(t): s = t * t;  p = -1/39916800; then p = p * s + c for c = 1/362880, -1/5040, 1/120, -1/6, 1;  sinp = p * t.
 *   sincosdeg(a), 0 <= a < 360:  q = min((int)(a * (1/90)), 3);  rr = (a - 90 * (float)q) * 0.017453292f;
 *       s = sinp(rr), c = sinp(1.5707964f - rr);  (sin, cos) = (s, c), (c, -s), (-s, -c), (-c, s) for q = 0, 1, 2, 3.
 *
 * Candidates.  pre = (float)floor(0.5 * (double)ct / 3.0 * 255.0) (float64 on the host).  In every octave with H > 10 and
 * W > 10, for i = 1, 2, 3 and 5 <= r < H - 5, 5 <= c < W - 5, with v = D[o][i][r][c] and its 26 neighbours in D[o][i - 1],
 * D[o][i], D[o][i + 1] at rows r - 1 .. r + 1 and columns c - 1 .. c + 1: (o, i, r, c) is a candidate when v > pre and
 * v >= every neighbour, or v < -pre and v <= every neighbour.
 *
 * Refinement of a candidate, at most 5 steps from (i, r, c); P = D[o][i - 1], Q = D[o][i], N = D[o][i + 1]:
 *     is = 1/255;  ds = is * 0.5f;  cs = is * 0.25f;   v2 = Q[r][c] * 2
 *     gx = (Q[r][c+1] - Q[r][c-1]) * ds;  gy = (Q[r+1][c] - Q[r-1][c]) * ds;  gs = (N[r][c] - P[r][c]) * ds
 *     dxx = (Q[r][c+1] + Q[r][c-1] - v2) * is;  dyy = (Q[r+1][c] + Q[r-1][c] - v2) * is;  dss = (N[r][c] + P[r][c] - v2) * is
 *     dxy = (Q[r+1][c+1] - Q[r+1][c-1] - Q[r-1][c+1] + Q[r-1][c-1]) * cs
 *     dxs = (N[r][c+1] - N[r][c-1] - P[r][c+1] + P[r][c-1]) * cs;  dys = (N[r+1][c] - N[r-1][c] - P[r+1][c] + P[r-1][c]) * cs
 * (sums left to right).  The 3 x 3 system is solved by its cofactors, in this order:
 *     c00 = dyy * dss - dys * dys;  c01 = dxs * dys - dxy * dss;  c02 = dxy * dys - dxs * dyy
 *     det = dxx * c00 + dxy * c01 + dxs * c02;       det == 0 rejects the candidate
 *     c11 = dxx * dss - dxs * dxs;  c12 = dxy * dxs - dxx * dys;  c22 = dxx * dyy - dxy * dxy
 *     xc = -((c00 * gx + c01 * gy + c02 * gs) / det);  xr = -((c01 * gx + c11 * gy + c12 * gs) / det)
 *     xi = -((c02 * gx + c12 * gy + c22 * gs) / det)
 * Unless |xc|, |xr| and |xi| are all <= 1e6 (a NaN is not), the candidate is rejected.  If all three are < 0.5 the
 * refinement has converged.  Else c += (int)rint(xc), r += (int)rint(xr), i += (int)rint(xi); the candidate is rejected
 * if then i < 1, i > 3, c < 5, c >= W - 5, r < 5 or r >= H - 5; otherwise the next step.  Five steps without convergence
 * reject it.  With the values of the converged step:
 *     t = gx * xc + gy * xr + gs * xi;   contr = Q[r][c] * is + t * 0.5f;        rejected if |contr| * 3 < ct
 *     tr = dxx + dyy;  d2 = dxx * dyy - dxy * dxy;     rejected if d2 <= 0 or tr * tr * edge >= (edge + 1) * (edge + 1) * d2
 *     scl = sf * expf((((float)i + xi) * (1/3)) * 0.6931472f)           (the scale in the octave's own pixels)
 *     x = ((float)c + xc) * (2^o * 0.5f);  y = ((float)r + xr) * (2^o * 0.5f);  size = scl * 2^o;  response = |contr|
 * (octave 0 is the doubled image, hence the 0.5).  packed = (float)(o + 256 * i), o this header's octave index.
 *
 * Orientations of a refined keypoint, on I = G[o][i] at the integer (r, c) where the refinement ended:
 *     radius = (int)rint(4.5f * scl);  sp = 1.5f * scl;  es = -1 / ((2 * sp) * sp)
 *     for di, dj in -radius .. radius with y = r + di, x = c + dj and 0 < y < H - 1, 0 < x < W - 1:
 *         dx = I[y][x+1] - I[y][x-1];  dy = I[y-1][x] - I[y+1][x];  ori = atan2deg(dy, dx);  mag = sqrt(dx * dx + dy * dy)
 *         wgt = expf((float)(di * di + dj * dj) * es);   b = (int)rint(ori * 0.1f), 36 taken off if b >= 36
 *         Hq[b] += (int64)rint((wgt * mag) * 1048576.0f)
 * The histogram is 64-bit integers at the fixed point 2^-20: a contribution is rounded once and integer sums have no
 * order.  (mag < 361, wgt <= 1, at most 83^2 samples: below 2^42.)  Then h[b] = (float)Hq[b] * (1/1048576), and with
 * indices taken modulo 36
 *     sm[b] = (h[b-2] + h[b+2]) * 0.0625f + (h[b-1] + h[b+1]) * 0.25f + h[b] * 0.375f
 * Every b with sm[b] > sm[b-1], sm[b] > sm[b+1] and sm[b] >= 0.8f * max(sm) gives one keypoint:
 *     bf = (float)b + (0.5f * (sm[b-1] - sm[b+1])) / ((sm[b-1] - 2 * sm[b]) + sm[b+1]);   + 36 if bf < 0, then - 36 if bf >= 36
 *     angle = 360 - 10 * bf;   0 if |angle - 360| < 1.1920929e-07f
 *
 * Descriptor of a keypoint, on the same I, (r, c) and scl:
 *     a = 360 - angle, 0 if |a - 360| < 1.1920929e-07f;   (sn, cs) = sincosdeg(a);   hw = 3 * scl
 *     radius = min((int)rint(hw * 1.4142135f * 2.5f), H + W);   cs = cs / hw;  sn = sn / hw
 *     for di, dj in -radius .. radius, y = r + di, x = c + dj:
 *         crot = (float)dj * cs - (float)di * sn;  rrot = (float)dj * sn + (float)di * cs;  rbin = rrot + 1.5f;  cbin = crot + 1.5f
 *         used when -1 < rbin < 4, -1 < cbin < 4, 0 < y < H - 1 and 0 < x < W - 1;  dx, dy, ori, mag as above
 *         wgt = expf((crot * crot + rrot * rrot) * -0.125f);   obin = (ori - a) * 0.022222223f;   m = mag * wgt
 *         r0 = floor(rbin), c0 = floor(cbin), o0 = floor(obin);  fr = rbin - r0;  fc = cbin - c0;  fo = obin - o0
 *         v1 = m * fr;  v0 = m - v1;  v11 = v1 * fc;  v10 = v1 - v11;  v01 = v0 * fc;  v00 = v0 - v01
 *         for (dr, dc) in (0,0), (0,1), (1,0), (1,1) with 0 <= r0 + dr <= 3 and 0 <= c0 + dc <= 3:
 *             hi = v[dr][dc] * fo;  lo = v[dr][dc] - hi
 *             Hd[r0+dr][c0+dc][o0 mod 8] += (int64)rint(lo * 1048576.0f);  Hd[r0+dr][c0+dc][(o0 + 1) mod 8] += (int64)rint(hi * ...)
 * (64-bit integers again; at most 193^2 samples of at most 361: below 2^44).  With d[k] = (float)Hd[k] * (1/1048576),
 * k = (row * 4 + column) * 8 + bin, and n2(v) the serial sum acc = v[0] * v[0], acc = acc + v[k] * v[k], k = 1 .. 127:
 *     thr = sqrt(n2(d)) * 0.2f;   d[k] = min(d[k], thr);   scale = 512 / max(sqrt(n2(d)), 1.1920929e-07f)
 *     descriptor[k] = min(255, (int)rint(d[k] * scale))                     (what amvs_desc_set of amvs_match.h takes)
 *
 * Order and selection.  The canonical order is ascending (o, i, r, c, b) with (i, r, c) those of the CANDIDATE the
 * keypoint was refined from (unique) and b its histogram bin.  With n_features > 0 and more keypoints than that, the
 * n_features first under (response descending, canonical index ascending) are kept, so ties are decided.  The output is
 * in canonical order.  Nothing is truncated silently: more than AMVS_SIFT_MAX_FEATURES keypoints before the selection
 * is AMVS_EINVAL, and nothing is then resident.
 *
 * ---- entry points ------------------------------------------------------------------------------------------------------
 * A NULL context returns AMVS_EINVAL first.  Parameter errors are AMVS_EINVAL and are reported before anything is
 * allocated or launched: a NULL required pointer; h or w < 1 (CLAHE) or < AMVS_SIFT_MIN_SIDE (scale space) or
 * > AMVS_FEATURES_MAX_SIDE; grid_x or grid_y < 1 or > AMVS_CLAHE_MAX_GRID; clip_limit negative or not finite; sigma not
 * finite, < AMVS_SIFT_MIN_SIGMA (below it sigma * sigma loses its meaning long before it underflows) or
 * > AMVS_SIFT_MAX_SIGMA; n_features < 0 or > AMVS_SIFT_MAX_FEATURES; contrast_threshold negative or not finite;
 * edge_threshold not finite or <= 0; an octave, index, size, count or slot that does not exist.  All entry points
 * synchronise (amvs_sift_fetch_level without out_host, and amvs_sift_fetch of nothing, touch no device).
 *
 * amvs_clahe_u8: above.  gray_host [h][w]; out_host [h][w] or NULL.
 *
 * amvs_sift_scale_space: gray_host [h][w], or NULL for the resident result of amvs_clahe_u8, whose size h and w must then
 * be (none resident: AMVS_EINVAL).  *n_octaves receives the octave count.
 *
 * amvs_sift_extract: the scale space as amvs_sift_scale_space builds it (it stays resident too), then the keypoints.
 * *n_keypoints receives their number; rows and descriptors stay RESIDENT until the next amvs_sift_extract or
 * amvs_sift_scale_space.
 *
 * amvs_sift_fetch: n must be the resident count.  keypoints_out [n][6] float32: x, y, size, angle in degrees, response,
 * packed; descriptors_out [n][128] uint8; either may be NULL.
 *
 * amvs_sift_to_slot: the resident descriptors into descriptor slot `slot` of amvs_match.h, as amvs_desc_set of the
 * fetched bytes would, without a visit to the host.
 *
 * amvs_sift_fetch_level: Gaussian image (dog == 0, index 0 .. 5) or difference image (dog != 0, index 0 .. 4) of an
 * octave of the resident scale space.  *h_out and *w_out receive its size (either may be NULL); out_host may be NULL to
 * ask for the size alone, else it receives [h][w] float32.                                                              */
#ifndef AMVS_FEATURES_H
#define AMVS_FEATURES_H

#include "amvs.h"

#define AMVS_FEATURES_MAX_SIDE 8192
#define AMVS_CLAHE_MAX_GRID 64
#define AMVS_SIFT_MIN_SIDE 3
#define AMVS_SIFT_MIN_SIGMA 0.1
#define AMVS_SIFT_MAX_SIGMA 4.0
#define AMVS_SIFT_MAX_FEATURES 1048576
#define AMVS_SIFT_MAX_RADIUS 32
#define AMVS_SIFT_LAYERS 3
#define AMVS_SIFT_GAUSS 6
#define AMVS_SIFT_DOG 5

#ifdef __cplusplus
extern "C" {
#endif

int amvs_clahe_u8(amvs_ctx *ctx, const uint8_t *gray_host, int h, int w, float clip_limit, int grid_x, int grid_y,
                  uint8_t *out_host);

int amvs_sift_scale_space(amvs_ctx *ctx, const uint8_t *gray_host, int h, int w, double sigma, int *n_octaves);

int amvs_sift_extract(amvs_ctx *ctx, const uint8_t *gray_host, int h, int w, int n_features, float contrast_threshold,
                      float edge_threshold, double sigma, int *n_keypoints);

int amvs_sift_fetch(amvs_ctx *ctx, float *keypoints_out, uint8_t *descriptors_out, int n);

int amvs_sift_to_slot(amvs_ctx *ctx, int slot);

int amvs_sift_fetch_level(amvs_ctx *ctx, int octave, int index, int dog, float *out_host, int *h_out, int *w_out);

#ifdef __cplusplus
}
#endif

#endif

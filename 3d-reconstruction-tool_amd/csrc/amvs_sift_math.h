// amvs_sift_math.h -- the arithmetic the feature stages share (include/amvs_features.h states every line of it): the
// folded reflect-101 border, and, on the host in float64, the octave count, the per-layer sigmas and the Gaussian taps
// with their own exp, so that no result depends on a library's exp, log or pow; and, in float32 for the kernels, the
// exp, the angle of a gradient in degrees and the sine / cosine of the keypoint stages.  The kernels receive the taps as
// an argument.  -ffp-contract=off (Makefile) holds for the host code too: a * b + c below is two roundings.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace amvs {

constexpr int SIFT_MAX_RADIUS = 32;

// 2 r + 1 taps of a blur, by value in a kernel's argument block (scalar loads)
struct GaussTaps {
    int r;
    float w[2 * SIFT_MAX_RADIUS + 1];
};

// reflect-101, folded as often as needed: any i, n >= 1
__host__ __device__ __forceinline__ int fold101(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// ---- float32, for the orientation and descriptor kernels (the header's expf, atan2deg and sincosdeg) ----
// -80 <= x <= 80 (0 below): Cody-Waite reduction by ln 2, the Taylor polynomial of degree 6, the scale by 2^n exact
__device__ __forceinline__ float sift_expf(float x)
{
    const float n = rintf(x * 1.44269504f);
    const float t = (x - n * 0.693359375f) - n * -2.12194440e-4f;
    float q = 1.0f / 720.0f;
    q = q * t + 1.0f / 120.0f;
    q = q * t + 1.0f / 24.0f;
    q = q * t + 1.0f / 6.0f;
    q = q * t + 1.0f / 2.0f;
    q = q * t + 1.0f;
    q = q * t + 1.0f;
    const bool low = !(x >= -80.0f);
    const int e = low ? 0 : (int)n;
    return low ? 0.0f : q * __int_as_float((e + 127) << 23);
}

// the angle of (x, y) in degrees, 0 .. 360: an odd polynomial of the smaller over the larger, unfolded by octant
__device__ __forceinline__ float sift_atan2deg(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    if (mx == 0.0f) return 0.0f;
    const float a = mn / mx, s = a * a;
    float p = -0.01172120f;
    p = p * s + 0.05265332f;
    p = p * s + -0.11643287f;
    p = p * s + 0.19354346f;
    p = p * s + -0.33262347f;
    p = p * s + 0.99997726f;
    float r = (p * a) * 57.29578f;
    if (ay > ax) r = 90.0f - r;
    if (x < 0.0f) r = 180.0f - r;
    if (y < 0.0f) r = 360.0f - r;
    return r;
}

__device__ __forceinline__ float sift_sinp(float t)
{
    const float s = t * t;
    float p = -1.0f / 39916800.0f;
    p = p * s + 1.0f / 362880.0f;
    p = p * s + -1.0f / 5040.0f;
    p = p * s + 1.0f / 120.0f;
    p = p * s + -1.0f / 6.0f;
    p = p * s + 1.0f;
    return p * t;
}

// 0 <= a < 360 degrees: the quadrant, then the Taylor polynomial of the sine of degree 11 on 0 .. pi / 2
__device__ __forceinline__ void sift_sincosdeg(float a, float *sn, float *cs)
{
    int q = (int)(a * (1.0f / 90.0f));
    q = q < 3 ? q : 3;
    const float rr = (a - 90.0f * (float)q) * 0.017453292f;
    const float s = sift_sinp(rr), c = sift_sinp(1.5707964f - rr);
    *sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    *cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}

// exp(x) for x <= 0: n = rint(x / ln 2), Cody-Waite reduction, the Taylor polynomial of degree 13 by Horner
inline double sift_exp64(double x)
{
    const double n = std::rint(x * 1.4426950408889634);
    const double t = (x - n * 0.693147180369123816490) - n * 1.90821492927058770002e-10;
    double fact[14];
    fact[0] = 1.0;
    for (int k = 1; k <= 13; ++k) fact[k] = fact[k - 1] * (double)k;     // exact: 13! < 2^53
    double q = 1.0 / fact[13];
    for (int k = 12; k >= 0; --k) q = q * t + 1.0 / fact[k];
    return std::ldexp(q, (int)n);
}

// the taps of a blur of sigma s (s <= 7.9 keeps the radius within SIFT_MAX_RADIUS; sigma <= 4 gives s <= 7.73)
inline GaussTaps sift_gauss_taps(double s)
{
    GaussTaps g{};
    const int n_taps = ((int)std::rint(8.0 * s + 1.0)) | 1;
    g.r = n_taps / 2;
    const double d = 2.0 * s * s;
    double e[2 * SIFT_MAX_RADIUS + 1], total = 0.0;
    for (int j = 0; j <= 2 * g.r; ++j) {
        e[j] = sift_exp64(-((double)((j - g.r) * (j - g.r))) / d);
        total = j == 0 ? e[0] : total + e[j];
    }
    for (int j = 0; j <= 2 * g.r; ++j) g.w[j] = (float)(e[j] / total);
    return g;
}

// s[0] the base blur of the doubled image, s[1 .. 5] the incremental blurs of an octave
inline void sift_sigmas(double sigma, double s[6])
{
    const double K3 = 1.2599210498948732;
    s[0] = std::sqrt(std::fmax(sigma * sigma - 1.0, 0.01));
    double prev = sigma;
    for (int i = 1; i <= 5; ++i) {
        const double total = prev * K3;
        s[i] = std::sqrt(total * total - prev * prev);
        prev = total;
    }
}

// floor((L - 3) / 2) + 1 with L the highest set bit of min(h, w)^2; min(h, w) >= 3
inline int sift_octaves(int h, int w)
{
    const long long m = h < w ? h : w, mm = m * m;
    int L = 0;
    while ((mm >> (L + 1)) != 0) ++L;
    return (L - 3) / 2 + 1;              // L >= 3: no negative division
}

}  // namespace amvs

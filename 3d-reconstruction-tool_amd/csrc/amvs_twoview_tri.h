// amvs_twoview_tri.h -- the triangulation of ONE candidate as include/amvs_twoview.h defines it (amvs_match.h steps 1 to 7
// and the header's seven comparisons), for the kernels that run it: twoview_triangulate_kernel (amvs_twoview.hip) and
// sfm_triangulate_kernel (amvs_sfm.hip, include/amvs_sfm.h), so that both produce the same bits from one text.  It forms
// no data-dependent index.  Include after amvs_dlt4.h, amvs_twoview_dev.h and amvs_twoview_host.h, in a unit built with
// -ffp-contract=off.
#pragma once
#include "amvs_dlt4.h"
#include "amvs_twoview_dev.h"
#include "amvs_twoview_host.h"

#include <cstring>

namespace amvs {

struct TriArgs {
    double P1[12], P2[12], C1[3], C2[3], R1[9], t1[3], R2[9], t2[3], K[9];
    TwoviewThresholds thr;
};

// the arguments of a call, formed once on the host
inline TriArgs tri_args(const double *K, const double R1[9], const double t1[3], const double R2[9], const double t2[3],
                        const TwoviewThresholds &thr)
{
    TriArgs a;
    twoview_projection(K, R1, t1, a.P1, a.C1);
    twoview_projection(K, R2, t2, a.P2, a.C2);
    std::memcpy(a.R1, R1, sizeof(a.R1));
    std::memcpy(a.R2, R2, sizeof(a.R2));
    std::memcpy(a.t1, t1, sizeof(a.t1));
    std::memcpy(a.t2, t2, sizeof(a.t2));
    std::memcpy(a.K, K, sizeof(a.K));
    a.thr = thr;
    return a;
}

__device__ __forceinline__ void cam_point(const double R[9], const double t[3], const double X[3], double pc[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = ((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2]) + t[r];
}

__device__ __forceinline__ double reproj_error(const double K[9], const double pc[3], double x, double y)
{
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = (K[3 * r] * pc[0] + K[3 * r + 1] * pc[1]) + K[3 * r + 2] * pc[2];
    const double du = h[0] / h[2] - x, dv = h[1] / h[2] - y;
    return sqrt(du * du + dv * dv);
}

// X and the cosine of the parallax angle of the candidate with pixels (x1, y1), (x2, y2); true: valid
__device__ __forceinline__ bool tri_candidate(const TriArgs &a, double x1, double y1, double x2, double y2, double X[3], double *cos_out)
{
    double v[4];
    dlt4_null_vector(a.P1, a.P2, x1, y1, x2, y2, v);
    X[0] = v[0] / v[3];
    X[1] = v[1] / v[3];
    X[2] = v[2] / v[3];
    double pc1[3], pc2[3];
    cam_point(a.R1, a.t1, X, pc1);
    cam_point(a.R2, a.t2, X, pc2);
    const double w1[3] = {X[0] - a.C1[0], X[1] - a.C1[1], X[2] - a.C1[2]};
    const double w2[3] = {X[0] - a.C2[0], X[1] - a.C2[1], X[2] - a.C2[2]};
    const double dot = (w1[0] * w2[0] + w1[1] * w2[1]) + w1[2] * w2[2];
    const double n1 = sqrt((w1[0] * w1[0] + w1[1] * w1[1]) + w1[2] * w1[2]);
    const double n2 = sqrt((w2[0] * w2[0] + w2[1] * w2[1]) + w2[2] * w2[2]);
    const double cs = dot / (n1 * n2 + 1e-8);
    const double e1 = reproj_error(a.K, pc1, x1, y1), e2 = reproj_error(a.K, pc2, x2, y2);
    *cos_out = cs;
    return pc1[2] > a.thr.depth_min && pc2[2] > a.thr.depth_min && pc1[2] <= a.thr.depth_max && pc2[2] <= a.thr.depth_max &&
           cs <= a.thr.cos_max_parallax && e1 <= a.thr.max_reproj && e2 <= a.thr.max_reproj;
}

}  // namespace amvs

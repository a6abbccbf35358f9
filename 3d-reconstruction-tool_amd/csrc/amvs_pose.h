// amvs_pose.h -- the intrinsics and a pose as the kernels of amvs_pnp.hip, amvs_twoview.hip and amvs_bundle.hip (Intr)
// take them by value.  Private to the library.  In an unnamed namespace, as those kernels are: each unit has its own.
#pragma once
#include <cstring>

namespace amvs {

namespace {

struct Intr { double fx, fy, cx, cy; };
struct Pose { double R[9], t[3]; };

// of the headers' K, double[9] row-major
inline Intr intrinsics_of(const double *K) { return Intr{K[0], K[4], K[2], K[5]}; }

inline Pose pose_of(const double R[9], const double t[3])
{
    Pose P;
    std::memcpy(P.R, R, sizeof(P.R));
    std::memcpy(P.t, t, sizeof(P.t));
    return P;
}

}  // namespace

}  // namespace amvs

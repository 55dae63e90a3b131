// Host side of the radar point cloud (radar_points.hip): the argument checks of both entries and the fuse entry's derived geometry.
// Plain C++ without the HIP runtime, so that a stand-alone host program can be built around it (scripts/radar_points_host_check.cpp).
#pragma once
#include <math.h>
#include <stddef.h>

namespace hupr {

constexpr int kPeaksMaxPoints = 256;      // rows of a points list
constexpr int kPeaksMaxSepRange = 4, kPeaksMaxSepAzimuth = 8;
constexpr int kPeaksStage = 4096;         // peaks staged and ranked per frame
constexpr int kFuseGeometryLen = 14;      // range_bin_m, doppler_mps_per_bin, a_h[3], o_h[3], a_v[3], o_v[3]

// What is wrong with a hupr_radar_peaks_f32 call's settings, or null.
inline const char* peaks_check(int n, int max_points, int sep_range, int sep_azimuth) {
    if (n < 0) return "negative frame count";
    if (max_points < 1 || max_points > kPeaksMaxPoints) return "max_points outside 1..256";
    if (sep_range < 0 || sep_range > kPeaksMaxSepRange) return "sep_range outside 0..4";
    if (sep_azimuth < 0 || sep_azimuth > kPeaksMaxSepAzimuth) return "sep_azimuth outside 0..8";
    return nullptr;
}

// What the fuse kernel needs of the geometry, by value with the launch: the two array axes, the third axis b = +-(a_v x a_h) with
// b . y > 0, and the origins' components along them.
struct FuseGeometry {
    double range_bin_m, doppler_mps_per_bin;
    double a_h[3], a_v[3], b[3];
    double oh_ah, ov_av, oh_av, oh_b;
};

inline double fuse_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// What is wrong with a hupr_radar_points_fuse_f32 call's settings, or null; fills `out` (if given) when nothing is.
inline const char* fuse_check(int n, int max_h, int max_v, const double* geometry, double range_gate, int doppler_gate, FuseGeometry* out) {
    if (n < 0) return "negative frame count";
    if (max_h < 1 || max_h > kPeaksMaxPoints || max_v < 1 || max_v > kPeaksMaxPoints) return "max_points outside 1..256";
    if (!(range_gate >= 0.0) || !isfinite(range_gate)) return "range_gate must be finite and >= 0";
    if (doppler_gate < 0 || doppler_gate > 7) return "doppler_gate outside 0..7";
    if (!geometry) return "null geometry";
    for (int i = 0; i < kFuseGeometryLen; ++i)
        if (!isfinite(geometry[i])) return "the geometry holds a value that is not finite";
    if (!(geometry[0] > 0.0)) return "range_bin_m must be positive";
    if (!(geometry[1] > 0.0)) return "doppler_mps_per_bin must be positive";
    const double *a_h = geometry + 2, *o_h = geometry + 5, *a_v = geometry + 8, *o_v = geometry + 11;
    if (fabs(fuse_dot(a_h, a_h) - 1.0) > 1e-9 || fabs(fuse_dot(a_v, a_v) - 1.0) > 1e-9) return "an array axis is no unit vector";
    if (fabs(fuse_dot(a_h, a_v)) > 1e-9) return "the two array axes are not orthogonal";
    double b[3] = {a_v[1] * a_h[2] - a_v[2] * a_h[1], a_v[2] * a_h[0] - a_v[0] * a_h[2], a_v[0] * a_h[1] - a_v[1] * a_h[0]};
    if (!(fabs(b[1]) > 1e-9)) return "the boresight y lies in the plane of the two array axes";
    if (b[1] < 0.0)
        for (int k = 0; k < 3; ++k) b[k] = -b[k];
    if (out) {
        out->range_bin_m = geometry[0];
        out->doppler_mps_per_bin = geometry[1];
        for (int k = 0; k < 3; ++k) {
            out->a_h[k] = a_h[k];
            out->a_v[k] = a_v[k];
            out->b[k] = b[k];
        }
        out->oh_ah = fuse_dot(o_h, a_h);
        out->ov_av = fuse_dot(o_v, a_v);
        out->oh_av = fuse_dot(o_h, a_v);
        out->oh_b = fuse_dot(o_h, b);
    }
    return nullptr;
}

}  // namespace hupr

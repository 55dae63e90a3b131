// The constant-velocity model shared by the Kalman tracker (pose_track.hip) and the Rauch-Tung-Striebel smoother that runs backwards
// over its recorded states (pose_smooth.hip).  The status codes of both are the HUPR_TRACK_* / HUPR_SMOOTH_* of include/hupr.h.
#pragma once
#include "hupr_common.h"

namespace hupr {

constexpr int kTrackFloats = 16;      // per row: x, y, vx, vy, the 10 upper-triangle entries of P (row-major), live, coast

// white-acceleration process noise of one frame of dt seconds: per axis [[q11, q12], [q12, q22]] on (position, velocity)
struct ProcessNoise {
    float q11, q12, q22;
};
__device__ __forceinline__ ProcessNoise process_noise(float accel_psd, float dt) {
    return {accel_psd * dt * dt * dt * (1.f / 3.f), accel_psd * dt * dt * 0.5f, accel_psd * dt};
}

}  // namespace hupr

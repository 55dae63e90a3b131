// The One-Euro filter (Casiez et al., CHI 2012) on a decoded image-pixel keypoint, shared by hupr_k_pose_decode (pose_decode.hip) and
// hupr_k_pose_decode_integral (pose_integral.hip): one state layout, one recurrence and one parameter rule, so that the two advance
// the same [rows][kFilterFloats] state to the same bits and a session may change the decode on a live state.  The rule is stated
// beside hupr_pose_decode_f32 in include/hupr.h.
#pragma once
#include "hupr_common.h"
#include "pose_refine.h"

namespace hupr {

constexpr int kFilterFloats = 8;      // per row: x, y, dx, dy (filtered position and velocity), valid, 3 x pad

struct OneEuro {
    float rate, min_cutoff, beta, d_cutoff, min_score;
};

__device__ __forceinline__ float euro_alpha(float rate, float cutoff) { return 1.f / (1.f + rate / (6.283185307179586f * cutoff)); }

// One filter step of row r on the raw keypoint (x, y) whose maximum is ``best``, called by lane 0 of the row's wave: reads and writes
// the row's state and stores the filtered keypoint and the velocity where those pointers are given.  Nothing without a state.
__device__ __forceinline__ void euro_step(float* state, long r, OneEuro f, float best, float x, float y, float* filtered,
                                          float* velocity) {
    if (!state) return;
    float* s = state + r * kFilterFloats;
    const float sx = s[0], sy = s[1], svx = s[2], svy = s[3];
    const bool valid = s[4] != 0.f;
    const bool missing = !(best > f.min_score) || !finitef(x) || !finitef(y);
    float fx = x, fy = y, vx = 0.f, vy = 0.f;
    if (missing) {
        if (valid) { fx = sx; fy = sy; }                  // the joint holds its place; the state is left as it is
    } else {
        if (valid) {
            const float ad = euro_alpha(f.rate, f.d_cutoff);
            const float rx = (x - sx) * f.rate, ry = (y - sy) * f.rate;
            vx = ad * rx + (1.f - ad) * svx;
            vy = ad * ry + (1.f - ad) * svy;
            const float ax = euro_alpha(f.rate, f.min_cutoff + f.beta * fabsf(vx));
            const float ay = euro_alpha(f.rate, f.min_cutoff + f.beta * fabsf(vy));
            fx = ax * x + (1.f - ax) * sx;
            fy = ay * y + (1.f - ay) * sy;
        }
        s[0] = fx;
        s[1] = fy;
        s[2] = vx;
        s[3] = vy;
        s[4] = 1.f;
    }
    if (filtered) *reinterpret_cast<float2*>(filtered + r * 2) = make_float2(fx, fy);
    if (velocity) *reinterpret_cast<float2*>(velocity + r * 2) = make_float2(vx, vy);
}

// the filter rule shared by the entries of both decodes
static inline int euro_check(const char* name, const float* state, const OneEuro& f, const float* filtered, const float* velocity) {
    if (state) {
        HUPR_REQUIRE(f.rate > 0.f && f.rate < INFINITY && f.min_cutoff > 0.f && f.min_cutoff < INFINITY && f.d_cutoff > 0.f &&
                         f.d_cutoff < INFINITY && f.beta >= 0.f && f.beta < INFINITY && f.min_score == f.min_score,
                     "%s: bad filter parameter (rate_hz %g, min_cutoff %g and d_cutoff %g must be positive, beta %g non-negative, "
                     "min_score %g a number)", name, f.rate, f.min_cutoff, f.d_cutoff, f.beta, f.min_score);
    } else {
        HUPR_REQUIRE(!filtered && !velocity, "%s: filtered keypoints / velocity asked for without a filter state", name);
    }
    return HUPR_OK;
}

}  // namespace hupr

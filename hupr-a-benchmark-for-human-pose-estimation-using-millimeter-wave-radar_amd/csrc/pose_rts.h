// One backward step of the Rauch-Tung-Striebel smoother, shared by the fixed-interval kernel (pose_smooth.hip) and the fixed-lag one
// (pose_lag.hip): both compile these very expressions, so that a window of the one is a recording of the other bit for bit.  The rule
// is stated in full beside hupr_pose_smooth_rts_f32 in include/hupr.h; the tracker's model is pose_track_model.h's.
#pragma once
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"

namespace hupr {

// the upper triangle of a symmetric 4 x 4 matrix row by row, as the tracker's state keeps it
__host__ __device__ constexpr int tri(int i, int j) { return i <= j ? i * (9 - i) / 2 + (j - i) : j * (9 - j) / 2 + (i - j); }

// One backward step.  x, p: the filter's state of frame k; xs, ps: the smoothed state of frame k + 1 on entry, of frame k on return.
// false (xs, ps untouched) where a Cholesky pivot is not positive and finite or a result is not finite.
__device__ __forceinline__ bool rts_step(const float (&x)[4], const float (&p)[10], float (&xs)[4], float (&ps)[10], float dt,
                                         ProcessNoise q) {
    // ---- predict, with the tracker's own expressions: xp = F x, Pp = F P F^T + Q ------------------------------------------------------
    float xp[4] = {x[0] + dt * x[2], x[1] + dt * x[3], x[2], x[3]};
    float pp[10];
    pp[tri(0, 0)] = p[tri(0, 0)] + (dt * (2.f * p[tri(0, 2)]) + dt * dt * p[tri(2, 2)] + q.q11);
    pp[tri(0, 1)] = p[tri(0, 1)] + (dt * (p[tri(0, 3)] + p[tri(1, 2)]) + dt * dt * p[tri(2, 3)]);
    pp[tri(1, 1)] = p[tri(1, 1)] + (dt * (2.f * p[tri(1, 3)]) + dt * dt * p[tri(3, 3)] + q.q11);
    pp[tri(0, 2)] = p[tri(0, 2)] + (dt * p[tri(2, 2)] + q.q12);
    pp[tri(0, 3)] = p[tri(0, 3)] + dt * p[tri(2, 3)];
    pp[tri(1, 2)] = p[tri(1, 2)] + dt * p[tri(2, 3)];
    pp[tri(1, 3)] = p[tri(1, 3)] + (dt * p[tri(3, 3)] + q.q12);
    pp[tri(2, 2)] = p[tri(2, 2)] + q.q22;
    pp[tri(2, 3)] = p[tri(2, 3)];
    pp[tri(3, 3)] = p[tri(3, 3)] + q.q22;

    // ---- Cholesky Pp = L L^T, column by column; l[tri(i, j)] = L[i][j] for i >= j ------------------------------------------------------
    float l[10], inv[4];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float d = pp[tri(j, j)];
#pragma unroll
        for (int m = 0; m < j; ++m) d -= l[tri(j, m)] * l[tri(j, m)];
        ok = ok && d > 0.f && finitef(d);
        const float root = sqrtf(d);
        l[tri(j, j)] = root;
        inv[j] = 1.f / root;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            float v = pp[tri(i, j)];
#pragma unroll
            for (int m = 0; m < j; ++m) v -= l[tri(i, m)] * l[tri(j, m)];
            l[tri(i, j)] = v * inv[j];
        }
    }

    // ---- C = P F^T Pp^-1: row i of C solves L L^T c = (P F^T)[i][:]^T, forward then backward ---------------------------------------------
    float c[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a[4] = {p[tri(i, 0)] + dt * p[tri(i, 2)], p[tri(i, 1)] + dt * p[tri(i, 3)], p[tri(i, 2)], p[tri(i, 3)]};
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = a[j];
#pragma unroll
            for (int m = 0; m < j; ++m) v -= l[tri(j, m)] * y[m];
            y[j] = v * inv[j];
        }
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            float v = y[j];
#pragma unroll
            for (int m = j + 1; m < 4; ++m) v -= l[tri(m, j)] * c[i][m];
            c[i][j] = v * inv[j];
        }
    }

    // ---- xs = x + C (xs' - xp);  Ps = P + C (Ps' - Pp) C^T, symmetrised ---------------------------------------------------------------------
    float dx[4], d[10];
#pragma unroll
    for (int j = 0; j < 4; ++j) dx[j] = xs[j] - xp[j];
#pragma unroll
    for (int j = 0; j < 10; ++j) d[j] = ps[j] - pp[j];
    float nx[4], m[4][4], n[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        nx[i] = x[i] + (c[i][0] * dx[0] + c[i][1] * dx[1] + c[i][2] * dx[2] + c[i][3] * dx[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            m[i][j] = c[i][0] * d[tri(0, j)] + c[i][1] * d[tri(1, j)] + c[i][2] * d[tri(2, j)] + c[i][3] * d[tri(3, j)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            n[i][j] = p[tri(i, j)] + (m[i][0] * c[j][0] + m[i][1] * c[j][1] + m[i][2] * c[j][2] + m[i][3] * c[j][3]);
    float np[10];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) np[tri(i, j)] = i == j ? n[i][i] : 0.5f * (n[i][j] + n[j][i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && finitef(nx[j]);
#pragma unroll
    for (int j = 0; j < 10; ++j) ok = ok && finitef(np[j]);
    if (ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[j] = nx[j];
#pragma unroll
        for (int j = 0; j < 10; ++j) ps[j] = np[j];
    }
    return ok;
}

}  // namespace hupr

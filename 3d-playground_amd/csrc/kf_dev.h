// Device functions of the tracker's Kalman filter shared by kf.hip and track_step.hip: both write Torch_KF.view rows and have to agree
// bit for bit.  Compile the including file with -ffp-contract=off (the Makefile's EXACT list).
#pragma once
#include "common.h"

#define KS 6   // state size
#define KM 5   // measurement size

__device__ __forceinline__ float kf_f05(float D, double dt, int dt_is_tensor) {
    return dt_is_tensor ? (float)((double)D * dt) : D * (float)dt;              // kf.py:278 / 310
}

// One row of Torch_KF.view (kf.py:264-289): x [KS] is the object's state, d its direction; has_dt = 0 copies the state, else the state
// is rolled forward by F with F[0][5] = d * dt.  o receives KS values, or KS + 1 with the direction inserted before the speed.
__device__ __forceinline__ void kf_view_row(const float (&x)[KS], float d, const float *__restrict__ F, int has_dt, double dt,
                                            int dt_is_tensor, int with_direction, float *__restrict__ o) {
    float xp[KS];
    if (has_dt) {
        const float f05 = kf_f05(d, dt, dt_is_tensor);
#pragma unroll
        for (int a = 0; a < KS; ++a) {
            float s = 0.f;
#pragma unroll
            for (int b = 0; b < KS; ++b) s += ((a == 0 && b == 5) ? f05 : F[a * KS + b]) * x[b];
            xp[a] = s;
        }
    } else {
#pragma unroll
        for (int a = 0; a < KS; ++a) xp[a] = x[a];
    }
    if (with_direction) {                                                       // cat(states[:, :-1], D, states[:, -1:]), kf.py:287
#pragma unroll
        for (int a = 0; a < KS - 1; ++a) o[a] = xp[a];
        o[KS - 1] = d;
        o[KS] = xp[KS - 1];
    } else {
#pragma unroll
        for (int a = 0; a < KS; ++a) o[a] = xp[a];
    }
}

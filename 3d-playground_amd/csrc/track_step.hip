// Front end of the tracker's crop frame (MC3D_crop_tracker.py:1150-1171), one lane per track.
//
// The reference views the filter 1/30 s ahead, builds [n, c] distance matrices to the camera centres with repeat / pow / argmin on
// the host, and then collects one Python float per track (time stamp + bias of the camera picked) for get_dt.  Here one launch
// writes the view, the camera and the per-track dt the following predict needs; nothing leaves the device.
//   pre_loc  the row rn_kf_view writes for the scalar dt = 1/30.0 with direction (kf_dev.h: the same device function)
//   cam      first k attaining the minimum of |(cx_k - x)(cx_k - x) + (cy_k - y)(cy_k - y)|, fp32, one rounding per operation; a NaN
//            distance counts as smaller than any number, so the first NaN wins (torch.argmin's rule on the CPU)
//   dt       (stamps[cam] + bias[cam]) - T in fp64: the time stamp sum is a Python float sum in the reference, get_dt subtracts T
// Latency-bound by construction: a few hundred tracks, up to a few dozen cameras.  Compiled with -ffp-contract=off.
#include "common.h"
#include "kf_dev.h"

__global__ __launch_bounds__(128) void track_crop_prior_kernel(const float *__restrict__ X, const float *__restrict__ D,
                                                               const double *__restrict__ T, const float *__restrict__ F,
                                                               const float *__restrict__ centers, const double *__restrict__ stamps,
                                                               const double *__restrict__ bias, int n_cam,
                                                               float *__restrict__ pre_loc, int32_t *__restrict__ cam,
                                                               double *__restrict__ dt, int n) {
    const int i = blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    float x[KS], o[KS + 1];
#pragma unroll
    for (int a = 0; a < KS; ++a) x[a] = X[i * KS + a];
    kf_view_row(x, D[i], F, 1, 1.0 / 30.0, 0, 1, o);                             // :1150
#pragma unroll
    for (int a = 0; a < KS + 1; ++a) pre_loc[(int64_t)i * (KS + 1) + a] = o[a];
    int best_k = 0;
    float best = 0.f;
    for (int k = 0; k < n_cam; ++k) {                                           // :1156-1163
        const float dx = centers[2 * k] - o[0], dy = centers[2 * k + 1] - o[1];
        const float dist = fabsf(dx * dx + dy * dy);
        if (k == 0 || (best == best && (dist != dist || dist < best))) {
            best = dist;
            best_k = k;
        }
    }
    cam[i] = best_k;
    dt[i] = (stamps[best_k] + bias[best_k]) - T[i];                             // :1169-1171
}

extern "C" int rn_track_crop_prior(const float *X, const float *D, const double *T, const float *F, const float *centers,
                                   const double *stamps, const double *bias, int n_cam, float *pre_loc, int32_t *cam, double *dt,
                                   int n, void *stream) {
    if (n_cam < 1 || n < 0) return (int)hipErrorInvalidValue;
    if (n == 0) return RN_OK;
    if (!X || !D || !T || !F || !centers || !stamps || !bias || !pre_loc || !cam || !dt) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(track_crop_prior_kernel, dim3(rn_blocks(n, 128)), dim3(128), 0, (hipStream_t)stream, X, D, T, F, centers,
                       stamps, bias, n_cam, pre_loc, cam, dt, n);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

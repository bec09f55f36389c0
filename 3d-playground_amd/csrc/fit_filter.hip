// Fitting the Kalman filter's covariances (fit_filter_3D.py), device-resident.
//
// The reference script runs tracklets and detector frames through the homography and the filter and then takes moments
// of the residuals in Python loops; the transforms and the filter step already run on the device (homography.hip,
// kf.hip).  This file adds the two pieces that were missing:
//   fit_nearest_kernel   the search of fit_filter_3D.py:356-375: per frame the road-plane footprints of its detections
//                        (:357-361) and of the ground truth (:331-336), the script's own iou (:30-61) in fp32, and the
//                        first detection whose distance 1.0 - iou is strictly below the running minimum (:363-372).  One
//                        wave per frame: lane l scans detections l, l + 64, ... (inside a lane the strict < keeps the
//                        lowest index), then a wave argmin in which equal distances go to the lower index -- together the
//                        serial loop's choice.  A NaN distance compares false and never wins, as in the script.
//   fit_compact_kernel   one workgroup: an exclusive scan of the "has a match" flags in frame order, the residual
//                        det[:5] - gt[:5] of every matched frame (:374-375) written behind its offset, and the counts
//   moments_kernel       the mean / covariance loops of :292-299, :377-384, :426-434, :471-478.  One workgroup per group:
//                        thread t adds rows t, t + 256, ... in fp64 (a fixed order), the partials meet in the xor tree of
//                        wave_sum and then wave 0 .. 3 in order, and each sum is rounded to fp32 once.  No atomics: the
//                        same input gives the same bits.  The covariance is centred on the fp32-rounded mean with the
//                        difference itself rounded to fp32, as the script's `vec - mean`; the products of two fp32
//                        values are exact in fp64.
// Compiled with -ffp-contract=off: one rounding per operation, in the script's order.
#include <math.h>

#include "common.h"
#include "homography_dev.h"
#include "wave_dev.h"

#define FIT_WAVES 4

// max(a, b) / min(a, b) of Python on two numbers: the second wins only when it compares strictly better
__device__ __forceinline__ float py_max(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ float py_min(float a, float b) { return b < a ? b : a; }

// fit_filter_3D.py:30-61 with a = the detection's footprint and b = the ground truth's, every operation in fp32.
// max(0, t) is t when t > 0 and the integer 0 otherwise (a NaN t included)
__device__ __forceinline__ float fit_iou(const float4 a, const float4 b) {
    const float area_a = (a.z - a.x) * (a.w - a.y);                             // :49
    const float area_b = (b.z - b.x) * (b.w - b.y);                             // :50
    const float minx = py_max(a.x, b.x), maxx = py_min(a.z, b.z);               // :52-53
    const float miny = py_max(a.y, b.y), maxy = py_min(a.w, b.w);               // :54-55
    const float dx = maxx - minx, dy = maxy - miny;
    const float inter = (dx > 0.f ? dx : 0.f) * (dy > 0.f ? dy : 0.f);          // :57
    const float uni = (area_a + area_b) - inter;                                // :58
    return __fdiv_rn(inter, uni);                                               // :59
}

// the detections of frame b: offsets clamped into [0, D] and made monotonic, so that no row outside det is read
__device__ __forceinline__ void fit_range(const int32_t *__restrict__ offsets, int b, int D, int &lo, int &hi) {
    lo = offsets[b];
    hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > D ? D : lo);
    hi = hi < lo ? lo : (hi > D ? D : hi);
}

__global__ __launch_bounds__(64 * FIT_WAVES) void fit_nearest_kernel(const float *__restrict__ gt,
                                                                    const float *__restrict__ det,
                                                                    const int32_t *__restrict__ offsets, int B, int D,
                                                                    int32_t *__restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * FIT_WAVES + (threadIdx.x >> 6);                  // wave-uniform
    if (b >= B) return;
    int lo, hi;
    fit_range(offsets, b, D, lo, hi);
    float g[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) g[q] = gt[(int64_t)b * 6 + q];
    const float4 fg = hg_footprint(g);
    float best = INFINITY;                                                      // min_dist = np.inf (:363)
    int arg = RN_NO_INDEX;
    for (int j = lo + lane; j < hi; j += 64) {
        float s[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) s[q] = det[(int64_t)j * 6 + q];
        const float dist = 1.0f - fit_iou(hg_footprint(s), fg);                 // :367
        if (dist < best) { best = dist; arg = j; }                              // :370-372
    }
    wave_arg_first(best, arg, rn_lt_first<float>());
    if (lane == 0) rows[b] = arg == RN_NO_INDEX ? -1 : arg;
}

// one workgroup of 1024; the frames are taken 1024 at a time, in order
__global__ __launch_bounds__(1024) void fit_compact_kernel(const float *__restrict__ gt, const float *__restrict__ det,
                                                           const int32_t *__restrict__ offsets, int B, int D,
                                                           const int32_t *__restrict__ rows, float *__restrict__ resid,
                                                           int32_t *__restrict__ info) {
    __shared__ int wave_tot[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int base = 0, n_empty = 0, n_bad = 0;
    for (int b0 = 0; b0 < B; b0 += 1024) {
        const int b = b0 + t;
        int row = -1;
        if (b < B) {
            int lo, hi;
            fit_range(offsets, b, D, lo, hi);
            row = rows[b];
            if (row < lo || row >= hi) row = -1;                                // only a row of the frame itself is read
            if (hi <= lo) ++n_empty;                                            // the script's `continue` (:343-344)
            else if (row < 0) ++n_bad;                                          // no distance compared below infinity
        }
        const int has = row >= 0;
        int total;
        const int incl = block_scan_incl<16>(has, wave_tot, total);
        if (has) {
            const int k = base + incl - 1;                                      // k <= b < B: inside resid [B,5]
#pragma unroll
            for (int q = 0; q < 5; ++q) resid[(int64_t)k * 5 + q] = det[(int64_t)row * 6 + q] - gt[(int64_t)b * 6 + q];   // :374-375
        }
        base += total;
    }
    n_empty = wave_sum(n_empty);
    n_bad = wave_sum(n_bad);
    __shared__ int cnt[16][2];
    if (lane == 0) { cnt[wv][0] = n_empty; cnt[wv][1] = n_bad; }
    __syncthreads();
    if (t == 0) {
        int e = 0, u = 0;
        for (int k = 0; k < 16; ++k) { e += cnt[k][0]; u += cnt[k][1]; }
        info[0] = base;
        info[1] = e;
        info[2] = u;
    }
}

extern "C" int rn_fit_nearest(const float *gt, const float *det, const int32_t *offsets, int64_t B, int64_t D,
                              int32_t *rows, float *resid, int32_t *info, void *stream) {
    if (B < 0 || D < 0 || B > RN_FIT_MAX || D > RN_FIT_MAX || !info) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        hipError_t e = hipMemsetAsync(info, 0, 12, s);
        return e != hipSuccess ? (int)e : RN_OK;
    }
    if (!gt || !offsets || !rows || !resid || (D > 0 && !det)) return RN_EINVAL;
    hipLaunchKernelGGL(fit_nearest_kernel, dim3(rn_blocks(B, FIT_WAVES)), dim3(64 * FIT_WAVES), 0, s, gt, det, offsets,
                       (int)B, (int)D, rows);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(fit_compact_kernel, dim3(1), dim3(1024), 0, s, gt, det, offsets, (int)B, (int)D,
                       (const int32_t *)rows, resid, info);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ------------------------------------------------------------------------------------------------ moments
#define MOM_THREADS 256
#define MOM_TRI (RN_MOMENTS_MAX_K * (RN_MOMENTS_MAX_K + 1) / 2)

// the block's total of NV per-thread fp64 values, in a fixed order: the xor tree inside a wave, then waves 0 .. 3 in
// order; every thread gets the totals.  `red` holds 4 * NV doubles.
template <int NV>
__device__ __forceinline__ void mom_block_sum(double (&v)[NV], int nv, double *red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();                                                            // red may still be read from the last call
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i < nv) {
            v[i] = wave_sum(v[i]);
            if (lane == 0) red[wv * NV + i] = v[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (i < nv) v[i] = ((red[i] + red[NV + i]) + red[2 * NV + i]) + red[3 * NV + i];
}

__global__ __launch_bounds__(MOM_THREADS) void moments_kernel(const float *__restrict__ E, int64_t N, int k,
                                                              const int32_t *__restrict__ group,
                                                              float *__restrict__ mean, float *__restrict__ cov,
                                                              int32_t *__restrict__ count) {
    __shared__ double red[4 * MOM_TRI];
    const int g = blockIdx.x, t = threadIdx.x;
    double s[RN_MOMENTS_MAX_K];
#pragma unroll
    for (int i = 0; i < RN_MOMENTS_MAX_K; ++i) s[i] = 0.0;
    int n = 0;
    for (int64_t r = t; r < N; r += MOM_THREADS) {
        if (group && group[r] != g) continue;
        ++n;
#pragma unroll
        for (int i = 0; i < RN_MOMENTS_MAX_K; ++i)
            if (i < k) s[i] += (double)E[r * k + i];
    }
    n = wave_sum(n);
    __shared__ int nred[4];
    if ((t & 63) == 0) nred[t >> 6] = n;
    mom_block_sum<RN_MOMENTS_MAX_K>(s, k, red);
    n = ((nred[0] + nred[1]) + nred[2]) + nred[3];
    float mu[RN_MOMENTS_MAX_K];
#pragma unroll
    for (int i = 0; i < RN_MOMENTS_MAX_K; ++i) mu[i] = (i < k && n > 0) ? (float)(s[i] / (double)n) : 0.f;   // torch.mean: fp32
    double c[MOM_TRI];
#pragma unroll
    for (int i = 0; i < MOM_TRI; ++i) c[i] = 0.0;
    for (int64_t r = t; r < N; r += MOM_THREADS) {
        if (group && group[r] != g) continue;
        float d[RN_MOMENTS_MAX_K];
#pragma unroll
        for (int i = 0; i < RN_MOMENTS_MAX_K; ++i) d[i] = i < k ? E[r * k + i] - mu[i] : 0.f;   // vec - mean, fp32
        int q = 0;
#pragma unroll
        for (int i = 0; i < RN_MOMENTS_MAX_K; ++i)
#pragma unroll
            for (int j = i; j < RN_MOMENTS_MAX_K; ++j, ++q)
                if (j < k) c[q] += (double)d[i] * (double)d[j];
    }
    mom_block_sum<MOM_TRI>(c, MOM_TRI, red);
    if (t == 0) {
        count[g] = n;
#pragma unroll
        for (int i = 0; i < RN_MOMENTS_MAX_K; ++i)
            if (i < k) mean[g * k + i] = mu[i];
        int q = 0;
#pragma unroll
        for (int i = 0; i < RN_MOMENTS_MAX_K; ++i)
#pragma unroll
            for (int j = i; j < RN_MOMENTS_MAX_K; ++j, ++q)
                if (j < k) {
                    const float v = n > 0 ? (float)(c[q] / (double)n) : 0.f;    // covariance / error_vectors.shape[0]
                    cov[(g * k + i) * k + j] = v;
                    cov[(g * k + j) * k + i] = v;
                }
    }
}

extern "C" int rn_residual_moments(const float *E, int64_t N, int k, const int32_t *group, int G, float *mean,
                                   float *cov, int32_t *count, void *stream) {
    if (N < 0 || k < 1 || k > RN_MOMENTS_MAX_K || G < 1 || G > RN_MOMENTS_MAX_G || (!group && G != 1) || !mean || !cov ||
        !count || (N > 0 && !E))
        return RN_EINVAL;
    hipLaunchKernelGGL(moments_kernel, dim3(G), dim3(MOM_THREADS), 0, (hipStream_t)stream, E, N, k, group, mean, cov,
                       count);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

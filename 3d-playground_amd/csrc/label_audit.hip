// The batch passes of the reference's annotator (seems_to_be_working.py) over a whole multi-camera label set:
//   Annotator.estimate_ts_bias (:1845-1947), est_y_error (:1950-2036), estimate_projection_error (:2249-2357),
//   remove_outliers (:2192-2233), interpolate (:780-836).
//
// The reference walks camera pairs x objects x ALL frames with one string-keyed dict lookup per step.  Here the host packs the
// labels once into a CSR table of tracklets -- tracklet t = object * n_cam + camera, rows in ascending frame, columns fp64
// (x, y, timestamp) plus the int32 frame index -- and everything proportional to rows runs here:
//   la_pair_kernel      one wave per (camera pair, object): min / max of the key column of both tracklets (wave reduction), the
//                       reference's overlap guard, the five sample points, for each point and tracklet the LAST segment that
//                       brackets it (the reference's loop overwrites: the last one wins), then lanes 0..4 interpolate one point
//                       each.  Key = x and value = timestamp / y for the first two estimators, key = timestamp and values = x, y
//                       for the third.  The kernel writes samples and flags only; diffs, means and the serial walk over the
//                       cameras are the host's (numpy's own summation on the same lists).
//   la_outliers_kernel  one lane per tracklet, serial over its rows: the reference deletes in place while it walks the frames, so
//                       whether a row's previous-frame neighbour still exists depends on the row before (a recurrence).
//   la_gap_kernel       one wave per tracklet: missing frames after every row, their exclusive prefix inside the tracklet
//   la_prefix_kernel    one workgroup: exclusive prefix of the tracklets' totals (int64)
//   la_fill_kernel      one thread per missing frame: two binary searches (tracklet, row), then the time-weighted mean of the
//                       two boxes around the gap at the camera's own time stamps
//
// Arithmetic: fp64, one rounding per operation in the reference's order (this file is in the Makefile's EXACT list: no fma
// contraction), so every sample and every filled box equals Python's floats bit for bit.
//
// Every index read from memory is checked before use (row ranges inside the R rows, frame indices inside the F frames and
// ascending along a tracklet, destinations inside the U output rows).  A bad value sets a bit of *status and the item is left
// out; it is never used as an index.  No kernel spins or asserts.
#include <math.h>

#include "common.h"
#include "wave_dev.h"

#define LA_THREADS 256
#define LA_WAVES (LA_THREADS / RN_WAVE)
#define LA_MAX ((int64_t)1 << 31)

// rows [lo, hi) of tracklet t; the caller guarantees 0 <= t < T (offsets holds T + 1 entries)
__device__ __forceinline__ bool la_rows(const int64_t *__restrict__ off, int64_t t, int64_t R, int64_t &lo, int64_t &hi) {
    lo = off[t];
    hi = off[t + 1];
    return lo >= 0 && lo <= hi && hi <= R;
}

// min and max of column kc over rows [lo, hi), wave-uniform
__device__ __forceinline__ void la_minmax(const double *__restrict__ cols, int kc, int64_t lo, int64_t hi, int lane, double &mn,
                                          double &mx) {
    mn = INFINITY;
    mx = -INFINITY;
    for (int64_t r = lo + lane; r < hi; r += RN_WAVE) {
        const double k = cols[r * 3 + kc];
        mn = fmin(mn, k);
        mx = fmax(mx, k);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
}

// for each of the five points, the last i in [1, n) with (K[i] - pt) * (K[i-1] - pt) <= 0 (0: none), wave-uniform
__device__ __forceinline__ void la_last_crossing(const double *__restrict__ cols, int kc, int64_t lo, int64_t n, int lane,
                                                 const double (&pt)[RN_LABEL_POINTS], int (&best)[RN_LABEL_POINTS]) {
#pragma unroll
    for (int q = 0; q < RN_LABEL_POINTS; ++q) best[q] = 0;
    for (int64_t i = 1 + lane; i < n; i += RN_WAVE) {                           // ascending per lane: the last hit is its largest
        const double ka = cols[(lo + i) * 3 + kc], kb = cols[(lo + i - 1) * 3 + kc];
#pragma unroll
        for (int q = 0; q < RN_LABEL_POINTS; ++q)
            if ((ka - pt[q]) * (kb - pt[q]) <= 0.0) best[q] = (int)i;           // :1908 (NaN compares false, as in Python)
    }
#pragma unroll
    for (int q = 0; q < RN_LABEL_POINTS; ++q) best[q] = wave_max(best[q]);
}

// value of column vc at key `pt` on segment (i - 1, i) of the tracklet at row lo (:1909-1910)
__device__ __forceinline__ double la_sample(const double *__restrict__ cols, int kc, int vc, int64_t lo, int i, double pt) {
    const double *a = cols + (lo + i) * 3, *b = cols + (lo + i - 1) * 3;
    const double ratio = (pt - b[kc]) / ((a[kc] - b[kc]) + 1e-08);
    return b[vc] + (a[vc] - b[vc]) * ratio;
}

// every output is written exactly once, by the lane that owns it: no guard, nothing found, zeros
__device__ __forceinline__ void la_no_samples(uint8_t *fl, double *o, int lane) {
    if (lane < RN_LABEL_POINTS) {
        fl[lane] = 0;
        o[0] = o[1] = o[2] = o[3] = 0.0;
    }
}

// ---- samples: one wave per (pair, object); pair = cam * (cam - 1) / 2 + prev for prev < cam
__global__ void __launch_bounds__(LA_THREADS) la_pair_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                             int64_t R, int C, int64_t N, int64_t entries, int kc, int v0, int v1,
                                                             uint8_t *__restrict__ flags, double *__restrict__ values,
                                                             int32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * LA_WAVES + (threadIdx.x >> 6);      // wave-uniform, like every exit below
    if (e >= entries) return;
    const int64_t pair = e / N, obj = e % N;
    int cam = 1;
    while (cam < C - 1 && (int64_t)(cam + 1) * cam / 2 <= pair) ++cam;
    const int prev = (int)(pair - (int64_t)cam * (cam - 1) / 2);                // < cam: entries = C (C - 1) / 2 * N
    uint8_t *fl = flags + e * RN_LABEL_POINTS;                                  // lane q < 5 owns point q: its flag byte, its four values
    double *o = values + e * (RN_LABEL_POINTS * 4) + (lane < RN_LABEL_POINTS ? lane : 0) * 4;
    int64_t a0, a1, b0, b1;                                                     // c1 = the camera's tracklet, c0 = the partner's
    const bool ok_a = la_rows(off, obj * C + cam, R, a0, a1), ok_b = la_rows(off, obj * C + prev, R, b0, b1);
    if (!ok_a || !ok_b) {
        if (lane == 0) rn_flag(status, RN_LABEL_BAD_OFFSETS);
        la_no_samples(fl, o, lane);
        return;
    }
    const int64_t n1 = a1 - a0, n0 = b1 - b0;
    double mn1 = 0.0, mx1 = 0.0, mn0 = 0.0, mx0 = 0.0;
    const bool both = n1 > 1 && n0 > 1;                                         // :1889
    if (both) {
        la_minmax(cols, kc, a0, a1, lane, mn1, mx1);
        la_minmax(cols, kc, b0, b1, lane, mn0, mx0);
    }
    if (!both || !(mx0 > mn1)) {                                                // :1889
        la_no_samples(fl, o, lane);
        return;
    }
    const double lo = fmax(mn1, mn0), hi = fmin(mx1, mx0);                      // :1892-1893
    const double ran = hi - lo, step = ran / 4.0;                               // :1897, ran / (p - 1)
    double pt[RN_LABEL_POINTS];
#pragma unroll
    for (int q = 0; q < RN_LABEL_POINTS; ++q) pt[q] = lo + step * (double)q;    // :1900
    int best1[RN_LABEL_POINTS], best0[RN_LABEL_POINTS];
    la_last_crossing(cols, kc, a0, n1, lane, pt, best1);
    la_last_crossing(cols, kc, b0, n0, lane, pt, best0);
    if (lane < RN_LABEL_POINTS) {
        int i1 = 0, i0 = 0;
        double p = 0.0;
#pragma unroll
        for (int q = 0; q < RN_LABEL_POINTS; ++q)
            if (lane == q) { i1 = best1[q]; i0 = best0[q]; p = pt[q]; }
        o[0] = i1 > 0 ? la_sample(cols, kc, v0, a0, i1, p) : 0.0;
        o[1] = i0 > 0 ? la_sample(cols, kc, v0, b0, i0, p) : 0.0;
        o[2] = i1 > 0 && v1 >= 0 ? la_sample(cols, kc, v1, a0, i1, p) : 0.0;
        o[3] = i0 > 0 && v1 >= 0 ? la_sample(cols, kc, v1, b0, i0, p) : 0.0;
        fl[lane] = (uint8_t)(RN_LABEL_GUARD | (i1 > 0 ? RN_LABEL_FOUND_CUR : 0) | (i0 > 0 ? RN_LABEL_FOUND_PREV : 0));
    }
}

// ---- outliers: one lane per tracklet (:2195-2231); del is cleared by the launcher
__device__ __forceinline__ bool la_jump(const double *__restrict__ a, const double *__restrict__ b) {
    return fabs(a[0] - b[0]) > 15.0 || (a[1] - b[1]) > 5.0;                     // :2221: np.abs(dy > 5) is the abs of a boolean
}

__global__ void __launch_bounds__(LA_THREADS) la_outliers_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                                 const int32_t *__restrict__ frame, int64_t T, int64_t R, int64_t F,
                                                                 int64_t n_visit, uint8_t *__restrict__ del, int32_t *status) {
    const int64_t t = (int64_t)blockIdx.x * LA_THREADS + threadIdx.x;
    if (t >= T) return;
    int64_t lo, hi;
    if (!la_rows(off, t, R, lo, hi)) {
        rn_flag(status, RN_LABEL_BAD_OFFSETS);
        return;
    }
    bool prev_deleted = false;
    int64_t f_before = -1;
    for (int64_t r = lo; r < hi; ++r) {
        const int64_t f = frame[r];
        if (f <= f_before || f >= F) {                                          // also f < 0
            rn_flag(status, RN_LABEL_BAD_FRAME);
            return;
        }
        if (f >= n_visit) return;                                               // :2197-2198: the walk has ended
        const double *cur = cols + r * 3;
        const double *prv = nullptr;
        if (f == 0) {                                                           // data[-1]: the last frame, not yet visited
            if ((int64_t)frame[hi - 1] == F - 1) prv = cols + (hi - 1) * 3;
        } else if (f_before == f - 1 && !prev_deleted) {
            prv = cols + (r - 1) * 3;
        }
        bool d = prv != nullptr && la_jump(cur, prv);
        if (!d && r + 1 < hi && f + 1 < F && (int64_t)frame[r + 1] == f + 1) d = la_jump(cur, cols + (r + 1) * 3);
        del[r] = d ? 1 : 0;
        prev_deleted = d;
        f_before = f;
    }
}

// ---- interpolation
struct LaWs {
    int32_t *row_pre;       // [R] missing frames before this row's gap, inside its tracklet
    int32_t *count;         // [T] missing frames of the tracklet
    int64_t *prefix;        // [T + 1]
};

__host__ __device__ static inline int64_t la_ws_layout(char *base, int64_t T, int64_t R, LaWs *w) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *r = base ? base + o : nullptr; o += (bytes + 15) & ~(int64_t)15; return r; };
    LaWs s;
    s.row_pre = reinterpret_cast<int32_t *>(take(R * 4));
    s.count = reinterpret_cast<int32_t *>(take(T * 4));
    s.prefix = reinterpret_cast<int64_t *>(take((T + 1) * 8));
    if (w) *w = s;
    return o;
}

extern "C" int64_t rn_label_interpolate_workspace_bytes(int64_t T, int64_t R) {
    if (T < 0 || R < 0 || T >= LA_MAX || R >= LA_MAX) return 0;
    return la_ws_layout(nullptr, T, R, nullptr);
}

__global__ void __launch_bounds__(LA_THREADS) la_gap_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ frame,
                                                            int64_t T, int64_t R, int64_t F, LaWs w, int32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * LA_WAVES + (threadIdx.x >> 6);      // wave-uniform
    if (t >= T) return;
    int64_t lo, hi;
    if (!la_rows(off, t, R, lo, hi)) {
        if (lane == 0) { rn_flag(status, RN_LABEL_BAD_OFFSETS); w.count[t] = 0; }
        return;
    }
    int carry = 0;
    for (int64_t base = lo; base < hi; base += RN_WAVE) {
        const int64_t r = base + lane;
        int g = 0;
        if (r + 1 < hi) {
            const int64_t f0 = frame[r], f1 = frame[r + 1];
            if (f0 < 0 || f1 <= f0 || f1 >= F) rn_flag(status, RN_LABEL_BAD_FRAME);
            else g = (int)(f1 - f0 - 1);
        }
        const int incl = wave_scan_incl(g);                                     // the waves leave on their own: no block scan
        if (r < hi) w.row_pre[r] = carry + incl - g;
        carry += __shfl(incl, RN_WAVE - 1, RN_WAVE);                            // every gap lies inside the F frames: no overflow
    }
    if (lane == 0) w.count[t] = carry;
}

// one workgroup walks the tracklets in chunks
__global__ void __launch_bounds__(LA_THREADS) la_prefix_kernel(int64_t T, int64_t U, LaWs w, int64_t *__restrict__ total,
                                                               int32_t *status) {
    __shared__ long long part[LA_WAVES];
    long long carry = 0;
    for (int64_t base = 0; base < T; base += LA_THREADS) {
        const int64_t t = base + threadIdx.x;
        const long long c = t < T ? (long long)w.count[t] : 0;
        long long sum;
        const long long incl = block_scan_incl<LA_WAVES>(c, part, sum);
        if (t < T) w.prefix[t] = carry + incl - c;
        carry += sum;
    }
    if (threadIdx.x == 0) {
        w.prefix[T] = carry;
        total[0] = carry;
        if (carry > U) rn_flag(status, RN_LABEL_BAD_PREFIX);                    // the fill leaves the rows beyond U out
    }
}

__global__ void __launch_bounds__(LA_THREADS) la_fill_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                             const int32_t *__restrict__ frame, const double *__restrict__ all_ts,
                                                             int64_t T, int64_t R, int64_t F, int C, int64_t U, LaWs w,
                                                             double *__restrict__ out, int32_t *__restrict__ out_src,
                                                             int32_t *__restrict__ out_frame, int32_t *status) {
    const int64_t u = (int64_t)blockIdx.x * LA_THREADS + threadIdx.x;
    if (u >= U || u >= w.prefix[T]) return;
    int64_t t = 0, t_hi = T;                                                    // the last t with prefix[t] <= u
    while (t_hi - t > 1) {
        const int64_t m = t + (t_hi - t) / 2;
        if (w.prefix[m] <= u) t = m; else t_hi = m;
    }
    const int64_t k = u - w.prefix[t];
    int64_t lo, hi;
    if (!la_rows(off, t, R, lo, hi) || hi - lo < 2 || k < 0 || k >= (int64_t)w.count[t]) {
        rn_flag(status, RN_LABEL_BAD_OFFSETS);
        return;
    }
    int64_t r = lo, r_hi = hi - 1;                                              // the last row with row_pre <= k that has a successor
    while (r_hi - r > 1) {
        const int64_t m = r + (r_hi - r) / 2;
        if ((int64_t)w.row_pre[m] <= k) r = m; else r_hi = m;
    }
    const int64_t f0 = frame[r], f1 = frame[r + 1], fi = f0 + 1 + (k - (int64_t)w.row_pre[r]);
    if (f0 < 0 || fi <= f0 || fi >= f1 || f1 >= F) {
        rn_flag(status, RN_LABEL_BAD_FRAME);
        return;
    }
    const int c = (int)(t % C);
    const double t1 = all_ts[f0 * C + c], t2 = all_ts[f1 * C + c], ti = all_ts[fi * C + c];   // :806-808
    const double p1 = (t2 - ti) / (t2 - t1);                                    // :809
    const double p2 = 1.0 - p1;                                                 // :810
    const double *a = cols + r * 3, *b = cols + (r + 1) * 3;
    out[u * 3] = p1 * a[0] + p2 * b[0];                                         // :814-815
    out[u * 3 + 1] = p1 * a[1] + p2 * b[1];
    out[u * 3 + 2] = ti;                                                        // :822
    out_src[u] = (int32_t)r;
    out_frame[u] = (int32_t)fi;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rn_label_pair_samples(const int64_t *offsets, const double *cols, int64_t R, int n_cam, int64_t n_ids, int key_col,
                                     int val0, int val1, uint8_t *flags, double *values, int32_t *status, void *stream) {
    if (R < 0 || R >= LA_MAX || n_cam < 0 || n_cam > RN_LABEL_MAX_CAMS || n_ids < 0 || n_ids >= LA_MAX || key_col < 0 ||
        key_col > 2 || val0 < 0 || val0 > 2 || val1 < -1 || val1 > 2 || !status)
        return RN_EINVAL;
    const int64_t entries = (int64_t)n_cam * (n_cam - 1) / 2 * n_ids;
    if (entries <= 0) return RN_OK;
    if (entries >= LA_MAX * LA_WAVES || !offsets || !cols || !flags || !values) return RN_EINVAL;
    hipLaunchKernelGGL(la_pair_kernel, dim3(rn_blocks(entries, LA_WAVES)), dim3(LA_THREADS), 0, (hipStream_t)stream, offsets, cols, R,
                       n_cam, n_ids, entries, key_col, val0, val1, flags, values, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_label_outliers(const int64_t *offsets, const double *cols, const int32_t *frame, int64_t T, int64_t R, int64_t F,
                                 int64_t n_visit, uint8_t *del, int32_t *status, void *stream) {
    if (T < 0 || R < 0 || F < 0 || T >= LA_MAX || R >= LA_MAX || F >= LA_MAX || n_visit < 0 || !status) return RN_EINVAL;
    if (R > 0) {
        if (!del) return RN_EINVAL;
        hipError_t e = hipMemsetAsync(del, 0, (size_t)R, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    if (T == 0) return RN_OK;
    if (!offsets || (R > 0 && (!cols || !frame))) return RN_EINVAL;
    hipLaunchKernelGGL(la_outliers_kernel, dim3(rn_blocks(T, LA_THREADS)), dim3(LA_THREADS), 0, (hipStream_t)stream, offsets, cols,
                       frame, T, R, F, n_visit, del, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_label_interpolate(const int64_t *offsets, const double *cols, const int32_t *frame, const double *all_ts,
                                    int64_t T, int64_t R, int64_t F, int n_cam, int64_t U, void *workspace, double *out,
                                    int32_t *out_src, int32_t *out_frame, int64_t *total, int32_t *status, void *stream) {
    if (T < 0 || R < 0 || F < 0 || U < 0 || T >= LA_MAX || R >= LA_MAX || F >= LA_MAX || U >= LA_MAX * LA_THREADS || n_cam <= 0 ||
        n_cam > RN_LABEL_MAX_CAMS || !total || !status)
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (U > 0) {
        if (!out_src) return RN_EINVAL;
        hipError_t e = hipMemsetAsync(out_src, 0xFF, (size_t)U * sizeof(int32_t), s);       // -1: a row that was left out
        if (e != hipSuccess) return (int)e;
    }
    if (T == 0) {
        hipError_t e = hipMemsetAsync(total, 0, sizeof(int64_t), s);
        return e != hipSuccess ? (int)e : RN_OK;
    }
    if (!offsets || !workspace || (R > 0 && (!cols || !frame)) || (U > 0 && (!all_ts || !out || !out_frame))) return RN_EINVAL;
    LaWs w;
    la_ws_layout(reinterpret_cast<char *>(workspace), T, R, &w);
    hipLaunchKernelGGL(la_gap_kernel, dim3(rn_blocks(T, LA_WAVES)), dim3(LA_THREADS), 0, s, offsets, frame, T, R, F, w, status);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(la_prefix_kernel, dim3(1), dim3(LA_THREADS), 0, s, T, U, w, total, status);
    RN_LAUNCH_CHECK();
    if (U > 0) {
        hipLaunchKernelGGL(la_fill_kernel, dim3(rn_blocks(U, LA_THREADS)), dim3(LA_THREADS), 0, s, offsets, cols, frame, all_ts, T, R,
                           F, n_cam, U, w, out, out_src, out_frame, status);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

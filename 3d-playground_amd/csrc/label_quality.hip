// The scores of a multi-camera label set, from the reference's later annotator (manual_annotator_state_v3.py):
//   calculate_total_variation (:3843-3889), calculate_feasibility (:3891-3979), the data half of plot_trajectories_unified
//   (:3634-3711, smooth = 1) and the reduction of annotator_rmse (:3981-4007).
//
// The reference collects, per object, the boxes of all cameras (camera outer, frame inner), sorts them by timestamp, drops a
// row that follows its predecessor by less than 0.01 s and differentiates what is left.  The input is the audit's CSR table
// (csrc/label_audit.hip): tracklet t = object * n_cam + camera, rows in ascending frame, so the rows of one object are
// contiguous and already in the reference's concatenation order.
//   lq_series_kernel      one workgroup per object.  (1) the optional lane filter lo < y < hi compacts the rows that survive
//                         (workgroup scan) into (fp64 key = timestamp, int32 index = position in the object's segment);
//                         (2) a bitonic network sorts them by (key, index), padded with +inf to a power of two: the index makes
//                         the order total, so the result is the stable sort by time whatever the network does; lq_sort is
//                         instantiated on LDS for an object of at most lds_rows rows and on a global workspace beyond;
//                         (3) keep[0] = 1, keep[i] = t[i] >= t[i-1] + 0.01 against the previous SORTED row (:3875-3878), a
//                         second scan compacts the m kept rows; (4) v, vy, a, theta on the kept rows; (5) m, max(x) - min(x),
//                         the count of feasible segments (order-free reductions) and the variation, summed in ascending order
//                         as Python's sum does: the workgroup stages 256 terms in LDS, one lane adds them.
//   lq_group_check_kernel one thread per row: the group ids ascend and lie inside the groups
//   lq_group_rmse_kernel  one workgroup per group of rows: im_pos = the mean of image corners 2 and 3, the group's mean of it,
//                         sqrt(sum(dx^2 + dy^2) / n), both sums in ascending row order through the same staged walk.
//
// Arithmetic: fp64, one rounding per operation in the reference's order (this file is in the Makefile's EXACT list: no fma
// contraction).  Only atan2 is not an IEEE operation: theta may differ from numpy's in its last bits.
//
// Every index read from memory is checked before use: an object's row range inside the R rows, a sorted index inside its
// segment, a group's row range inside the n rows.  A bad value sets a bit of *status and the item is left out or replaced by
// row 0 of its segment; it is never used as an index.  No kernel spins or asserts.
#include <math.h>

#include "common.h"
#include "wave_dev.h"

#define LQ_THREADS 256
#define LQ_WAVES (LQ_THREADS / RN_WAVE)
#define LQ_MAX ((int64_t)1 << 31)
#define LQ_PLANES 7                     // t, x, y, v, vy, a, theta

__device__ __forceinline__ int64_t lq_pow2(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// exclusive position of this thread's flag among the workgroup's; total = their number (workgroup-uniform).  part: LQ_WAVES ints.
__device__ __forceinline__ int lq_scan(int flag, int *part, int &total) {
    return block_scan_incl<LQ_WAVES>(flag, part, total) - flag;
}

// The sums of a(i) and b(i) over i < count in ascending order, started from 0.0, on every thread.  buf: 2 * LQ_THREADS doubles.
template <class F>
__device__ __forceinline__ void lq_serial_sum2(F term, int64_t count, double *buf, double &sa, double &sb) {
    double a = 0.0, b = 0.0;                                                    // thread 0's are the sums
    for (int64_t base = 0; base < count; base += LQ_THREADS) {
        const int64_t i = base + threadIdx.x;
        if (i < count) term(i, buf[threadIdx.x], buf[LQ_THREADS + threadIdx.x]);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int lim = (int)(count - base < LQ_THREADS ? count - base : LQ_THREADS);
            for (int k = 0; k < lim; ++k) {
                a += buf[k];
                b += buf[LQ_THREADS + k];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        buf[0] = a;
        buf[1] = b;
    }
    __syncthreads();
    sa = buf[0];
    sb = buf[1];
    __syncthreads();
}

// ascending by (key, index) over P = a power of two entries; ends behind a barrier
__device__ __forceinline__ void lq_sort(double *key, int *idx, int64_t P) {
    for (int64_t k = 2; k <= P; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t t = threadIdx.x; t < (P >> 1); t += LQ_THREADS) {
                const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;   // the pair (i, i ^ j), i below
                const double ka = key[i], kb = key[l];
                const int ia = idx[i], ib = idx[l];
                const bool after = ka > kb || (ka == kb && ia > ib);
                if (after == ((i & k) == 0)) {
                    key[i] = kb;
                    key[l] = ka;
                    idx[i] = ib;
                    idx[l] = ia;
                }
            }
            __syncthreads();
        }
    }
}

struct LqOut {
    int32_t *order;         // [R] the sorted rows of every object, -1 behind its n survivors
    uint8_t *keep;          // [R] the keep flag of every sorted row
    double *ser;            // [LQ_PLANES, R] the compacted series, 0.0 behind an object's m kept rows
    int32_t *counts;        // [n_ids, 3] n, m, feasible segments
    double *figs;           // [n_ids, 2] range, variation
};

// one object: rows [s0, s0 + L) of cols; key / idx hold lq_pow2(L) entries, in LDS or in global memory
__device__ __forceinline__ void lq_object(const double *__restrict__ cols, int64_t R, int64_t obj, int64_t s0, int64_t L, int lane_on,
                                          double lane_lo, double lane_hi, double *key, int *idx, int *part, double *buf,
                                          const LqOut &o, int32_t *status) {
    const int tid = threadIdx.x;
    double *st = o.ser + s0, *sx = st + R, *sy = sx + R, *sv = sy + R, *svy = sv + R, *sa = svy + R, *sth = sa + R;
    // (1) the rows the lane filter leaves, in segment order (:3645-3649)
    int64_t n = 0;
    for (int64_t base = 0; base < L; base += LQ_THREADS) {
        const int64_t i = base + tid;
        int f = 0;
        double t = 0.0;
        if (i < L) {
            const double *c = cols + (s0 + i) * 3;
            t = c[2];
            f = !lane_on || (c[1] > lane_lo && c[1] < lane_hi);
        }
        int tot;
        const int pos = lq_scan(f, part, tot);
        if (f) {
            key[n + pos] = t;
            idx[n + pos] = (int)i;
        }
        n += tot;
    }
    // (2) the sort
    const int64_t P = lq_pow2(n);
    for (int64_t i = n + tid; i < P; i += LQ_THREADS) {
        key[i] = INFINITY;
        idx[i] = RN_NO_INDEX;
    }
    __syncthreads();
    lq_sort(key, idx, P);
    // (3) order, keep flags, the kept rows
    int64_t m = 0;
    for (int64_t base = 0; base < n; base += LQ_THREADS) {
        const int64_t i = base + tid;
        int kp = 0;
        int64_t r = s0;
        double t = 0.0;
        if (i < n) {
            int64_t ii = idx[i];
            if (ii < 0 || ii >= L) {
                rn_flag(status, RN_LABEL_BAD_OFFSETS);
                ii = 0;
            }
            r = s0 + ii;
            t = key[i];
            kp = i == 0 || t >= key[i - 1] + 0.01;                              // :3877
            o.order[s0 + i] = (int32_t)r;
            o.keep[s0 + i] = (uint8_t)kp;
        }
        int tot;
        const int pos = lq_scan(kp, part, tot);
        if (kp) {
            st[m + pos] = t;
            sx[m + pos] = cols[r * 3];
            sy[m + pos] = cols[r * 3 + 1];
        }
        m += tot;
    }
    for (int64_t i = n + tid; i < L; i += LQ_THREADS) {
        o.order[s0 + i] = -1;
        o.keep[s0 + i] = 0;
    }
    __syncthreads();
    // (4) the series: v and vy on segment (k, k + 1), the last value repeated (:3943-3951), theta (:3958)
    for (int64_t k = tid; k < L; k += LQ_THREADS) {
        if (k >= m) {
            st[k] = sx[k] = sy[k] = sv[k] = svy[k] = sa[k] = sth[k] = 0.0;
            continue;
        }
        double v = 0.0, vy = 0.0;
        if (m > 1) {
            const int64_t q = k < m - 1 ? k : m - 2;
            const double dt = (st[q + 1] - st[q]) + 1e-08;
            v = -((sx[q + 1] - sx[q]) / dt);
            vy = (sy[q + 1] - sy[q]) / dt;
        }
        sv[k] = v;
        svy[k] = vy;
        sth[k] = atan2(vy, v) * 180.0 / 3.141592653589793;
    }
    __syncthreads();
    for (int64_t k = tid; k < m; k += LQ_THREADS) {                             // :3954-3956, on the negated and extended v
        double a = 0.0;
        if (m > 1) {
            const int64_t q = k < m - 1 ? k : m - 2;
            a = (sv[q + 1] - sv[q]) / ((st[q + 1] - st[q]) + 1e-08);
        }
        sa[k] = a;
    }
    // (5) the figures.  np.max(seg) < hi and np.min(seg) > lo is both ends inside, NaN failing either way (:3963, :3973);
    // the acceleration mask is numpy's `out=` there and does not enter (:3975)
    double mn = INFINITY, mx = -INFINITY;
    int feas = 0;
    for (int64_t k = tid; k < m; k += LQ_THREADS) {
        mn = fmin(mn, sx[k]);
        mx = fmax(mx, sx[k]);
        if (k < m - 1) {
            const double v0 = sv[k], v1 = sv[k + 1], h0 = sth[k], h1 = sth[k + 1];
            feas += v0 < 140.0 && v1 < 140.0 && v0 > 0.0 && v1 > 0.0 && h0 < 25.0 && h1 < 25.0 && h0 > -25.0 && h1 > -25.0;
        }
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    feas = wave_sum(feas);
    if ((tid & 63) == 0) {
        buf[tid >> 6] = mn;
        buf[LQ_WAVES + (tid >> 6)] = mx;
        part[tid >> 6] = feas;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < LQ_WAVES; ++k) {
            mn = fmin(mn, buf[k]);
            mx = fmax(mx, buf[LQ_WAVES + k]);
            feas += part[k];
        }
    }
    __syncthreads();
    double var, unused;
    lq_serial_sum2([&](int64_t i, double &a, double &b) { a = fabs(sx[i + 1] - sx[i]); b = 0.0; }, m > 1 ? m - 1 : 0, buf, var,
                   unused);                                                     // :3882
    if (tid == 0) {
        o.counts[obj * 3] = (int32_t)n;
        o.counts[obj * 3 + 1] = (int32_t)m;
        o.counts[obj * 3 + 2] = feas;
        o.figs[obj * 2] = m > 0 ? mx - mn : 0.0;                                // :3881
        o.figs[obj * 2 + 1] = var;
    }
}

extern "C" int64_t rn_label_series_workspace_bytes(int64_t R) {
    if (R < 0 || R >= LQ_MAX) return 0;
    return 2 * R * 8 + ((2 * R * 4 + 15) & ~(int64_t)15);                       // keys, then indices: lq_pow2(L) <= 2 L per object
}

__global__ void __launch_bounds__(LQ_THREADS) lq_series_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                               int64_t R, int C, int64_t N, int lane_on, double lane_lo,
                                                               double lane_hi, int lds_rows, double *ws_key, int *ws_idx, LqOut o,
                                                               int32_t *status) {
    extern __shared__ double lq_lds[];                                          // lds_rows keys, then lds_rows indices
    __shared__ int part[LQ_WAVES];
    __shared__ double buf[2 * LQ_THREADS];
    const int64_t obj = blockIdx.x;
    if (obj == 0 && threadIdx.x == 0 && (off[0] != 0 || off[N * C] != R)) rn_flag(status, RN_LABEL_BAD_OFFSETS);
    const int64_t s0 = off[obj * C], s1 = off[(obj + 1) * C];
    if (s0 < 0 || s0 > s1 || s1 > R) {                                          // workgroup-uniform
        if (threadIdx.x == 0) {
            rn_flag(status, RN_LABEL_BAD_OFFSETS);
            o.counts[obj * 3] = o.counts[obj * 3 + 1] = o.counts[obj * 3 + 2] = 0;
            o.figs[obj * 2] = o.figs[obj * 2 + 1] = 0.0;
        }
        return;
    }
    const int64_t L = s1 - s0;
    if (lq_pow2(L) <= lds_rows)
        lq_object(cols, R, obj, s0, L, lane_on, lane_lo, lane_hi, lq_lds, reinterpret_cast<int *>(lq_lds + lds_rows), part, buf, o,
                  status);
    else                                                                        // 2 s0 + lq_pow2(L) <= 2 s1: the objects' slices are apart
        lq_object(cols, R, obj, s0, L, lane_on, lane_lo, lane_hi, ws_key + 2 * s0, ws_idx + 2 * s0, part, buf, o, status);
}

// ---- annotator_rmse: the rows of group g are those with group[r] == g, contiguous because the ids ascend
__global__ void __launch_bounds__(LQ_THREADS) lq_group_check_kernel(const int32_t *__restrict__ group, int64_t n, int64_t G,
                                                                    int32_t *status) {
    const int64_t r = (int64_t)blockIdx.x * LQ_THREADS + threadIdx.x;
    if (r >= n) return;
    const int64_t g = group[r];
    if (g < 0 || g >= G || (r > 0 && (int64_t)group[r - 1] > g)) rn_flag(status, RN_LABEL_BAD_GROUP);
}

// the first row in [0, n] whose group is not below g
__device__ __forceinline__ int64_t lq_lower(const int32_t *__restrict__ group, int64_t n, int64_t g) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)group[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(LQ_THREADS) lq_group_rmse_kernel(const double *__restrict__ im, const int32_t *__restrict__ group,
                                                                   int64_t n, double *__restrict__ rmse, double *__restrict__ mean,
                                                                   int32_t *__restrict__ count) {
    __shared__ double buf[2 * LQ_THREADS];
    const int64_t g = blockIdx.x;
    const int64_t lo = lq_lower(group, n, g), hi = lq_lower(group, n, g + 1);   // both inside [0, n], workgroup-uniform
    const int64_t cnt = hi - lo;
    if (cnt <= 0) {                                                             // an empty group (or ids out of order: flagged)
        if (threadIdx.x == 0) {
            rmse[g] = mean[g * 2] = mean[g * 2 + 1] = NAN;
            count[g] = 0;
        }
        return;
    }
    auto pos = [&](int64_t i, double &px, double &py) {                         // :3997: the mean of corners 2 and 3
        const double *c = im + (lo + i) * 16;
        px = (c[4] + c[6]) / 2.0;
        py = (c[5] + c[7]) / 2.0;
    };
    double sx, sy, ss, unused;
    lq_serial_sum2(pos, cnt, buf, sx, sy);
    const double mx = sx / (double)cnt, my = sy / (double)cnt;                  // :3998
    lq_serial_sum2([&](int64_t i, double &a, double &b) {
        double px, py;
        pos(i, px, py);
        const double dx = px - mx, dy = py - my;
        a = dx * dx + dy * dy;                                                  // :4000
        b = 0.0;
    }, cnt, buf, ss, unused);
    if (threadIdx.x == 0) {
        rmse[g] = sqrt(ss / (double)cnt);
        mean[g * 2] = mx;
        mean[g * 2 + 1] = my;
        count[g] = (int32_t)cnt;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rn_label_series(const int64_t *offsets, const double *cols, int64_t R, int n_cam, int64_t n_ids, int lane_on,
                               double lane_lo, double lane_hi, int lds_rows, void *workspace, int32_t *order, uint8_t *keep,
                               double *series, int32_t *counts, double *figs, int32_t *status, void *stream) {
    if (R < 0 || R >= LQ_MAX || n_cam <= 0 || n_cam > RN_LABEL_MAX_CAMS || n_ids < 0 || n_ids >= LQ_MAX || lds_rows < 2 ||
        lds_rows > RN_LABEL_SERIES_MAX_LDS_ROWS || (lds_rows & (lds_rows - 1)) || !status)
        return RN_EINVAL;
    if (n_ids == 0) return RN_OK;
    if (!offsets || !counts || !figs || (R > 0 && (!cols || !workspace || !order || !keep || !series))) return RN_EINVAL;
    LqOut o;
    o.order = order;
    o.keep = keep;
    o.ser = series;
    o.counts = counts;
    o.figs = figs;
    double *ws_key = reinterpret_cast<double *>(workspace);
    int *ws_idx = reinterpret_cast<int *>(ws_key + 2 * R);
    hipLaunchKernelGGL(lq_series_kernel, dim3((unsigned)n_ids), dim3(LQ_THREADS), (size_t)lds_rows * 12, (hipStream_t)stream, offsets,
                       cols, R, n_cam, n_ids, lane_on ? 1 : 0, lane_lo, lane_hi, lds_rows, ws_key, ws_idx, o, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_label_group_rmse(const double *im, const int32_t *group, int64_t n, int64_t n_groups, double *rmse, double *mean,
                                   int32_t *count, int32_t *status, void *stream) {
    if (n < 0 || n >= LQ_MAX || n_groups < 0 || n_groups >= LQ_MAX || !status) return RN_EINVAL;
    if (n_groups == 0) return RN_OK;
    if (!rmse || !mean || !count || (n > 0 && (!im || !group))) return RN_EINVAL;
    if (n > 0) {
        hipLaunchKernelGGL(lq_group_check_kernel, dim3(rn_blocks(n, LQ_THREADS)), dim3(LQ_THREADS), 0, (hipStream_t)stream, group, n,
                           n_groups, status);
        RN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lq_group_rmse_kernel, dim3((unsigned)n_groups), dim3(LQ_THREADS), 0, (hipStream_t)stream, im, group, n, rmse,
                       mean, count);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

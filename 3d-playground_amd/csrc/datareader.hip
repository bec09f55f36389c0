// Data_Reader.reinterpolate / write_to_file (datareader.py:401-451 / 453-584) for all rows of a tracking CSV at once.
//
// The reference resamples every track with a Python double loop over instants and ids (:411-434) and rewrites the file with
// two single-box homography calls per row (:530-550).  Here the serial walk over instants (:406-444: which frame pair
// (a, a + 1) an instant falls in, the accumulated output_time) stays on the host, bit-equal by construction, and everything
// proportional to rows runs here:
//   rn_reinterp_mate     per input row, the row of the NEXT frame with the same id (:416-417); a property of the input only
//   rn_reinterp_offsets  per instant, how many rows of its frame a are mated, and the exclusive prefix (int64)
//   rn_reinterp_rows     per instant, the mated rows compacted in the frame's own order and interpolated (:422-427)
//   rn_track_rows        per row, fp32 state, keep = state[0] != 0, space corners, image corners, 2D box (:530-550)
//
// Arithmetic: fp64, one rounding per operation (this file is in the Makefile's EXACT list: no fma contraction), so the
// interpolation rounds like Python's floats; the state is rounded to fp32 as torch.tensor([...]) does; corners and the
// projection are state_corners / hg_project_to_im of homography_dev.h, i.e. the values of rn_state_to_im.
//
// Every index read from memory is checked before use (frame offsets monotone and inside the row count, a + 1 below the frame
// count, mates inside the next frame, destinations inside the prefix slot, mat_index below the matrix count).  A bad value
// sets a bit of *status and the item is left out; it is never used as an index.
#include "common.h"
#include "homography_dev.h"
#include "wave_dev.h"

#define DR_THREADS 256
#define DR_WAVES (DR_THREADS / RN_WAVE)

// rows [lo, hi) of frame f; the caller guarantees 0 <= f < F (offsets holds F + 1 entries)
__device__ __forceinline__ bool dr_frame(const int64_t *__restrict__ off, int64_t f, int64_t R, int64_t &lo, int64_t &hi) {
    lo = off[f];
    hi = off[f + 1];
    return lo >= 0 && lo <= hi && hi <= R;
}

// ---- mates: one workgroup per frame pair (f, f + 1); the next frame's ids pass through LDS in tiles of RN_REINTERP_TILE
__global__ void __launch_bounds__(DR_THREADS) dr_mate_kernel(const int64_t *__restrict__ off, const int64_t *__restrict__ ids,
                                                             int64_t R, int32_t *__restrict__ mate, int32_t *status) {
    __shared__ int64_t tile[RN_REINTERP_TILE];
    const int64_t f = blockIdx.x;
    int64_t a0, a1, b0, b1;
    const bool ok_a = dr_frame(off, f, R, a0, a1), ok_b = dr_frame(off, f + 1, R, b0, b1);
    if (!ok_a || !ok_b) {                                                       // uniform over the workgroup
        if (threadIdx.x == 0) rn_flag(status, RN_REINTERP_BAD_OFFSETS);
        return;
    }
    for (int64_t t0 = b0; t0 < b1; t0 += RN_REINTERP_TILE) {
        const int n = (int)((b1 - t0) < (int64_t)RN_REINTERP_TILE ? (b1 - t0) : (int64_t)RN_REINTERP_TILE);
        __syncthreads();                                                        // the tile before is done with
        for (int k = threadIdx.x; k < n; k += DR_THREADS) tile[k] = ids[t0 + k];
        __syncthreads();
        for (int64_t r = a0 + threadIdx.x; r < a1; r += DR_THREADS) {
            if (mate[r] >= 0) continue;                                         // found in an earlier tile (this lane wrote it)
            const int64_t id = ids[r];
            for (int k = 0; k < n; ++k)
                if (tile[k] == id) { mate[r] = (int32_t)(t0 + k); break; }
        }
    }
}

// a row is mated when its mate lies in the next frame's rows [b0, b1); any other non-negative value is a bad input
__device__ __forceinline__ bool dr_mated(int32_t m, int64_t b0, int64_t b1, int32_t *status) {
    if (m < 0) return false;
    if ((int64_t)m >= b0 && (int64_t)m < b1) return true;
    rn_flag(status, RN_REINTERP_BAD_MATE);
    return false;
}

// ---- mated rows per frame: one workgroup per frame
__global__ void __launch_bounds__(DR_THREADS) dr_frame_count_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ mate,
                                                                    int64_t F, int64_t R, int32_t *__restrict__ frame_count,
                                                                    int32_t *status) {
    __shared__ int part[DR_WAVES];
    const int64_t f = blockIdx.x;
    int n = 0;
    if (f + 1 < F) {
        int64_t a0, a1, b0, b1;
        const bool ok_a = dr_frame(off, f, R, a0, a1), ok_b = dr_frame(off, f + 1, R, b0, b1);
        if (!ok_a || !ok_b) {
            if (threadIdx.x == 0) rn_flag(status, RN_REINTERP_BAD_OFFSETS);
        } else {
            for (int64_t r = a0 + threadIdx.x; r < a1; r += DR_THREADS) n += dr_mated(mate[r], b0, b1, status) ? 1 : 0;
        }
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < DR_WAVES; ++k) s += part[k];
        frame_count[f] = s;
    }
}

// ---- per instant: the count of its frame a, and the exclusive prefix.  One workgroup walks the instants in chunks.
__global__ void __launch_bounds__(DR_THREADS) dr_prefix_kernel(const int32_t *__restrict__ frame_count, const int32_t *__restrict__ inst_a,
                                                               int64_t F, int64_t T, int32_t *__restrict__ count,
                                                               int64_t *__restrict__ prefix, int32_t *status) {
    __shared__ long long part[DR_WAVES];
    int64_t carry = 0;
    for (int64_t base = 0; base < T; base += DR_THREADS) {
        const int64_t t = base + threadIdx.x;
        int c = 0;
        if (t < T) {
            const int64_t a = inst_a[t];
            if (a < 0 || a + 1 >= F) rn_flag(status, RN_REINTERP_BAD_PAIR);
            else c = frame_count[a];
            if (c < 0) c = 0;
            count[t] = c;
        }
        long long total;
        const long long incl = block_scan_incl<DR_WAVES, long long>(c, part, total);    // 256 frame counts can pass 2^31
        if (t < T) prefix[t] = carry + (int64_t)(incl - c);
        carry += (int64_t)total;
    }
    if (threadIdx.x == 0) prefix[T] = carry;
}

// ---- rows: one workgroup per instant; ordered compaction of the mated rows of frame a, then the interpolation
__global__ void __launch_bounds__(DR_THREADS) dr_rows_kernel(const int64_t *__restrict__ off, const double *__restrict__ frame_ts,
                                                             const double *__restrict__ fields, const int32_t *__restrict__ mate,
                                                             const int32_t *__restrict__ inst_a, const double *__restrict__ inst_time,
                                                             const int64_t *__restrict__ prefix, int64_t F, int64_t R, int64_t U,
                                                             double *__restrict__ out_fields, int32_t *__restrict__ out_src,
                                                             int32_t *__restrict__ out_inst, int32_t *status) {
    __shared__ int part[DR_WAVES];
    const int64_t t = blockIdx.x;
    const int64_t a = inst_a[t];
    if (a < 0 || a + 1 >= F) {                                                  // every exit below is uniform over the workgroup
        if (threadIdx.x == 0) rn_flag(status, RN_REINTERP_BAD_PAIR);
        return;
    }
    int64_t a0, a1, b0, b1;
    const bool ok_a = dr_frame(off, a, R, a0, a1), ok_b = dr_frame(off, a + 1, R, b0, b1);
    if (!ok_a || !ok_b) {
        if (threadIdx.x == 0) rn_flag(status, RN_REINTERP_BAD_OFFSETS);
        return;
    }
    const int64_t p0 = prefix[t], p1 = prefix[t + 1];
    if (p0 < 0 || p1 < p0 || p1 > U) {
        if (threadIdx.x == 0) rn_flag(status, RN_REINTERP_BAD_PREFIX);
        return;
    }
    const double ts = frame_ts[a], next_ts = frame_ts[a + 1], out_t = inst_time[t];
    const double r1 = (out_t - ts) / (next_ts - ts);                            // datareader.py:422
    const double r2 = 1.0 - r1;                                                 // :423
    int64_t carry = 0;
    for (int64_t base = a0; base < a1; base += DR_THREADS) {
        const int64_t r = base + threadIdx.x;
        int32_t m = -1;
        bool on = false;
        if (r < a1) {
            m = mate[r];
            on = dr_mated(m, b0, b1, status);
        }
        int total;
        const int incl = block_scan_incl<DR_WAVES>(on ? 1 : 0, part, total);
        if (on) {
            const int64_t dst = p0 + carry + (int64_t)(incl - 1);
            if (dst < p1) {
                const double *cur = fields + r * 6, *nxt = fields + (int64_t)m * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) out_fields[dst * 6 + k] = cur[k] * r1 + nxt[k] * r2;     // :427, as written
                out_src[dst] = (int32_t)r;
                out_inst[dst] = (int32_t)t;
            } else {
                rn_flag(status, RN_REINTERP_BAD_PREFIX);
            }
        }
        carry += total;
    }
}

// ---- write_to_file's per-row arithmetic, one lane per row
__device__ __forceinline__ double dr_min(double m, double v) { return (v < m || v != v) ? v : m; }   // torch.min: NaN wins
__device__ __forceinline__ double dr_max(double m, double v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(DR_THREADS) dr_track_rows_kernel(const double *__restrict__ fields, const double *__restrict__ direction,
                                                                   const int32_t *__restrict__ mat_index, const double *__restrict__ P,
                                                                   const double *__restrict__ P2, int64_t n_mats, int64_t N,
                                                                   float *__restrict__ state, float *__restrict__ space,
                                                                   double *__restrict__ im, double *__restrict__ box,
                                                                   uint8_t *__restrict__ keep, int32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * DR_THREADS + threadIdx.x;
    if (i >= N) return;
    const double *f = fields + i * 6;                                           // x, y, l, w, h, v
    float s[7];
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = (float)f[k];                             // :530-533: one rounding, fp64 -> fp32
    s[5] = (float)direction[i];
    s[6] = (float)f[5];
#pragma unroll
    for (int k = 0; k < 7; ++k) state[i * 7 + k] = s[k];
    const int32_t m = mat_index ? mat_index[i] : 0;
    float *sp = space + i * 8;
    double *o = im + i * 16, *b = box + i * 4;
    if (m < 0 || (int64_t)m >= n_mats) {
        rn_flag(status, RN_REINTERP_BAD_MAT_INDEX);
        keep[i] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) sp[k] = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = 0.0;
        return;
    }
    keep[i] = s[0] != 0.f ? 1 : 0;                                              // :535, on the fp32 value
    float x[8], y[8], z[8];
    state_corners(s, x, y, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) { sp[2 * k] = x[k]; sp[2 * k + 1] = y[k]; }     // :539
    double2 pt[8];
    hg_project_to_im(x, y, z, P, P2, m, pt);                                    // :543
    double x0 = pt[0].x, y0 = pt[0].y, x1 = pt[0].x, y1 = pt[0].y;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        o[2 * k] = pt[k].x;
        o[2 * k + 1] = pt[k].y;
        if (k) { x0 = dr_min(x0, pt[k].x); y0 = dr_min(y0, pt[k].y); x1 = dr_max(x1, pt[k].x); y1 = dr_max(y1, pt[k].y); }
    }
    b[0] = x0; b[1] = y0; b[2] = x1; b[3] = y1;                                 // :547-550
}

// ------------------------------------------------------------------------------------------------ entry points
#define DR_MAX_ROWS ((int64_t)1 << 31)

extern "C" int rn_reinterp_mate(const int64_t *offsets, const int64_t *ids, int64_t F, int64_t R, int32_t *mate,
                                int32_t *status, void *stream) {
    if (F < 0 || R < 0 || R >= DR_MAX_ROWS || F >= DR_MAX_ROWS) return RN_EINVAL;
    if (R > 0) {
        hipError_t e = hipMemsetAsync(mate, 0xFF, (size_t)R * sizeof(int32_t), (hipStream_t)stream);     // -1: no mate
        if (e != hipSuccess) return (int)e;
    }
    if (F >= 2) {
        hipLaunchKernelGGL(dr_mate_kernel, dim3((unsigned)(F - 1)), dim3(DR_THREADS), 0, (hipStream_t)stream, offsets, ids, R, mate,
                           status);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

extern "C" int rn_reinterp_offsets(const int64_t *offsets, const int32_t *mate, int64_t F, int64_t R, const int32_t *inst_a,
                                   int64_t T, int32_t *frame_count, int32_t *count, int64_t *prefix, int32_t *status,
                                   void *stream) {
    if (F < 0 || R < 0 || T < 0 || R >= DR_MAX_ROWS || F >= DR_MAX_ROWS || T >= DR_MAX_ROWS) return RN_EINVAL;
    if (F > 0) {
        hipLaunchKernelGGL(dr_frame_count_kernel, dim3((unsigned)F), dim3(DR_THREADS), 0, (hipStream_t)stream, offsets, mate, F, R,
                           frame_count, status);
        RN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(dr_prefix_kernel, dim3(1), dim3(DR_THREADS), 0, (hipStream_t)stream, frame_count, inst_a, F, T, count, prefix,
                       status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_reinterp_rows(const int64_t *offsets, const double *frame_ts, const double *fields, const int32_t *mate,
                                const int32_t *inst_a, const double *inst_time, const int64_t *prefix, int64_t F, int64_t R,
                                int64_t T, int64_t U, double *out_fields, int32_t *out_src, int32_t *out_inst, int32_t *status,
                                void *stream) {
    if (F < 0 || R < 0 || T < 0 || U < 0 || R >= DR_MAX_ROWS || F >= DR_MAX_ROWS || T >= DR_MAX_ROWS) return RN_EINVAL;
    if (T > 0) {
        hipLaunchKernelGGL(dr_rows_kernel, dim3((unsigned)T), dim3(DR_THREADS), 0, (hipStream_t)stream, offsets, frame_ts, fields, mate,
                           inst_a, inst_time, prefix, F, R, U, out_fields, out_src, out_inst, status);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

extern "C" int rn_track_rows(const double *fields, const double *direction, const int32_t *mat_index, const double *P,
                             const double *P2, int64_t n_mats, int64_t N, float *state, float *space, double *im, double *box,
                             uint8_t *keep, int32_t *status, void *stream) {
    if (N < 0 || n_mats < 1 || N >= DR_MAX_ROWS * DR_THREADS) return RN_EINVAL;
    if (N > 0) {
        hipLaunchKernelGGL(dr_track_rows_kernel, dim3(rn_blocks(N, DR_THREADS)), dim3(DR_THREADS), 0, (hipStream_t)stream, fields,
                           direction, mat_index, P, P2, n_mats, N, state, space, im, box, keep, status);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

// Traffic state from tracking output (traffic_state.py): Edie's generalised flow, density and space-mean speed per lane over a
// space-time grid, and for every vehicle at every instant its leader, space gap, time headway and time to collision.  This goes
// beyond the reference; tests/traffic_cases.py is the plain restatement of every rule.
//
// A tracklet is all rows of one id, in time order; the host packs offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v) and
// direction int32 [R] (track_stitch.pack_tracklets).
//   rn_traffic_lanes     one thread per tracklet for its direction, then one thread per packed row for the row's lane
//   rn_traffic_cells     one thread per segment (two consecutive rows of a tracklet): the segment is cut at every grid line it
//                        crosses and each piece adds its time and its distance, in units of 2^-20, to one cell by 64-bit integer
//                        atomics -- integer sums do not depend on the order they land in, so the fields equal the restatement bit
//                        for bit without a sort or a second pass
//   rn_traffic_leaders   one workgroup per frame: the frame's rows staged in LDS in tiles of 256, one thread per row
//
// Arithmetic: fp64, one rounding per operation (this file is in the Makefile's EXACT list: no fma contraction).
//
// Every index read from memory is checked before use; a refused row or segment sets a bit of *status and is left out.  No thread
// of the cells kernel leaves before its end: the counters are summed over the wave first.
#include "common.h"
#include "wave_dev.h"

#define TF_THREADS 256
#define TF_NONE 2.0                                                             // "no cut pending": every real cut is below 1

// the first k with e[k] <= y < e[k+1], else -1
__device__ __forceinline__ int tf_lane_of(const double *__restrict__ e, int n, double y) {
    int k = -1;
    for (int q = 0; q + 1 < n; ++q)
        if (k < 0 && e[q] <= y && y < e[q + 1]) k = q;
    return k;
}

// the largest i in 0 .. N-1 with off[i] <= r (N >= 1); the caller checks off[i] <= r < off[i+1]
__device__ __forceinline__ int64_t tf_tracklet_of(const int64_t *__restrict__ off, int64_t N, int64_t r) {
    int64_t lo = 0, hi = N - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool tf_finite(double v) { return fabs(v) < INFINITY; }   // false for a NaN

// the wave's sum of a per-thread count, added once per wave
__device__ __forceinline__ void tf_count(int64_t *counter, int v) {
    v = wave_sum(v);
    if ((threadIdx.x & (RN_WAVE - 1)) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long *>(counter), (unsigned long long)v);
}

// ------------------------------------------------------------------------------------------------ lanes
__global__ void __launch_bounds__(TF_THREADS) tf_dir_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ direction, int64_t N,
                                                             int64_t R, int32_t *__restrict__ dir, int32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (i >= N) return;
    const int64_t lo = off[i], hi = off[i + 1];
    if (lo < 0 || hi < lo || hi > R || (i == 0 && lo != 0) || (i == N - 1 && hi != R)) { rn_flag(status, RN_TRAFFIC_BAD_OFFSETS); dir[i] = 1; return; }
    int64_t dsum = 0;
    for (int64_t r = lo; r < hi; ++r) dsum += direction[r];
    dir[i] = dsum >= 0 ? 1 : -1;
}

__global__ void __launch_bounds__(TF_THREADS) tf_lane_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                              const int32_t *__restrict__ dir, const double *__restrict__ ep, int n_pos,
                                                              const double *__restrict__ en, int n_neg, int64_t N, int64_t R,
                                                              int32_t *__restrict__ lane, int32_t *status) {
    const int64_t r = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (r >= R) return;
    lane[r] = -1;
    const double *c = cols + r * 7;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 7; ++q) ok = ok && tf_finite(c[q]);
    if (!ok) { rn_flag(status, RN_TRAFFIC_NONFINITE); return; }
    const int64_t i = tf_tracklet_of(off, N, r);
    if (r < off[i] || r >= off[i + 1]) { rn_flag(status, RN_TRAFFIC_BAD_OFFSETS); return; }
    lane[r] = dir[i] >= 0 ? tf_lane_of(ep, n_pos, c[2]) : tf_lane_of(en, n_neg, c[2]);
}

// ------------------------------------------------------------------------------------------------ cells
// Consecutive segments of a tracklet mostly hit the same cell.  Adding the pieces of neighbouring lanes up over the wave first (a
// segmented suffix sum over runs of equal cells, one atomic per run) was built and measured: no gain at 212 400 segments into 10 425
// cells (profiles/traffic_state.txt), so every piece issues its own atomics.
__global__ void __launch_bounds__(TF_THREADS) tf_cells_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                               const int32_t *__restrict__ dir, const double *__restrict__ ep, int n_pos,
                                                               const double *__restrict__ en, int n_neg, int64_t N, int64_t R, double t0,
                                                               double dt, int64_t nt, double x0, double dx, int64_t nx, double max_gap,
                                                               int64_t L, int64_t *__restrict__ T, int64_t *__restrict__ D,
                                                               int32_t *__restrict__ cnt, int64_t *__restrict__ counters, int32_t *status) {
    const int64_t r = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    const double Q = (double)RN_TRAFFIC_Q, LIMIT = 1099511627776.0;             // 2^40
    int c_seg = 0, c_used = 0, c_gap = 0, c_lane = 0, c_pieces = 0, c_out = 0;
    bool more = false;
    double ta = 0.0, xa = 0.0, Tt = 0.0, X = 0.0, ka = 0.0, ma = 0.0;
    int nk = 0, nm = 0;
    int64_t base = 0;
    if (r < R) {
        const int64_t i = tf_tracklet_of(off, N, r);
        const int64_t hi = off[i + 1];
        if (r < off[i] || r >= hi || hi > R) {                                  // hi > R: row r + 1 may not exist
            rn_flag(status, RN_TRAFFIC_BAD_OFFSETS);
        } else if (r + 1 < hi) {                                                // a tracklet's last row starts no segment
            c_seg = 1;
            const double *a = cols + r * 7, *b = a + 7;
            const double tb = b[0], xb = b[1], ya = a[2], yb = b[2];
            ta = a[0];
            xa = a[1];
            const int d = dir[i];
            if (!(tf_finite(ta) && tf_finite(xa) && tf_finite(ya) && tf_finite(tb) && tf_finite(xb) && tf_finite(yb))) {
                rn_flag(status, RN_TRAFFIC_NONFINITE);
            } else if (d != 1 && d != -1) {
                rn_flag(status, RN_TRAFFIC_BAD_DIR);
            } else {
                Tt = tb - ta;
                X = xb - xa;
                if (!(Tt > 0.0 && Tt <= max_gap)) {
                    c_gap = 1;
                } else {
                    const double ym = (ya + yb) * 0.5;
                    const int ln = d > 0 ? tf_lane_of(ep, n_pos, ym) : tf_lane_of(en, n_neg, ym);
                    if (ln < 0) {
                        c_lane = 1;
                    } else if (!(Tt * Q < LIMIT && fabs(X) * Q < LIMIT)) {
                        rn_flag(status, RN_TRAFFIC_RANGE);
                    } else {
                        ka = floor((ta - t0) / dt);
                        const double kb = floor((tb - t0) / dt);
                        ma = floor((fmin(xa, xb) - x0) / dx);
                        const double mb = floor((fmax(xa, xb) - x0) / dx);
                        if (!((kb - ka) + (mb - ma) <= (double)RN_TRAFFIC_MAX_CUTS)) {   // also a NaN of inf - inf
                            rn_flag(status, RN_TRAFFIC_TOO_MANY_CUTS);
                        } else {
                            nk = (int)(kb - ka);
                            nm = (int)(mb - ma);
                            base = ((d > 0 ? 0 : L) + ln) * nt * nx;
                            c_used = 1;
                            more = true;
                        }
                    }
                }
            }
        }
    }
    // both cut lists ascend in s: the time cuts in k, the x cuts in m when X > 0 and against m when X < 0
    double u = 0.0, st = TF_NONE, sx = TF_NONE;
    int ik = 0, im = 0;
    while (more) {
        while (st == TF_NONE && ik < nk) {
            const double s = ((t0 + (ka + (double)(ik + 1)) * dt) - ta) / Tt;
            ++ik;
            if (s > 0.0 && s < 1.0) st = s;
        }
        while (sx == TF_NONE && im < nm) {
            const double m = ma + (double)(X > 0.0 ? im + 1 : nm - im);
            const double s = ((x0 + m * dx) - xa) / X;
            ++im;
            if (s > 0.0 && s < 1.0) sx = s;
        }
        double v = 1.0;
        if (st == TF_NONE && sx == TF_NONE) more = false;
        else if (st <= sx) { v = st; st = TF_NONE; }
        else { v = sx; sx = TF_NONE; }
        if (!(v > u)) continue;                                                 // a time cut and an x cut at the same s
        const double sm = (u + v) * 0.5;
        const double ft = floor(((ta + sm * Tt) - t0) / dt), fx = floor(((xa + sm * X) - x0) / dx);
        ++c_pieces;
        if (!(ft >= 0.0 && ft < (double)nt && fx >= 0.0 && fx < (double)nx)) {
            ++c_out;
        } else {
            const int64_t key = base + (int64_t)ft * nx + (int64_t)fx;
            atomicAdd(reinterpret_cast<unsigned long long *>(T + key), (unsigned long long)(int64_t)rint(((v - u) * Tt) * Q));
            atomicAdd(reinterpret_cast<unsigned long long *>(D + key), (unsigned long long)(int64_t)rint(((v - u) * fabs(X)) * Q));
            atomicAdd(cnt + key, 1);
        }
        u = v;
    }
    tf_count(counters + 0, c_seg);
    tf_count(counters + 1, c_used);
    tf_count(counters + 2, c_gap);
    tf_count(counters + 3, c_lane);
    tf_count(counters + 4, c_pieces);
    tf_count(counters + 5, c_out);
}

// ------------------------------------------------------------------------------------------------ leaders
struct TfRow { double x, l, v; int32_t dir, lane, trk, row; };

// entry q of frame_rows, checked: lane -2 (never a candidate, never searched for) when the row cannot be used
__device__ __forceinline__ TfRow tf_row(const int64_t *__restrict__ off, const double *__restrict__ cols, const int32_t *__restrict__ dir,
                                        const int32_t *__restrict__ lane, const int32_t *__restrict__ frame_rows, int64_t q, int64_t N, int64_t R,
                                        int32_t *status) {
    TfRow w = {0.0, 0.0, 0.0, 0, -2, -1, -1};
    const int64_t r = frame_rows[q];
    if (r < 0 || r >= R) { rn_flag(status, RN_TRAFFIC_BAD_FRAME); return w; }
    const int64_t i = tf_tracklet_of(off, N, r);
    if (r < off[i] || r >= off[i + 1]) { rn_flag(status, RN_TRAFFIC_BAD_OFFSETS); return w; }
    const double *c = cols + r * 7;
    if (!(tf_finite(c[1]) && tf_finite(c[3]) && tf_finite(c[6]))) { rn_flag(status, RN_TRAFFIC_NONFINITE); return w; }
    w.x = c[1]; w.l = c[3]; w.v = c[6];
    w.dir = dir[i]; w.lane = lane[r]; w.trk = (int32_t)i; w.row = (int32_t)r;
    return w;
}

__global__ void __launch_bounds__(TF_THREADS) tf_leaders_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                                 const int32_t *__restrict__ dir, const int32_t *__restrict__ lane,
                                                                 const int64_t *__restrict__ frame_off, const int32_t *__restrict__ frame_rows,
                                                                 int64_t N, int64_t R, int64_t Rf, int32_t *__restrict__ leader,
                                                                 double *__restrict__ spacing, double *__restrict__ gap,
                                                                 double *__restrict__ headway, double *__restrict__ ttc,
                                                                 int64_t *__restrict__ counters, int32_t *status) {
    __shared__ double s_x[TF_THREADS], s_v[TF_THREADS];
    __shared__ int32_t s_dir[TF_THREADS], s_lane[TF_THREADS], s_trk[TF_THREADS], s_row[TF_THREADS];
    const int64_t lo = frame_off[blockIdx.x], hi = frame_off[blockIdx.x + 1];
    if (lo < 0 || hi < lo || hi > Rf) {                                         // the same for the whole workgroup
        if (threadIdx.x == 0) rn_flag(status, RN_TRAFFIC_BAD_FRAME);
        return;
    }
    const int64_t n = hi - lo;
    int c_lead = 0, c_over = 0;
    for (int64_t own = 0; own < n; own += TF_THREADS) {                         // the rows this pass searches for
        const bool mine = own + threadIdx.x < n;
        TfRow me = {0.0, 0.0, 0.0, 0, -2, -1, -1};
        if (mine) me = tf_row(off, cols, dir, lane, frame_rows, lo + own + threadIdx.x, N, R, status);
        const double sgn = (double)me.dir;
        double bs = INFINITY, bv = 0.0;
        int32_t bt = RN_NO_INDEX, br = -1;
        for (int64_t tile = 0; tile < n; tile += TF_THREADS) {
            __syncthreads();                                                    // the readers of the tile before are done
            if (tile + threadIdx.x < n) {
                const TfRow w = tile == own ? me : tf_row(off, cols, dir, lane, frame_rows, lo + tile + threadIdx.x, N, R, status);
                s_x[threadIdx.x] = w.x; s_v[threadIdx.x] = w.v;
                s_dir[threadIdx.x] = w.dir; s_lane[threadIdx.x] = w.lane; s_trk[threadIdx.x] = w.trk; s_row[threadIdx.x] = w.row;
            }
            __syncthreads();
            const int m = (int)(n - tile < TF_THREADS ? n - tile : TF_THREADS);
            if (me.lane >= 0) {
                for (int j = 0; j < m; ++j) {
                    if (s_row[j] == me.row || s_dir[j] != me.dir || s_lane[j] != me.lane) continue;
                    const double s = sgn * (s_x[j] - me.x);
                    if (!(s > 0.0)) continue;
                    const int32_t tj = s_trk[j], rj = s_row[j];
                    if (s < bs || (s == bs && (tj < bt || (tj == bt && rj < br)))) { bs = s; bt = tj; br = rj; bv = s_v[j]; }
                }
            }
        }
        if (me.row >= 0) {
            const double inf = INFINITY;
            double g = inf, h = inf, c = inf;
            if (br >= 0) {
                g = bs - me.l;
                if (me.v > 0.0) h = bs / me.v;
                if (me.v > bv && g > 0.0) c = g / (me.v - bv);
                ++c_lead;
                if (g < 0.0) ++c_over;
            }
            leader[me.row] = br;
            spacing[me.row] = bs;
            gap[me.row] = g;
            headway[me.row] = h;
            ttc[me.row] = c;
        }
    }
    tf_count(counters + 0, c_lead);
    tf_count(counters + 1, c_over);
}

// ------------------------------------------------------------------------------------------------ entry points
static inline bool tf_sizes_ok(int64_t N, int64_t R) { return N >= 0 && N < ((int64_t)1 << 31) && R >= 0 && R < ((int64_t)1 << 31); }
static inline bool tf_edges_ok(const double *e, int n) { return n >= 0 && n <= RN_TRAFFIC_MAX_EDGES && (n == 0 || e); }
static inline int64_t tf_lanes(int n_pos, int n_neg) { const int m = (n_pos > n_neg ? n_pos : n_neg) - 1; return m > 0 ? m : 0; }

extern "C" int rn_traffic_lanes(const int64_t *offsets, const double *cols, const int32_t *direction, const double *edges_pos, int n_pos,
                                const double *edges_neg, int n_neg, int64_t N, int64_t R, int32_t *dir, int32_t *lane, int32_t *status,
                                void *stream) {
    if (!tf_sizes_ok(N, R) || !tf_edges_ok(edges_pos, n_pos) || !tf_edges_ok(edges_neg, n_neg) || !status) return RN_EINVAL;
    if (N == 0) return R == 0 ? RN_OK : RN_EINVAL;
    if (!offsets || !dir || (R > 0 && (!cols || !direction || !lane))) return RN_EINVAL;
    hipLaunchKernelGGL(tf_dir_kernel, dim3(rn_blocks(N, TF_THREADS)), dim3(TF_THREADS), 0, (hipStream_t)stream, offsets, direction, N, R,
                       dir, status);
    RN_LAUNCH_CHECK();
    if (R == 0) return RN_OK;
    hipLaunchKernelGGL(tf_lane_kernel, dim3(rn_blocks(R, TF_THREADS)), dim3(TF_THREADS), 0, (hipStream_t)stream, offsets, cols, dir,
                       edges_pos, n_pos, edges_neg, n_neg, N, R, lane, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_traffic_cells(const int64_t *offsets, const double *cols, const int32_t *dir, const double *edges_pos, int n_pos,
                                const double *edges_neg, int n_neg, int64_t N, int64_t R, double t0, double dt, int64_t nt, double x0,
                                double dx, int64_t nx, double max_gap, int64_t *T, int64_t *D, int32_t *n, int64_t *counters,
                                int32_t *status, void *stream) {
    if (!tf_sizes_ok(N, R) || !tf_edges_ok(edges_pos, n_pos) || !tf_edges_ok(edges_neg, n_neg) || !status || !counters) return RN_EINVAL;
    if (!(fabs(t0) < INFINITY) || !(fabs(x0) < INFINITY) || !(dt > 0.0) || !(dt < INFINITY) || !(dx > 0.0) || !(dx < INFINITY) || !(max_gap > 0.0))
        return RN_EINVAL;
    const int64_t L = tf_lanes(n_pos, n_neg), lim = (int64_t)1 << 31;
    if (nt < 0 || nx < 0 || nt >= lim || nx >= lim || (nt > 0 && nx > 0 && 2 * L > (lim - 1) / nt / nx)) return RN_EINVAL;
    if (N == 0) return R == 0 ? RN_OK : RN_EINVAL;
    if (R == 0) return RN_OK;
    if (!offsets || !cols || !dir || (2 * L * nt * nx > 0 && (!T || !D || !n))) return RN_EINVAL;
    hipLaunchKernelGGL(tf_cells_kernel, dim3(rn_blocks(R, TF_THREADS)), dim3(TF_THREADS), 0, (hipStream_t)stream, offsets, cols, dir,
                       edges_pos, n_pos, edges_neg, n_neg, N, R, t0, dt, nt, x0, dx, nx, max_gap, L, T, D, n, counters, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_traffic_leaders(const int64_t *offsets, const double *cols, const int32_t *dir, const int32_t *lane,
                                  const int64_t *frame_off, const int32_t *frame_rows, int64_t N, int64_t R, int64_t F, int64_t Rf,
                                  int32_t *leader, double *spacing, double *gap, double *headway, double *ttc, int64_t *counters,
                                  int32_t *status, void *stream) {
    if (!tf_sizes_ok(N, R) || F < 0 || F >= ((int64_t)1 << 31) || Rf < 0 || Rf >= ((int64_t)1 << 31) || !status || !counters) return RN_EINVAL;
    if (N == 0 && R != 0) return RN_EINVAL;
    if (F == 0) return RN_OK;
    if (!frame_off || (Rf > 0 && (N == 0 || !frame_rows || !offsets || !cols || !dir || !lane || !leader || !spacing || !gap || !headway || !ttc)))
        return RN_EINVAL;
    hipLaunchKernelGGL(tf_leaders_kernel, dim3((unsigned)F), dim3(TF_THREADS), 0, (hipStream_t)stream, offsets, cols, dir, lane, frame_off,
                       frame_rows, N, R, Rf, leader, spacing, gap, headway, ttc, counters, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// Track stitching (track_stitch.py): the fragments one vehicle leaves behind when the tracker loses it at an occlusion or a camera
// hand-over are joined again.  This goes beyond the reference; tests/stitch_cases.py is the plain restatement of every stage.
//
// A tracklet is all rows of one id, in time order; the host packs offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v) and
// direction int32 [R].
//   rn_stitch_endpoints    one thread per (tracklet, end): a line fit through the k = min(n, fit_n) rows nearest the end, sums
//                          sequential in ascending row order -> the end-point block ep fp64 [N,2,RN_STITCH_EP] (head, tail)
//   rn_stitch_costs        the dense matrix W [N,N] of every ordered pair (a's tail -> b's head): a 2-D grid of 64 x 64 tiles, the
//                          b side of a tile staged in LDS, stores coalesced along b.  For tests and small inputs.
//   rn_stitch_candidates   pass A over the same device function: row_has / col_has as plain idempotent byte stores (every writer
//                          writes 1), then a workgroup scan per (direction, side) compacts the tails and heads that have a
//                          candidate, in ascending order
//   rn_stitch_compact      pass B: the compressed matrix Wc [nr', nc'] per direction; recomputing gives the same bits
//   rn_stitch_assign       one wave64 per direction solves linear_sum_assignment(Wc) with the body of lsap_dev.h (the third file
//                          to compile it); the links are the assigned cells with W < 0
//   rn_stitch_chains       pointer jumping over prev in one launch: root, rank, new_id
//   rn_stitch_fill_count   new rows per link and their exclusive prefix
//   rn_stitch_fill_rows    one thread per new row; it finds its link by binary search in the prefix
//
// Arithmetic: fp64, one rounding per operation (this file is in the Makefile's EXACT list: no fma contraction), every expression in
// the order the restatement writes it.
//
// Every index read from memory is checked before use (offsets monotone and inside the rows, candidates, links and prefix slots inside
// their arrays).  A bad value sets a bit of *status and the item is left out; it is never used as an index.
#include "common.h"
#include "lsap_dev.h"
#include "wave_dev.h"

#define ST_THREADS 256
#define ST_WAVES (ST_THREADS / RN_WAVE)
#define ST_TILE 64
#define ST_CHAIN_THREADS 1024
#define ST_LDS_MAX (64 * 1024)       // the solver's arrays move to LDS when they fit in this much

// fields of one end point (include/retinanet_mi355x.h)
enum { EP_T = 0, EP_XH, EP_VX, EP_Y, EP_L, EP_W, EP_H, EP_RX, EP_RY, EP_RL, EP_RW, EP_RH, EP_SGN, EP_K };

struct StParams { double max_gap, back_tol, sx0, sx1, sy, ss, max_cost; };
struct StEnd { double t, xh, vx, y, l, w, h, sgn; };

__device__ __forceinline__ const double *st_ep(const double *ep, int64_t i, int end) { return ep + (i * 2 + end) * RN_STITCH_EP; }

__device__ __forceinline__ StEnd st_load(const double *e) {
    StEnd s;
    s.t = e[EP_T]; s.xh = e[EP_XH]; s.vx = e[EP_VX]; s.y = e[EP_Y]; s.l = e[EP_L]; s.w = e[EP_W]; s.h = e[EP_H]; s.sgn = e[EP_SGN];
    return s;
}

// a's tail -> b's head: linkable?  cost as the restatement writes it, left to right.  A NaN fails every comparison: not linkable.
__device__ __forceinline__ bool st_pair(const StEnd &A, const StEnd &B, const StParams &p, double &cost) {
    cost = 0.0;
    const double gap = B.t - A.t;
    if (!(gap > 0.0) || !(gap <= p.max_gap) || A.sgn != B.sgn) return false;
    if (!(A.sgn * (B.xh - A.xh) >= -p.back_tol)) return false;
    const double fwd = fabs(A.xh + A.vx * gap - B.xh), bwd = fabs(B.xh - B.vx * gap - A.xh);
    cost = ((fwd + bwd) / 2.0) / (p.sx0 + p.sx1 * gap) + fabs(A.y - B.y) / p.sy + (fabs(A.l - B.l) + fabs(A.w - B.w) + fabs(A.h - B.h)) / p.ss;
    return cost < p.max_cost;
}

// ------------------------------------------------------------------------------------------------ end points
__global__ void __launch_bounds__(ST_THREADS) st_finite_kernel(const double *__restrict__ cols, int64_t total, int32_t *status) {
    int bad = 0;
    for (int64_t k = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x; k < total; k += (int64_t)gridDim.x * ST_THREADS) {
        const double c = cols[k];
        bad |= !(fabs(c) < INFINITY);                                           // NaN or +-inf
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) rn_flag(status, RN_STITCH_NONFINITE);
}

__global__ void __launch_bounds__(ST_THREADS) st_endpoints_kernel(const int64_t *__restrict__ off, const double *__restrict__ cols,
                                                                   const int32_t *__restrict__ direction, int64_t N, int64_t R, int fit_n,
                                                                   double *__restrict__ ep, int32_t *status) {
    const int64_t idx = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (idx >= 2 * N) return;
    const int64_t i = idx >> 1;
    const int end = (int)(idx & 1);                                             // 0: the head (first rows), 1: the tail
    double *o = ep + idx * RN_STITCH_EP;
    const int64_t lo = off[i], hi = off[i + 1];
    if (lo < 0 || hi <= lo || hi > R) {                                         // a tracklet holds at least one row
        rn_flag(status, RN_STITCH_BAD_OFFSETS);
#pragma unroll
        for (int k = 0; k < RN_STITCH_EP; ++k) o[k] = 0.0;
        return;
    }
    int64_t dsum = 0;
    for (int64_t r = lo; r < hi; ++r) dsum += direction[r];
    const double sgn = dsum >= 0 ? 1.0 : -1.0;
    const int64_t n = hi - lo, k = n < fit_n ? n : fit_n;
    const int64_t r0 = end == 0 ? lo : hi - k, rend = end == 0 ? lo : hi - 1;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                               // t, x, y, l, w, h
    for (int64_t r = r0; r < r0 + k; ++r) {
#pragma unroll
        for (int q = 0; q < 6; ++q) s[q] = s[q] + cols[r * 7 + q];
    }
    const double kd = (double)k;
    const double mt = s[0] / kd, mx = s[1] / kd;
    double Stt = 0.0, Stx = 0.0;
    for (int64_t r = r0; r < r0 + k; ++r) {
        const double dt = cols[r * 7] - mt;
        Stt = Stt + dt * dt;
        Stx = Stx + dt * (cols[r * 7 + 1] - mx);
    }
    const double *e = cols + rend * 7;
    const double vx = (k >= 2 && Stt > 0.0) ? Stx / Stt : sgn * e[6];
    o[EP_T] = e[0];
    o[EP_XH] = mx + vx * (e[0] - mt);
    o[EP_VX] = vx;
    o[EP_Y] = s[2] / kd; o[EP_L] = s[3] / kd; o[EP_W] = s[4] / kd; o[EP_H] = s[5] / kd;
    o[EP_RX] = e[1]; o[EP_RY] = e[2]; o[EP_RL] = e[3]; o[EP_RW] = e[4]; o[EP_RH] = e[5];
    o[EP_SGN] = sgn;
    o[EP_K] = kd;
    o[14] = 0.0; o[15] = 0.0;
}

// ------------------------------------------------------------------------------------------------ link costs
enum { ST_DENSE = 0, ST_HAS = 1, ST_COMPACT = 2 };

// where direction d's compressed matrix starts, and its shape; false when the counts are not a layout inside N and cap
__device__ __forceinline__ bool st_compact_layout(const int32_t *__restrict__ ncand, int64_t N, int64_t cap, int d, int &nr, int &nc,
                                                  int64_t &base) {
    const int64_t r0 = ncand[0], c0 = ncand[1], r1 = ncand[2], c1 = ncand[3];
    if (r0 < 0 || c0 < 0 || r1 < 0 || c1 < 0 || r0 > N || c0 > N || r1 > N || c1 > N || r0 * c0 + r1 * c1 > cap) return false;
    nr = (int)(d ? r1 : r0);
    nc = (int)(d ? c1 : c0);
    base = d ? r0 * c0 : 0;
    return true;
}

// One workgroup per 64 x 64 tile; thread (tx, ty) = (b inside the tile, one of four a rows per step).  ST_DENSE: W [N,N] over the
// tracklets themselves.  ST_HAS: no matrix, has[a] = 1 / has[N + b] = 1 for a linkable pair.  ST_COMPACT: blockIdx.z = direction, the
// a and b of a cell come from the candidate lists and the matrix is Wc of that direction.
template <int MODE>
__global__ void __launch_bounds__(ST_THREADS) st_cost_kernel(const double *__restrict__ ep, int64_t N, StParams p,
                                                              const int32_t *__restrict__ cand, const int32_t *__restrict__ ncand,
                                                              int64_t cap, double *__restrict__ W, uint8_t *__restrict__ has,
                                                              int32_t *status) {
    __shared__ double sb[8][ST_TILE];
    __shared__ int32_t sbi[ST_TILE];
    const int d = blockIdx.z;
    int nr = (int)N, nc = (int)N;
    int64_t base = 0;
    const int32_t *tails = nullptr, *heads = nullptr;
    if (MODE == ST_COMPACT) {
        if (!st_compact_layout(ncand, N, cap, d, nr, nc, base)) {               // uniform over the grid
            if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) rn_flag(status, RN_STITCH_BAD_CANDIDATES);
            return;
        }
        tails = cand + (int64_t)(2 * d) * N;
        heads = cand + (int64_t)(2 * d + 1) * N;
    }
    const int b0 = blockIdx.x * ST_TILE, a0 = blockIdx.y * ST_TILE;
    if (b0 >= nc || a0 >= nr) return;                                           // uniform over the workgroup
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    if (threadIdx.x < ST_TILE) {
        const int jb = b0 + threadIdx.x;
        int32_t b = -1;
        if (jb < nc) {
            b = heads ? heads[jb] : jb;
            if (b < 0 || (int64_t)b >= N) {
                if (MODE == ST_COMPACT) rn_flag(status, RN_STITCH_BAD_CANDIDATES);
                b = -1;
            }
        }
        sbi[threadIdx.x] = b;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 8 * ST_TILE; q += ST_THREADS) {
        const int f = q >> 6, j = q & 63;
        const int32_t b = sbi[j];
        sb[f][j] = b < 0 ? 0.0 : st_ep(ep, b, 0)[f < 7 ? f : EP_SGN];
    }
    __syncthreads();
    const int jb = b0 + tx;
    const int32_t b = sbi[tx];
    StEnd B;
    B.t = sb[0][tx]; B.xh = sb[1][tx]; B.vx = sb[2][tx]; B.y = sb[3][tx]; B.l = sb[4][tx]; B.w = sb[5][tx]; B.h = sb[6][tx]; B.sgn = sb[7][tx];
    for (int ii = ty; ii < ST_TILE; ii += ST_WAVES) {                           // a is uniform over the wave
        const int ia = a0 + ii;
        if (ia >= nr) break;
        const int32_t a = tails ? tails[ia] : ia;
        if (a < 0 || (int64_t)a >= N) {
            if (MODE == ST_COMPACT && tx == 0) rn_flag(status, RN_STITCH_BAD_CANDIDATES);
            if (MODE == ST_COMPACT && jb < nc) W[base + (int64_t)ia * nc + jb] = 0.0;
            continue;
        }
        const StEnd A = st_load(st_ep(ep, a, 1));
        double cost;
        const bool link = b >= 0 && a != b && st_pair(A, B, p, cost);
        if (MODE == ST_HAS) {
            if (link) has[N + b] = 1;
            if (__ballot(link) != 0ull && tx == 0) has[a] = 1;
        } else if (jb < nc) {
            W[base + (int64_t)ia * nc + jb] = link ? cost - p.max_cost : 0.0;
        }
    }
}

// One workgroup per (direction, side): side 0 = the tails with a candidate (row_has), side 1 = the heads (col_has), ascending.
__global__ void __launch_bounds__(ST_THREADS) st_candidates_kernel(const double *__restrict__ ep, const uint8_t *__restrict__ has, int64_t N,
                                                                    int32_t *__restrict__ cand, int32_t *__restrict__ ncand) {
    __shared__ int part[ST_WAVES];
    const int d = blockIdx.x >> 1, side = blockIdx.x & 1;
    int32_t *out = cand + (int64_t)blockIdx.x * N;
    int carry = 0;
    for (int64_t base = 0; base < N; base += ST_THREADS) {
        const int64_t i = base + threadIdx.x;
        bool on = false;
        if (i < N) on = has[(int64_t)side * N + i] != 0 && (st_ep(ep, i, 0)[EP_SGN] > 0.0 ? 0 : 1) == d;
        int total;
        const int incl = block_scan_incl<ST_WAVES>(on ? 1 : 0, part, total);
        if (on) out[carry + incl - 1] = (int32_t)i;                             // carry + incl - 1 <= i < N
        carry += total;
    }
    for (int64_t i = carry + threadIdx.x; i < N; i += ST_THREADS) out[i] = -1;
    if (threadIdx.x == 0) ncand[blockIdx.x] = carry;
}

// ------------------------------------------------------------------------------------------------ assignment
__global__ void __launch_bounds__(64) st_assign_kernel(const double *__restrict__ ep, int64_t N, StParams p, const int32_t *__restrict__ cand,
                                                        const int32_t *__restrict__ ncand, const double *__restrict__ Wc, int64_t cap,
                                                        char *__restrict__ workspace, int64_t ws_stride, int32_t *__restrict__ next,
                                                        int32_t *__restrict__ prev, double *__restrict__ link_cost, int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x, d = blockIdx.x;
    int nr0, nc0;
    int64_t base;
    if (!st_compact_layout(ncand, N, cap, d, nr0, nc0, base)) {
        if (lane == 0) rn_flag(status, RN_STITCH_BAD_CANDIDATES);
        return;
    }
    if (nr0 == 0 || nc0 == 0) return;
    const bool tr = nr0 > nc0;                                                  // scipy transposes tall problems
    const int nr = tr ? nc0 : nr0, nc = tr ? nr0 : nc0;
    if (nr > RN_LSAP_MAX_MIN) {
        if (lane == 0) rn_flag(status, RN_STITCH_TOO_MANY);
        return;
    }
    const int64_t rs = tr ? 1 : nc0, cs = tr ? nc0 : 1;
    const double *C = Wc + base;
    LsapWs w;
    const int64_t bytes = lsap_arrays_layout(nullptr, nr, nc, nullptr);
    if (bytes > ws_stride && bytes > ST_LDS_MAX) {                              // cannot happen for nr <= RN_LSAP_MAX_MIN, nc <= N
        if (lane == 0) rn_flag(status, RN_STITCH_SOLVER);
        return;
    }
    lsap_arrays_layout(bytes <= ST_LDS_MAX ? lds : workspace + (int64_t)d * ws_stride, nr, nc, &w);
    if (lsap_solve_wave<false>(C, rs, cs, nr, nc, w, lane) != 0) {
        if (lane == 0) rn_flag(status, RN_STITCH_SOLVER);
        return;
    }
    const int32_t *tails = cand + (int64_t)(2 * d) * N, *heads = cand + (int64_t)(2 * d + 1) * N;
    for (int i = lane; i < nr; i += 64) {
        const int j = w.col4row[i];
        if (j < 0 || j >= nc) continue;
        const int r = tr ? j : i, c = tr ? i : j;                               // r: the tail's place in its list, c: the head's
        if (!(C[(int64_t)r * nc0 + c] < 0.0)) continue;
        const int32_t a = tails[r], b = heads[c];
        if (a < 0 || b < 0 || (int64_t)a >= N || (int64_t)b >= N) { rn_flag(status, RN_STITCH_BAD_CANDIDATES); continue; }
        double cost;
        st_pair(st_load(st_ep(ep, a, 1)), st_load(st_ep(ep, b, 0)), p, cost);
        next[a] = b;                                                            // a tail and a head are assigned once each
        prev[b] = a;
        link_cost[a] = cost;
    }
}

// ------------------------------------------------------------------------------------------------ chains
// One workgroup; ws holds two (pointer, rank) pairs of N int32 each.  A root points to itself with rank 0, so a jump over it adds
// nothing: after ceil(log2 N) rounds every pointer is the chain's root and the rank the distance to it.
__global__ void __launch_bounds__(ST_CHAIN_THREADS) st_chains_kernel(const int32_t *__restrict__ prev, const int64_t *__restrict__ ids, int64_t N,
                                                                      int32_t *ws, int32_t *__restrict__ root, int32_t *__restrict__ rank,
                                                                      int64_t *__restrict__ new_id, int32_t *status) {
    int32_t *pin = ws, *rin = ws + N, *pout = ws + 2 * N, *rout = ws + 3 * N;
    for (int64_t i = threadIdx.x; i < N; i += ST_CHAIN_THREADS) {
        int32_t q = prev[i];
        if (q < -1 || (int64_t)q >= N || (int64_t)q == i) { rn_flag(status, RN_STITCH_BAD_LINK); q = -1; }
        pin[i] = q < 0 ? (int32_t)i : q;
        rin[i] = q < 0 ? 0 : 1;
    }
    __syncthreads();
    for (int64_t span = 1; span < N; span <<= 1) {                              // uniform over the workgroup
        for (int64_t i = threadIdx.x; i < N; i += ST_CHAIN_THREADS) {
            const int32_t q = pin[i];
            pout[i] = pin[q];
            rout[i] = rin[i] + rin[q];
        }
        __syncthreads();
        int32_t *t = pin; pin = pout; pout = t;
        t = rin; rin = rout; rout = t;
    }
    for (int64_t i = threadIdx.x; i < N; i += ST_CHAIN_THREADS) {
        const int32_t q = pin[i];
        root[i] = q;
        rank[i] = rin[i];
        new_id[i] = ids[q];
    }
}

// ------------------------------------------------------------------------------------------------ gap fill
// how many k >= 1 have t_e + k * dt < t_s: the largest such k, by bisection (the predicate is monotone in k)
__device__ __forceinline__ int st_fill_n(double te, double ts, double dt, int32_t *status) {
    const double g = ts - te;
    if (!(g > 0.0)) return 0;
    const double est = g / dt;
    if (!(est < (double)RN_STITCH_MAX_FILL)) { rn_flag(status, RN_STITCH_FILL_OVERFLOW); return 0; }
    int lo = 0, hi = (int)est + 2;
    while (lo < hi) {                                                           // at most 22 steps
        const int mid = lo + (hi - lo + 1) / 2;
        if (te + (double)mid * dt < ts) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the link of tracklet a, checked: false when it has none
__device__ __forceinline__ bool st_link(const int32_t *__restrict__ next, int64_t a, int64_t N, int32_t &b, int32_t *status) {
    b = next[a];
    if (b < 0) return false;
    if ((int64_t)b >= N || (int64_t)b == a) { rn_flag(status, RN_STITCH_BAD_LINK); return false; }
    return true;
}

__global__ void __launch_bounds__(ST_THREADS) st_fill_count_kernel(const double *__restrict__ ep, const int32_t *__restrict__ next, int64_t N,
                                                                    double fill_rate, int32_t *__restrict__ count, int64_t *__restrict__ prefix,
                                                                    int32_t *status) {
    __shared__ long long part[ST_WAVES];
    const double dt = 1.0 / fill_rate;
    int64_t carry = 0;
    for (int64_t base = 0; base < N; base += ST_THREADS) {
        const int64_t a = base + threadIdx.x;
        int c = 0;
        if (a < N) {
            int32_t b;
            if (st_link(next, a, N, b, status)) c = st_fill_n(st_ep(ep, a, 1)[EP_T], st_ep(ep, b, 0)[EP_T], dt, status);
            count[a] = c;
        }
        long long total;
        const long long incl = block_scan_incl<ST_WAVES, long long>(c, part, total);
        if (a < N) prefix[a] = carry + (int64_t)(incl - c);
        carry += (int64_t)total;
    }
    if (threadIdx.x == 0) prefix[N] = carry;
}

__global__ void __launch_bounds__(ST_THREADS) st_fill_rows_kernel(const double *__restrict__ ep, const int32_t *__restrict__ next,
                                                                   const int64_t *__restrict__ prefix, int64_t N, int64_t U, double fill_rate,
                                                                   double *__restrict__ fields, double *__restrict__ time,
                                                                   int32_t *__restrict__ link, uint8_t *__restrict__ side, int32_t *status) {
    const int64_t u = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    const int64_t total = prefix[N];
    if (total < 0 || total > U) {
        if (u == 0) rn_flag(status, RN_STITCH_BAD_PREFIX);
        return;
    }
    if (u >= total) return;
    int64_t lo = 0, hi = N - 1;                                                 // the last a with prefix[a] <= u
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (prefix[mid] <= u) lo = mid;
        else hi = mid - 1;
    }
    const int64_t a = lo, k = u - prefix[a] + 1;
    int32_t b;
    if (prefix[a] > u || prefix[a + 1] <= u || !st_link(next, a, N, b, status)) { rn_flag(status, RN_STITCH_BAD_PREFIX); return; }
    const double *A = st_ep(ep, a, 1), *B = st_ep(ep, b, 0);
    const double te = A[EP_T], ts = B[EP_T];
    const double g = ts - te, dt = 1.0 / fill_rate;
    const double tk = te + (double)k * dt;
    const double s = (tk - te) / g;                                             // u of the issue
    const double om = 1.0 - s;
    const double xa = A[EP_RX], xb = B[EP_RX], va = A[EP_VX], vb = B[EP_VX];
    const double h00 = (1.0 + 2.0 * s) * (om * om), h10 = s * (om * om), h01 = (s * s) * (3.0 - 2.0 * s), h11 = (s * s) * (s - 1.0);
    const double d00 = 6.0 * s * s - 6.0 * s, d10 = 3.0 * s * s - 4.0 * s + 1.0, d01 = 6.0 * s - 6.0 * s * s, d11 = 3.0 * s * s - 2.0 * s;
    double *o = fields + u * 6;
    o[0] = h00 * xa + h10 * g * va + h01 * xb + h11 * g * vb;
    o[1] = om * A[EP_RY] + s * B[EP_RY];
    o[2] = om * A[EP_RL] + s * B[EP_RL];
    o[3] = om * A[EP_RW] + s * B[EP_RW];
    o[4] = om * A[EP_RH] + s * B[EP_RH];
    o[5] = fabs((d00 * xa + d10 * g * va + d01 * xb + d11 * g * vb) / g);
    time[u] = tk;
    link[u] = (int32_t)a;
    side[u] = s <= 0.5 ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------ entry points
static inline bool st_params(double max_gap, double back_tol, double sx0, double sx1, double sy, double ss, double max_cost, StParams &p) {
    p.max_gap = max_gap; p.back_tol = back_tol; p.sx0 = sx0; p.sx1 = sx1; p.sy = sy; p.ss = ss; p.max_cost = max_cost;
    return max_gap > 0.0 && back_tol >= 0.0 && sx0 > 0.0 && sx1 >= 0.0 && sy > 0.0 && ss > 0.0 && max_cost > 0.0;
}
static inline dim3 st_tiles(int64_t N, int z) { return dim3(rn_blocks(N, ST_TILE), rn_blocks(N, ST_TILE), z); }
static inline bool st_count_ok(int64_t N) { return N >= 0 && N <= RN_STITCH_MAX_TRACKLETS; }

extern "C" int rn_stitch_endpoints(const int64_t *offsets, const double *cols, const int32_t *direction, int64_t N, int64_t R, int fit_n,
                                   double *ep, int32_t *status, void *stream) {
    if (!st_count_ok(N) || R < 0 || R >= ((int64_t)1 << 31) || fit_n < 1 || fit_n > RN_STITCH_MAX_FIT || !status) return RN_EINVAL;
    if (N == 0) return RN_OK;
    if (!offsets || !cols || !direction || !ep) return RN_EINVAL;
    if (R > 0) {
        int blocks = rn_blocks(R * 7, ST_THREADS * 8);
        blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
        hipLaunchKernelGGL(st_finite_kernel, dim3(blocks), dim3(ST_THREADS), 0, (hipStream_t)stream, cols, R * 7, status);
        RN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(st_endpoints_kernel, dim3(rn_blocks(2 * N, ST_THREADS)), dim3(ST_THREADS), 0, (hipStream_t)stream, offsets, cols,
                       direction, N, R, fit_n, ep, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_stitch_costs(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1, double sigma_y,
                               double sigma_size, double max_cost, double *W, void *stream) {
    StParams p;
    if (!st_count_ok(N) || !st_params(max_gap, back_tol, sigma_x0, sigma_x1, sigma_y, sigma_size, max_cost, p)) return RN_EINVAL;
    if (N == 0) return RN_OK;
    if (!ep || !W) return RN_EINVAL;
    hipLaunchKernelGGL(st_cost_kernel<ST_DENSE>, st_tiles(N, 1), dim3(ST_THREADS), 0, (hipStream_t)stream, ep, N, p, (const int32_t *)nullptr,
                       (const int32_t *)nullptr, (int64_t)0, W, (uint8_t *)nullptr, (int32_t *)nullptr);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_stitch_candidates(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1,
                                    double sigma_y, double sigma_size, double max_cost, uint8_t *has, int32_t *cand, int32_t *ncand,
                                    void *stream) {
    StParams p;
    if (!st_count_ok(N) || !st_params(max_gap, back_tol, sigma_x0, sigma_x1, sigma_y, sigma_size, max_cost, p) || !ncand) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        hipError_t e = hipMemsetAsync(ncand, 0, 4 * sizeof(int32_t), s);
        return e == hipSuccess ? RN_OK : (int)e;
    }
    if (!ep || !has || !cand) return RN_EINVAL;
    hipError_t e = hipMemsetAsync(has, 0, (size_t)(2 * N), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(st_cost_kernel<ST_HAS>, st_tiles(N, 1), dim3(ST_THREADS), 0, s, ep, N, p, (const int32_t *)nullptr,
                       (const int32_t *)nullptr, (int64_t)0, (double *)nullptr, has, (int32_t *)nullptr);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(st_candidates_kernel, dim3(4), dim3(ST_THREADS), 0, s, ep, has, N, cand, ncand);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_stitch_compact(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1,
                                 double sigma_y, double sigma_size, double max_cost, const int32_t *cand, const int32_t *ncand, int64_t cap,
                                 double *Wc, int32_t *status, void *stream) {
    StParams p;
    if (!st_count_ok(N) || cap < 0 || !st_params(max_gap, back_tol, sigma_x0, sigma_x1, sigma_y, sigma_size, max_cost, p) || !status)
        return RN_EINVAL;
    if (N == 0 || cap == 0) return RN_OK;
    if (!ep || !cand || !ncand || !Wc) return RN_EINVAL;
    hipLaunchKernelGGL(st_cost_kernel<ST_COMPACT>, st_tiles(N, 2), dim3(ST_THREADS), 0, (hipStream_t)stream, ep, N, p, cand, ncand, cap, Wc,
                       (uint8_t *)nullptr, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

static inline int64_t st_assign_stride(int64_t N) {
    return lsap_arrays_layout(nullptr, N < RN_LSAP_MAX_MIN ? N : RN_LSAP_MAX_MIN, N, nullptr);
}

extern "C" int64_t rn_stitch_assign_workspace_bytes(int64_t N) {
    return N <= 0 || N > RN_STITCH_MAX_TRACKLETS ? 0 : 2 * st_assign_stride(N);
}

extern "C" int rn_stitch_assign(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1, double sigma_y,
                                double sigma_size, double max_cost, const int32_t *cand, const int32_t *ncand, const double *Wc, int64_t cap,
                                void *workspace, int32_t *next, int32_t *prev, double *link_cost, int32_t *status, void *stream) {
    StParams p;
    if (!st_count_ok(N) || cap < 0 || !st_params(max_gap, back_tol, sigma_x0, sigma_x1, sigma_y, sigma_size, max_cost, p) || !status)
        return RN_EINVAL;
    if (N == 0) return RN_OK;
    if (!ep || !cand || !ncand || !workspace || !next || !prev || !link_cost || (cap > 0 && !Wc)) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(next, 0xFF, (size_t)N * sizeof(int32_t), s);  // -1: no link
    if (e == hipSuccess) e = hipMemsetAsync(prev, 0xFF, (size_t)N * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(link_cost, 0, (size_t)N * sizeof(double), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(st_assign_kernel, dim3(2), dim3(64), ST_LDS_MAX, s, ep, N, p, cand, ncand, Wc, cap, reinterpret_cast<char *>(workspace),
                       st_assign_stride(N), next, prev, link_cost, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_stitch_chains(const int32_t *prev, const int64_t *ids, int64_t N, int32_t *workspace, int32_t *root, int32_t *rank,
                                int64_t *new_id, int32_t *status, void *stream) {
    if (!st_count_ok(N) || !status) return RN_EINVAL;
    if (N == 0) return RN_OK;
    if (!prev || !ids || !workspace || !root || !rank || !new_id) return RN_EINVAL;
    hipLaunchKernelGGL(st_chains_kernel, dim3(1), dim3(ST_CHAIN_THREADS), 0, (hipStream_t)stream, prev, ids, N, workspace, root, rank, new_id,
                       status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_stitch_fill_count(const double *ep, const int32_t *next, int64_t N, double fill_rate, int32_t *count, int64_t *prefix,
                                    int32_t *status, void *stream) {
    if (!st_count_ok(N) || !(fill_rate > 0.0) || !(fill_rate < INFINITY) || !prefix || !status) return RN_EINVAL;
    if (N > 0 && (!ep || !next || !count)) return RN_EINVAL;
    hipLaunchKernelGGL(st_fill_count_kernel, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, ep, next, N, fill_rate, count, prefix, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_stitch_fill_rows(const double *ep, const int32_t *next, const int64_t *prefix, int64_t N, int64_t U, double fill_rate,
                                   double *fields, double *time, int32_t *link, uint8_t *side, int32_t *status, void *stream) {
    if (!st_count_ok(N) || U < 0 || U >= ((int64_t)1 << 31) * ST_THREADS || !(fill_rate > 0.0) || !(fill_rate < INFINITY) || !status)
        return RN_EINVAL;
    if (N == 0 || U == 0) return RN_OK;
    if (!ep || !next || !prefix || !fields || !time || !link || !side) return RN_EINVAL;
    hipLaunchKernelGGL(st_fill_rows_kernel, dim3(rn_blocks(U, ST_THREADS)), dim3(ST_THREADS), 0, (hipStream_t)stream, ep, next, prefix, N, U,
                       fill_rate, fields, time, link, side, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// The rectangular assignment solver shared by track_assoc.hip (rn_linear_sum_assignment) and mot_eval.hip (rn_mot_assign):
// scipy's rectangular_lsap restated for one wave64 (Crouse 2016, shortest augmenting path), with scipy's evaluation order
// and tie rule -- see the header of track_assoc.hip.  Both files compile this one body.
#pragma once
#include <limits.h>
#include <math.h>

#include "common.h"

// ---------------------------------------------------------------------------------------------- assignment
// Problem after the transpose: nr <= nc.  Column arrays sized nc, row arrays sized nr.
struct LsapWs {
    double *u, *v, *spc;            // row duals [nr], column duals [nc], shortest path costs [nc]
    int32_t *path, *row4col, *remaining, *col4row;
    uint8_t *SR, *SC;
};

// Layout of the per-problem arrays from `base` (nullptr: only the size).  The same layout is used in global memory and
// in LDS.
__host__ __device__ static inline int64_t lsap_arrays_layout(char *base, int64_t nr, int64_t nc, LsapWs *w) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *r = base ? base + o : nullptr; o += (bytes + 15) & ~(int64_t)15; return r; };
    LsapWs t;
    t.u = reinterpret_cast<double *>(take(nr * 8));
    t.v = reinterpret_cast<double *>(take(nc * 8));
    t.spc = reinterpret_cast<double *>(take(nc * 8));
    t.path = reinterpret_cast<int32_t *>(take(nc * 4));
    t.row4col = reinterpret_cast<int32_t *>(take(nc * 4));
    t.remaining = reinterpret_cast<int32_t *>(take(nc * 4));
    t.col4row = reinterpret_cast<int32_t *>(take(nr * 4));
    t.SR = reinterpret_cast<uint8_t *>(take(nr));
    t.SC = reinterpret_cast<uint8_t *>(take(nc));
    if (w) *w = t;
    return o;
}

// Make the lanes' LDS / global writes visible to the other lanes of the wave before they read them.
__device__ __forceinline__ void lsap_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// (value, unassigned, position) merge with scipy's tie rule; order-independent, so it is a valid lane reduction.
__device__ __forceinline__ void lsap_pick(double &v, int &un, int &pos, double v2, int un2, int pos2) {
    bool take;
    if (v2 < v) take = true;
    else if (v < v2) take = false;
    else if (un && un2) take = pos2 > pos;              // equal: the last unassigned column
    else if (un || un2) take = un2 != 0;                // an unassigned column beats an assigned one
    else take = pos2 < pos;                             // none unassigned: the first column
    if (take) { v = v2; un = un2; pos = pos2; }
}

// One wave64 solves one problem with nr <= nc (the caller transposes through the strides): C(i,j) = cost[i*rs + j*cs],
// negated when NEGATE (scipy's maximize=True negates the matrix and runs the same solver).  The arrays of w are
// initialised here.  Returns 0 with the assignment in w.col4row / w.row4col, or 2 when no finite complete assignment
// exists.  Every loop is bounded: nr augmentations of at most nc steps, and a path of at most nr + 1 rows.
template <bool NEGATE>
__device__ __forceinline__ int lsap_solve_wave(const double *__restrict__ cost, int64_t rs, int64_t cs, int nr, int nc,
                                               const LsapWs &w, int lane) {
    for (int r = lane; r < nr; r += 64) { w.u[r] = 0.0; w.col4row[r] = -1; }
    for (int c = lane; c < nc; c += 64) { w.v[c] = 0.0; w.row4col[c] = -1; w.path[c] = -1; }
    lsap_wave_sync();

    for (int curRow = 0; curRow < nr; ++curRow) {
        // augmenting_path(): reset, then a Dijkstra-like search from curRow
        for (int it = lane; it < nc; it += 64) { w.remaining[it] = nc - it - 1; w.spc[it] = INFINITY; w.SC[it] = 0; }
        for (int r = lane; r < nr; r += 64) w.SR[r] = 0;
        lsap_wave_sync();
        double minVal = 0.0;
        int i = curRow, nrem = nc, sink = -1;
        for (int step = 0; step < nc && sink == -1; ++step) {
            if (lane == 0) w.SR[i] = 1;
            const double ui = w.u[i];
            const double *crow = cost + (int64_t)i * rs;
            double lv = INFINITY;
            int lu = 0, lp = INT_MAX;
            for (int it = lane; it < nrem; it += 64) {
                const int j = w.remaining[it];
                const double r = ((minVal + (NEGATE ? -crow[(int64_t)j * cs] : crow[(int64_t)j * cs])) - ui) - w.v[j];
                double s = w.spc[j];
                if (r < s) { w.path[j] = i; w.spc[j] = r; s = r; }
                lsap_pick(lv, lu, lp, s, w.row4col[j] == -1, it);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double v2 = __shfl_xor(lv, off, 64);
                const int u2 = __shfl_xor(lu, off, 64), p2 = __shfl_xor(lp, off, 64);
                lsap_pick(lv, lu, lp, v2, u2, p2);
            }
            lsap_wave_sync();
            minVal = lv;
            if (minVal == INFINITY || lp == INT_MAX) break;                  // no finite path: infeasible
            const int j = w.remaining[lp];
            if (w.row4col[j] == -1) sink = j;
            else i = w.row4col[j];
            lsap_wave_sync();
            if (lane == 0) {
                w.SC[j] = 1;
                w.remaining[lp] = w.remaining[nrem - 1];                     // swap-with-last removal
            }
            --nrem;                                                          // lane-uniform
            lsap_wave_sync();
        }
        if (sink < 0) return 2;                                                  // infeasible (or the bound was hit)
        // dual update
        if (lane == 0) w.u[curRow] += minVal;
        for (int r = lane; r < nr; r += 64)
            if (w.SR[r] && r != curRow) w.u[r] += minVal - w.spc[w.col4row[r]];
        for (int c = lane; c < nc; c += 64)
            if (w.SC[c]) w.v[c] -= minVal - w.spc[c];
        lsap_wave_sync();
        // augment along path (at most nr + 1 rows)
        if (lane == 0) {
            int j = sink;
            for (int k = 0; k <= nr; ++k) {
                const int r = w.path[j];
                w.row4col[j] = r;
                const int t = w.col4row[r];
                w.col4row[r] = j;
                j = t;
                if (r == curRow) break;
            }
        }
        lsap_wave_sync();
    }
    return 0;
}

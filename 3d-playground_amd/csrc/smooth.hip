// Fixed-interval (Rauch-Tung-Striebel) smoothing of tracking output (track_smooth.py): an offline pass over every tracklet that
// uses all of its rows, past and future, with the motion model fit_filter.py fits.  This goes beyond the reference;
// tests/smooth_cases.py is the plain restatement of both passes.
//
// A tracklet is all rows of one id, in time order; the host packs offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v) and
// direction int32 [R] (track_stitch.pack_tracklets).  State (x, y, l, w, h, v), measurement (x, y, l, w, h): H = [I5 | 0], fixed.
//   rn_smooth_filter   forward: predict with F = I + f e0 e5^T (f = d dt), the innovation's chi-square (nis), the gate, the
//                      Joseph-form update -> filt fp64 [R,27] (6 means, the 21 entries a <= b of the covariance), nis, flag
//   rn_smooth_rts      backward: C = P F^T (P-)^-1 from the stored filtered rows -> out fp64 [R,12] (6 means, 6 variances)
// One lane per tracklet, lane i of the grid on tracklet order[i]; a lane is a serial fp64 recurrence with its covariance in
// registers (no LDS, no scratch memory: every array index is a compile-time constant after unrolling).
//
// Arithmetic: fp64, one rounding per operation (this file is in the Makefile's EXACT list: no fma contraction), every sum in
// ascending index from its first product, every covariance computed for a <= b only and read through sm_tri, so it is symmetric
// by construction.
//
// Every index read from memory is checked before use: an order entry outside the tracklets or offsets outside the rows set a bit
// of *status and the lane ends; so do a non-finite field, a time step <= 0 and a pivot <= 0.  What such a tracklet's rows hold
// afterwards is unspecified.
#include "common.h"
#include "wave_dev.h"

#define SM_THREADS 64
#define SM_FILT 27
#define SM_OUT 12

__host__ __device__ constexpr int sm_tri(int a, int b) { return a <= b ? a * 6 - a * (a - 1) / 2 + (b - a) : b * 6 - b * (b - 1) / 2 + (a - b); }

struct SmTrack { int64_t lo, hi; double d; };

// the lane's tracklet, checked: false (and a status bit) when it cannot be walked
__device__ __forceinline__ bool sm_track(const int64_t *__restrict__ off, const int32_t *__restrict__ order,
                                         const int32_t *__restrict__ direction, int64_t N, int64_t R, int32_t *status, SmTrack &tk) {
    const int64_t lane = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (lane >= N) return false;
    const int64_t i = order[lane];
    if (i < 0 || i >= N) { rn_flag(status, RN_SMOOTH_BAD_ORDER); return false; }
    tk.lo = off[i];
    tk.hi = off[i + 1];
    if (tk.lo < 0 || tk.hi <= tk.lo || tk.hi > R) { rn_flag(status, RN_SMOOTH_BAD_OFFSETS); return false; }
    int64_t dsum = 0;
    for (int64_t r = tk.lo; r < tk.hi; ++r) dsum += direction[r];
    tk.d = dsum >= 0 ? 1.0 : -1.0;
    return true;
}

// F s and F P F^T + Qk: row 0 of G = F P, then column 0 of G F^T, entries a <= b only; Qk = ((q_scale Q) dt) / dt_default
__device__ __forceinline__ void sm_predict(double (&s)[6], double (&U)[21], double f, double dt, const double *__restrict__ model,
                                           double dt_default) {
    s[0] = s[0] + f * s[5];
    double G0[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) G0[b] = U[sm_tri(0, b)] + f * U[sm_tri(5, b)];
    U[sm_tri(0, 0)] = G0[0] + f * G0[5];
#pragma unroll
    for (int b = 1; b < 6; ++b) U[sm_tri(0, b)] = G0[b];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) U[sm_tri(a, b)] = U[sm_tri(a, b)] + (model[a * 6 + b] * dt) / dt_default;
}

// S = L D L^T in Cholesky-Crout order, S given as its triangle (S[sm_tri-like index n-wide] through the functor); false on a
// pivot that is not a positive finite number
template <int NN, typename Get>
__device__ __forceinline__ bool sm_ldl(Get S, double (&L)[NN][NN], double (&D)[NN]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NN; ++j) {
        double v[NN];
#pragma unroll
        for (int k = 0; k < j; ++k) v[k] = L[j][k] * D[k];
        double acc = S(j, j);
#pragma unroll
        for (int k = 0; k < j; ++k) acc = acc - L[j][k] * v[k];
        D[j] = acc;
        ok = ok && acc > 0.0 && acc < INFINITY;
#pragma unroll
        for (int i = j + 1; i < NN; ++i) {
            double a2 = S(i, j);
#pragma unroll
            for (int k = 0; k < j; ++k) a2 = a2 - L[i][k] * v[k];
            L[i][j] = a2 / D[j];
        }
    }
    return ok;
}

template <int NN>
__device__ __forceinline__ void sm_solve(const double (&L)[NN][NN], const double (&D)[NN], const double (&rhs)[NN], double (&x)[NN]) {
    double w[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
        double acc = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) acc = acc - L[i][k] * w[k];
        w[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) w[i] = w[i] / D[i];
#pragma unroll
    for (int i = NN - 1; i >= 0; --i) {
        double acc = w[i];
#pragma unroll
        for (int k = i + 1; k < NN; ++k) acc = acc - L[k][i] * x[k];
        x[i] = acc;
    }
}

__device__ __forceinline__ bool sm_finite_row(const double *__restrict__ c) {
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 7; ++q) ok = ok && fabs(c[q]) < INFINITY;               // false for a NaN
    return ok;
}

__device__ __forceinline__ void sm_store_filt(double *__restrict__ o, const double (&s)[6], const double (&U)[21]) {
#pragma unroll
    for (int a = 0; a < 6; ++a) o[a] = s[a];
#pragma unroll
    for (int i = 0; i < 21; ++i) o[6 + i] = U[i];
}

// ------------------------------------------------------------------------------------------------ forward
__global__ void __launch_bounds__(SM_THREADS) sm_filter_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ order,
                                                                const double *__restrict__ cols, const int32_t *__restrict__ direction,
                                                                const double *__restrict__ model, double gate, double dt_default, int64_t N,
                                                                int64_t R, double *__restrict__ filt, double *__restrict__ nis,
                                                                uint8_t *__restrict__ flag, int32_t *status) {
    SmTrack tk;
    if (!sm_track(off, order, direction, N, R, status, tk)) return;
    const double *Rm = model + 36, *P0 = model + 61;
    const double *c = cols + tk.lo * 7;
    if (!sm_finite_row(c)) { rn_flag(status, RN_SMOOTH_NONFINITE); return; }
    double s[6], U[21];
#pragma unroll
    for (int a = 0; a < 6; ++a) s[a] = c[1 + a];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) U[sm_tri(a, b)] = P0[a * 6 + b];
    sm_store_filt(filt + tk.lo * SM_FILT, s, U);
    nis[tk.lo] = 0.0;
    flag[tk.lo] = 0;
    double t_prev = c[0];
    for (int64_t r = tk.lo + 1; r < tk.hi; ++r) {
        c = cols + r * 7;
        if (!sm_finite_row(c)) { rn_flag(status, RN_SMOOTH_NONFINITE); return; }
        const double dt = c[0] - t_prev;
        if (!(dt > 0.0)) { rn_flag(status, RN_SMOOTH_BAD_DT); return; }
        t_prev = c[0];
        sm_predict(s, U, tk.d * dt, dt, model, dt_default);
        double y[5], L[5][5], D[5], x[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) y[j] = c[1 + j] - s[j];
        if (!sm_ldl<5>([&](int i, int j) { return U[sm_tri(j, i)] + Rm[j * 5 + i]; }, L, D)) { rn_flag(status, RN_SMOOTH_PIVOT); return; }
        sm_solve<5>(L, D, y, x);
        double q = y[0] * x[0];
#pragma unroll
        for (int j = 1; j < 5; ++j) q = q + y[j] * x[j];
        const bool out = gate > 0.0 && q > gate;
        if (!out) {                                                             // else the row counts as missing: s = s-, P = P-
            double K[6][5], A[6][6];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double rhs[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) rhs[j] = U[sm_tri(a, j)];
                sm_solve<5>(L, D, rhs, K[a]);
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double acc = K[a][0] * y[0];
#pragma unroll
                for (int j = 1; j < 5; ++j) acc = acc + K[a][j] * y[j];
                s[a] = s[a] + acc;
#pragma unroll
                for (int cc = 0; cc < 5; ++cc) A[a][cc] = (a == cc ? 1.0 : 0.0) - K[a][cc];
                A[a][5] = a == 5 ? 1.0 : 0.0;
            }
            double Un[21];
#pragma unroll
            for (int a = 0; a < 6; ++a) {                                       // P = A P- A^T + K R K^T, row a: B = (A P-)[a], KR = (K R)[a]
                double B[6], KR[5];
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    double acc = A[a][0] * U[sm_tri(0, b)];
#pragma unroll
                    for (int cc = 1; cc < 6; ++cc) acc = acc + A[a][cc] * U[sm_tri(cc, b)];
                    B[b] = acc;
                }
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    double acc = K[a][0] * Rm[j];
#pragma unroll
                    for (int i = 1; i < 5; ++i) acc = acc + K[a][i] * Rm[i * 5 + j];
                    KR[j] = acc;
                }
#pragma unroll
                for (int b = a; b < 6; ++b) {
                    double t1 = B[0] * A[b][0];
#pragma unroll
                    for (int cc = 1; cc < 6; ++cc) t1 = t1 + B[cc] * A[b][cc];
                    double t2 = KR[0] * K[b][0];
#pragma unroll
                    for (int j = 1; j < 5; ++j) t2 = t2 + KR[j] * K[b][j];
                    Un[sm_tri(a, b)] = t1 + t2;
                }
            }
#pragma unroll
            for (int i = 0; i < 21; ++i) U[i] = Un[i];
        }
        sm_store_filt(filt + r * SM_FILT, s, U);
        nis[r] = q;
        flag[r] = out ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ backward
__global__ void __launch_bounds__(SM_THREADS) sm_rts_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ order,
                                                             const double *__restrict__ cols, const int32_t *__restrict__ direction,
                                                             const double *__restrict__ model, double dt_default, int64_t N, int64_t R,
                                                             const double *__restrict__ filt, double *__restrict__ out, int32_t *status) {
    SmTrack tk;
    if (!sm_track(off, order, direction, N, R, status, tk)) return;
    double ss[6], Us[21];                                                       // the smoothed row k + 1
    {
        const double *fr = filt + (tk.hi - 1) * SM_FILT;
#pragma unroll
        for (int a = 0; a < 6; ++a) ss[a] = fr[a];
#pragma unroll
        for (int i = 0; i < 21; ++i) Us[i] = fr[6 + i];
        double *o = out + (tk.hi - 1) * SM_OUT;
#pragma unroll
        for (int a = 0; a < 6; ++a) { o[a] = ss[a]; o[6 + a] = Us[sm_tri(a, a)]; }
    }
    for (int64_t r = tk.hi - 2; r >= tk.lo; --r) {
        const double dt = cols[(r + 1) * 7] - cols[r * 7];
        if (!(dt > 0.0)) { rn_flag(status, RN_SMOOTH_BAD_DT); return; }
        const double f = tk.d * dt;
        const double *fr = filt + r * SM_FILT;
        double s[6], U[21], sp[6], Um[21];
#pragma unroll
        for (int a = 0; a < 6; ++a) sp[a] = s[a] = fr[a];
#pragma unroll
        for (int i = 0; i < 21; ++i) Um[i] = U[i] = fr[6 + i];
        sm_predict(sp, Um, f, dt, model, dt_default);
        double L[6][6], D[6], C[6][6];
        if (!sm_ldl<6>([&](int i, int j) { return Um[sm_tri(j, i)]; }, L, D)) { rn_flag(status, RN_SMOOTH_PIVOT); return; }
#pragma unroll
        for (int a = 0; a < 6; ++a) {                                           // row a of P F^T: column 0 only differs from P
            double rhs[6];
            rhs[0] = U[sm_tri(a, 0)] + f * U[sm_tri(a, 5)];
#pragma unroll
            for (int b = 1; b < 6; ++b) rhs[b] = U[sm_tri(a, b)];
            sm_solve<6>(L, D, rhs, C[a]);
        }
        double e[6], Dl[21];
#pragma unroll
        for (int b = 0; b < 6; ++b) e[b] = ss[b] - sp[b];
#pragma unroll
        for (int i = 0; i < 21; ++i) Dl[i] = Us[i] - Um[i];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double acc = C[a][0] * e[0];
#pragma unroll
            for (int b = 1; b < 6; ++b) acc = acc + C[a][b] * e[b];
            ss[a] = s[a] + acc;
            double E[6];
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) {
                double a2 = C[a][0] * Dl[sm_tri(0, cc)];
#pragma unroll
                for (int b = 1; b < 6; ++b) a2 = a2 + C[a][b] * Dl[sm_tri(b, cc)];
                E[cc] = a2;
            }
#pragma unroll
            for (int b = a; b < 6; ++b) {
                double a3 = E[0] * C[b][0];
#pragma unroll
                for (int cc = 1; cc < 6; ++cc) a3 = a3 + E[cc] * C[b][cc];
                Us[sm_tri(a, b)] = U[sm_tri(a, b)] + a3;
            }
        }
        double *o = out + r * SM_OUT;
#pragma unroll
        for (int a = 0; a < 6; ++a) { o[a] = ss[a]; o[6 + a] = Us[sm_tri(a, a)]; }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static inline bool sm_sizes_ok(int64_t N, int64_t R) { return N >= 0 && N <= RN_SMOOTH_MAX_TRACKLETS && R >= 0 && R < ((int64_t)1 << 31); }

extern "C" int rn_smooth_filter(const int64_t *offsets, const int32_t *order, const double *cols, const int32_t *direction,
                                const double *model, double gate, double dt_default, int64_t N, int64_t R, double *filt, double *nis,
                                uint8_t *flag, int32_t *status, void *stream) {
    if (!sm_sizes_ok(N, R) || !(gate >= 0.0) || !(dt_default > 0.0) || !(dt_default < INFINITY) || !status) return RN_EINVAL;
    if (N == 0) return RN_OK;
    if (!offsets || !order || !cols || !direction || !model || !filt || !nis || !flag) return RN_EINVAL;
    hipLaunchKernelGGL(sm_filter_kernel, dim3(rn_blocks(N, SM_THREADS)), dim3(SM_THREADS), 0, (hipStream_t)stream, offsets, order, cols,
                       direction, model, gate, dt_default, N, R, filt, nis, flag, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_smooth_rts(const int64_t *offsets, const int32_t *order, const double *cols, const int32_t *direction,
                             const double *model, double dt_default, int64_t N, int64_t R, const double *filt, double *out,
                             int32_t *status, void *stream) {
    if (!sm_sizes_ok(N, R) || !(dt_default > 0.0) || !(dt_default < INFINITY) || !status) return RN_EINVAL;
    if (N == 0) return RN_OK;
    if (!offsets || !order || !cols || !direction || !model || !filt || !out) return RN_EINVAL;
    hipLaunchKernelGGL(sm_rts_kernel, dim3(rn_blocks(N, SM_THREADS)), dim3(SM_THREADS), 0, (hipStream_t)stream, offsets, order, cols,
                       direction, model, dt_default, N, R, filt, out, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

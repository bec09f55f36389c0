// Smoothing-spline trajectories of the reference's annotator (seems_to_be_working.py): Annotator.create_trajectory (:1137-1314),
// get_splines (:1338-1350), gen_trajectories (:1317-1336), adjust_ts_with_trajectories (:1353-1458).
//
// The reference builds, per object, 200 + 100 scipy UnivariateSpline fits (FITPACK curfit, iopt = 0), one per smoothing factor,
// scores each and keeps the first with the smallest error.  Here:
//   sp_weights_kernel  one thread per box: the box's corners through its own camera (homography_dev.h, fp32 corners, fp64 image)
//                      and the two pixel-per-foot weights (:1186-1196).
//   sp_fit_kernel      one LANE per (object, axis, candidate); the 64 lanes of a wave are consecutive candidates of one
//                      (object, axis), so their loads of x, y, w are one address and their control flow stays close.  FITPACK's
//                      fpcurf restated: the least-squares polynomial, knot insertion (fpknot and the nplus rule), the banded
//                      weighted least squares by Givens rotations in row order (fpgivs / fprota / fpback), the discontinuity
//                      rows (fpdisc) and the rational search for p (fprati), with its ier outcomes.  The per-lane arrays live in
//                      a workspace interleaved by lane (element e of lane L at ws[e * NL + L]); the basis values are recomputed
//                      where FITPACK reads its m x (k+1) table q.
//   sp_select_kernel   one workgroup per (object, axis): every surviving candidate at the object's own timestamps, the score
//                      summed in ascending row order, the first smallest, the winner's t, c, n, ier, fp and error figures.
//   sp_eval_kernel     one thread per (spline, time): de Boor evaluation as FITPACK's splev, extrapolating the end intervals.
//   sp_shift_kernel    one wave per (frame, camera): lane j the j-th shifted time (lane `trials` the unshifted one), the error
//                      over the kept objects in ascending order, the first smallest.
//
// Early rejection: with iopt = 0 knots are only ever added, so a candidate whose knot count passes the reference's limit
// (np.floor(duration) * 4 + 2 for x, + 2 for y) can only end above it and the reference skips it (:1240, :1264).  A lane stops
// there, flagged RN_SPLINE_REJECTED, and the per-lane arrays are sized by that limit, not by m + k + 1.
//
// Arithmetic: fp64, one rounding per operation in FITPACK's order (this file is in the Makefile's EXACT list: no fma
// contraction).  Every index read from memory is checked before use; a bad table sets a bit of *status and the item is left
// out.  No kernel spins or asserts; memory is written by plain C++ stores.
#include <math.h>

#include "common.h"
#include "homography_dev.h"
#include "wave_dev.h"

#define SP_THREADS 256
#define SP_MAX ((int64_t)1 << 31)
#define SP_MAXIT 20

// a 1-based array with a stride: a lane's slice of the interleaved workspace (stride NL) or a packed row (stride 1)
struct SpArr {
    double *p;
    int64_t stride;
    __device__ __forceinline__ double &operator()(int i) const { return p[(int64_t)(i - 1) * stride]; }
};
struct SpCArr {
    const double *p;
    int64_t stride;
    __device__ __forceinline__ double operator()(int i) const { return p[(int64_t)(i - 1) * stride]; }
};

// fpbspl: the k + 1 non-zero B-splines of degree K at x on t(l) <= x < t(l+1) (violated on purpose when extrapolating)
template <int K, typename TA>
__device__ __forceinline__ void sp_bspl(const TA &t, double x, int l, double (&h)[K + 2]) {
    double hh[K + 1];
    h[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= K; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
#pragma unroll
        for (int i = 1; i <= j; ++i) {
            const double tli = t(l + i), tlj = t(l + i - j);
            if (tli == tlj) {
                h[i] = 0.0;
            } else {
                const double f = hh[i - 1] / (tli - tlj);
                h[i - 1] = h[i - 1] + f * (tli - x);
                h[i] = f * (x - tlj);
            }
        }
    }
}

// splev for one argument: the interval t(l) <= x < t(l+1) inside [k+1, n-k-1], clamped at both ends (extrapolation)
template <int K, typename TA, typename CA>
__device__ __forceinline__ double sp_value(const TA &t, const CA &c, int n, double x) {
    const int k1 = K + 1, nk1 = n - k1;
    int l = k1;
    while (!(x < t(l + 1) || l == nk1)) ++l;
    double h[K + 2];
    sp_bspl<K>(t, x, l, h);
    double sp = 0.0;
#pragma unroll
    for (int j = 1; j <= k1; ++j) sp = sp + c(l - k1 + j) * h[j - 1];
    return sp;
}

__device__ __forceinline__ void sp_givs(double piv, double &ww, double &cs, double &sn) {
    const double store = fabs(piv);
    double dd;
    if (store >= ww) {
        const double r = ww / piv;
        dd = store * sqrt(1.0 + r * r);
    } else {
        const double r = piv / ww;
        dd = ww * sqrt(1.0 + r * r);
    }
    cs = ww / dd;
    sn = piv / dd;
    ww = dd;
}

__device__ __forceinline__ void sp_rota(double cs, double sn, double &a, double &b) {
    const double s1 = a, s2 = b;
    b = cs * s2 + sn * s1;
    a = cs * s1 - sn * s2;
}

// Fortran's int(x) as the reference's build computes it (cvttsd2si): out of range or NaN -> the most negative integer
__device__ __forceinline__ int sp_int(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return INT32_MIN;
    return (int)v;
}

struct SpLane {
    double *ws;
    int64_t NL;
    int N;
    __device__ __forceinline__ SpArr arr(int col) const { return SpArr{ws + (int64_t)col * N * NL, NL}; }
};
// columns of the per-lane workspace, each N = ncap doubles: t, c, z, fpint, nrdata, a (4), g (5), b (5)
#define SP_COL_T 0
#define SP_COL_C 1
#define SP_COL_Z 2
#define SP_COL_FPINT 3
#define SP_COL_NRD 4
#define SP_COL_A 5
#define SP_COL_G 9
#define SP_COL_B 14
#define SP_COLS RN_SPLINE_WS_COLS

// the sum of (w (s(x) - y))^2 with FITPACK's two interval counters: `l` (one step per point, picks the coefficients) and `lq`
// (the search of the least-squares pass, picks the basis values that FITPACK keeps in q)
template <int K, bool FPINT>
__device__ __forceinline__ double sp_residual(const SpArr &T, const SpArr &C, const SpArr &FP, const double *x, const double *y,
                                              const double *w, int m, int nk1, int nrint) {
    const int k1 = K + 1, k2 = K + 2;
    double fpart = 0.0;
    int i = 1, l = k2, lq = k1, nw = 0;
    for (int it = 1; it <= m; ++it) {
        const double xi = x[it - 1];
        if (!(xi < T(l) || l > nk1)) {
            nw = 1;
            ++l;
        }
        while (!(xi < T(lq + 1) || lq == nk1)) ++lq;
        double h[K + 2];
        sp_bspl<K>(T, xi, lq, h);
        double term = 0.0;
#pragma unroll
        for (int j = 1; j <= k1; ++j) term = term + C(l - k2 + j) * h[j - 1];
        const double d = w[it - 1] * (term - y[it - 1]);
        term = d * d;
        fpart = fpart + term;
        if (FPINT && nw) {
            const double store = term * 0.5;
            FP(i) = fpart - store;
            ++i;
            fpart = store;
        }
        nw = 0;
    }
    if (FPINT) FP(nrint) = fpart;
    return fpart;
}

// fpback: a is n x kb banded upper triangular
template <int KB>
__device__ __forceinline__ void sp_back(const SpLane &L, int acol, const SpArr &Z, int n, const SpArr &C) {
    const SpArr a1 = L.arr(acol);
    C(n) = Z(n) / a1(n);
    int i = n - 1;
    for (int j = 2; j <= n; ++j) {
        double store = Z(i);
        const int i1 = j <= KB - 1 ? j - 1 : KB - 1;
        int mm = i;
        for (int l = 1; l <= i1; ++l) {
            ++mm;
            store = store - C(mm) * L.arr(acol + l)(i);
        }
        C(i) = store / a1(i);
        --i;
    }
}

template <int K>
__device__ void sp_fit(const SpLane &L, const double *x, const double *y, const double *w, int m, double s, int ncap, int &n_out,
                       int &ier_out, double &fp_out, int &iters_out) {
    constexpr int k1 = K + 1, k2 = K + 2, nmin = 2 * k1;
    // UnivariateSpline calls fpcurf with nest = max(m / 2, 2k + 2) and, on ier = 1, again with iopt = 1 and nest = m + k + 1
    // (_reset_nest).  The second call finds the same knots and sums, but it enters with ier = 1, so the next round adds ONE
    // knot instead of what the nplus rule gives; and a batch of new knots stops at the first nest.
    const int nmax = m + k1, nest_full = nmax > 2 * K + 3 ? nmax : 2 * K + 3;
    int nest = m / 2 > nmin ? m / 2 : nmin;
    const SpArr T = L.arr(SP_COL_T), C = L.arr(SP_COL_C), Z = L.arr(SP_COL_Z), FP = L.arr(SP_COL_FPINT), NRD = L.arr(SP_COL_NRD);
    const double acc = 1e-3 * s, xb = x[0], xe = x[m - 1];
    int n = nmin, ier = 0, nplus = 0, iters = 0, nk1 = 0, nrint = 0;
    double fp = 0.0, fpold = 0.0, fp0 = 0.0, fpms = 0.0;
    NRD(1) = (double)(m - 2);
    bool done = false;
    for (bool again = true; again && !done;) {                                  // label 60, entered again after label 10
        again = false;
        for (int iter = 1; iter <= m; ++iter) {
            ++iters;
            if (n == nmin) ier = -2;
            nrint = n - nmin + 1;
            nk1 = n - k1;
            for (int j = 1, i = n; j <= k1; ++j, --i) {
                T(j) = xb;
                T(i) = xe;
            }
            fp = 0.0;
            for (int i = 1; i <= nk1; ++i) {
                Z(i) = 0.0;
#pragma unroll
                for (int j = 0; j < k1; ++j) L.arr(SP_COL_A + j)(i) = 0.0;
            }
            int l = k1;
            for (int it = 1; it <= m; ++it) {
                const double xi = x[it - 1], wi = w[it - 1];
                double yi = y[it - 1] * wi;
                while (!(xi < T(l + 1) || l == nk1)) ++l;
                double h[K + 2];
                sp_bspl<K>(T, xi, l, h);
#pragma unroll
                for (int i = 0; i < k1; ++i) h[i] = h[i] * wi;
                int j = l - k1;
#pragma unroll
                for (int i = 1; i <= k1; ++i) {
                    ++j;
                    const double piv = h[i - 1];
                    if (piv == 0.0) continue;
                    double cs, sn;
                    sp_givs(piv, L.arr(SP_COL_A)(j), cs, sn);
                    sp_rota(cs, sn, yi, Z(j));
#pragma unroll
                    for (int i1 = i + 1; i1 <= k1; ++i1) sp_rota(cs, sn, h[i1 - 1], L.arr(SP_COL_A + i1 - i)(j));
                }
                fp = fp + yi * yi;
            }
            if (ier == -2) fp0 = fp;
            FP(n) = fp0;
            FP(n - 1) = fpold;
            NRD(n) = (double)nplus;
            sp_back<k1>(L, SP_COL_A, Z, nk1, C);
            fpms = fp - s;
            if (fabs(fpms) < acc) { done = true; break; }
            if (fpms < 0.0) break;                                              // part 2
            if (n == nmax) { ier = -1; done = true; break; }
            if (n == nest) {
                if (nest == nest_full) { ier = 1; done = true; break; }
                nest = nest_full;
                if (n != nmin) ier = 1;
            }
            if (ier == 0) {
                int npl1 = nplus * 2;
                const double rn = (double)nplus;
                if (fpold - fp > acc) npl1 = sp_int(rn * fpms / (fpold - fp));
                int mx = npl1 > nplus / 2 ? npl1 : nplus / 2;
                mx = mx > 1 ? mx : 1;
                nplus = nplus * 2 < mx ? nplus * 2 : mx;
            } else {
                nplus = 1;
                ier = 0;
            }
            fpold = fp;
            sp_residual<K, true>(T, C, FP, x, y, w, m, nk1, nrint);
            for (int lp = 1; lp <= nplus; ++lp) {
                if (n >= ncap) { ier = RN_SPLINE_REJECTED; done = true; break; }    // one more knot passes the limit
                // fpknot
                double fpmax = 0.0;
                int jbegin = 1, number = 0, maxpt = 0, maxbeg = 0;
                for (int j = 1; j <= nrint; ++j) {
                    const int jpoint = (int)NRD(j);
                    const double fj = FP(j);
                    if (!(fpmax >= fj || jpoint == 0)) {
                        fpmax = fj;
                        number = j;
                        maxpt = jpoint;
                        maxbeg = jbegin;
                    }
                    jbegin = jbegin + jpoint + 1;
                }
                const int ihalf = maxpt / 2 + 1, nrx = maxbeg + ihalf, next = number + 1;
                if (number == 0 || nrx < 1 || nrx > m) { ier = RN_SPLINE_STUCK; done = true; break; }   // FITPACK reads an unset index here
                for (int j = next; j <= nrint; ++j) {
                    const int jj = next + nrint - j;
                    FP(jj + 1) = FP(jj);
                    NRD(jj + 1) = NRD(jj);
                    T(jj + K + 1) = T(jj + K);
                }
                NRD(number) = (double)(ihalf - 1);
                NRD(next) = (double)(maxpt - ihalf);
                const double am = (double)maxpt;
                FP(number) = fpmax * (double)(ihalf - 1) / am;
                FP(next) = fpmax * (double)(maxpt - ihalf) / am;
                T(next + K) = x[nrx - 1];
                ++n;
                ++nrint;
                if (n == nmax) {                                                // label 10: the knots of the interpolating spline
                    const int mk1 = m - k1;
                    int i = k2, j = K / 2 + 2;
                    for (int q = 1; q <= mk1; ++q, ++i, ++j) T(i) = (K & 1) ? x[j - 1] : (x[j - 1] + x[j - 2]) * 0.5;
                    again = true;
                    break;
                }
                if (n == nest) break;
            }
            if (done || again) break;
        }
    }
    if (!done && ier != -2) {
        // part 2: the smoothing spline sp(x) with f(p) = s
        const int n8 = n - nmin;
        {   // fpdisc
            const double fac = (double)(nk1 - K) / (T(nk1 + 1) - T(k1));
            for (int l = k2; l <= nk1; ++l) {
                const int lmk = l - k1;
                double h[2 * k1];
#pragma unroll
                for (int j = 1; j <= k1; ++j) {
                    h[j - 1] = T(l) - T(l + j - k2);
                    h[j + k1 - 1] = T(l) - T(l + j);
                }
                int lp = lmk;
#pragma unroll
                for (int j = 1; j <= k2; ++j) {
                    double prod = h[j - 1];
#pragma unroll
                    for (int i = 1; i <= K; ++i) prod = prod * h[j + i - 1] * fac;
                    L.arr(SP_COL_B + j - 1)(lmk) = (T(lp + k1) - T(lp)) / prod;
                    ++lp;
                }
            }
        }
        double p1 = 0.0, f1 = fp0 - s, p3 = -1.0, f3 = fpms, p = 0.0;
        for (int i = 1; i <= nk1; ++i) p = p + L.arr(SP_COL_A)(i);
        p = (double)nk1 / p;
        int ich1 = 0, ich3 = 0;
        const double con1 = 0.1, con9 = 0.9, con4 = 0.04;
        ier = 3;                                                                // what is left when the loop runs out
        for (int iter = 1; iter <= SP_MAXIT; ++iter) {
            ++iters;
            const double pinv = 1.0 / p;
            for (int i = 1; i <= nk1; ++i) {
                C(i) = Z(i);
                L.arr(SP_COL_G + k1)(i) = 0.0;
#pragma unroll
                for (int j = 0; j < k1; ++j) L.arr(SP_COL_G + j)(i) = L.arr(SP_COL_A + j)(i);
            }
            for (int it = 1; it <= n8; ++it) {
                double h[k2 + 1];
#pragma unroll
                for (int i = 0; i < k2; ++i) h[i] = L.arr(SP_COL_B + i)(it) * pinv;
                double yi = 0.0;
                for (int j = it; j <= nk1; ++j) {
                    const double piv = h[0];
                    double cs, sn;
                    sp_givs(piv, L.arr(SP_COL_G)(j), cs, sn);
                    sp_rota(cs, sn, yi, C(j));
                    if (j == nk1) break;
                    const int i2 = j > n8 ? nk1 - j : k1;
#pragma unroll
                    for (int i = 1; i <= k1; ++i) {
                        if (i <= i2) {
                            sp_rota(cs, sn, h[i], L.arr(SP_COL_G + i)(j));
                            h[i - 1] = h[i];
                        }
                    }
#pragma unroll
                    for (int i = 0; i <= k1; ++i)
                        if (i == i2) h[i] = 0.0;
                }
            }
            sp_back<k2>(L, SP_COL_G, C, nk1, C);
            fp = sp_residual<K, false>(T, C, FP, x, y, w, m, nk1, nrint);
            fpms = fp - s;
            if (fabs(fpms) < acc) { ier = 0; break; }
            if (iter == SP_MAXIT) break;                                        // ier = 3
            const double p2 = p, f2 = fpms;
            if (ich3 == 0) {
                if (!(f2 - f3 > acc)) {                                         // the initial choice of p is too large
                    p3 = p2;
                    f3 = f2;
                    p = p * con4;
                    if (p <= p1) p = p1 * con9 + p2 * con1;
                    continue;
                }
                if (f2 < 0.0) ich3 = 1;
            }
            if (ich1 == 0) {
                if (!(f1 - f2 > acc)) {                                         // the initial choice of p is too small
                    p1 = p2;
                    f1 = f2;
                    p = p / con4;
                    if (p3 < 0.0) continue;
                    if (p >= p3) p = p2 * con1 + p3 * con9;
                    continue;
                }
                if (f2 > 0.0) ich1 = 1;
            }
            if (f2 >= f1 || f2 <= f3) { ier = 2; break; }
            // fprati
            if (p3 > 0.0) {
                const double h1 = f1 * (f2 - f3), h2 = f2 * (f3 - f1), h3 = f3 * (f1 - f2);
                p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3);
            } else {
                p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3);
            }
            if (f2 < 0.0) {
                p3 = p2;
                f3 = f2;
            } else {
                p1 = p2;
                f1 = f2;
            }
        }
    }
    n_out = n;
    ier_out = ier;
    fp_out = fp;
    iters_out = iters;
}

// grp int32 [G, RN_SPLINE_GRP]: row0, m, k, ncap, cand0, ncand, wave0, axis (0: x, 1: y)
struct SpGroup {
    int row0, m, k, ncap, cand0, ncand, wave0, axis;
};
__device__ __forceinline__ bool sp_group(const int32_t *__restrict__ grp, int64_t g, int64_t R, int64_t NC, int64_t NW, int N, SpGroup &o) {
    const int32_t *r = grp + g * RN_SPLINE_GRP;
    o.row0 = r[0]; o.m = r[1]; o.k = r[2]; o.ncap = r[3]; o.cand0 = r[4]; o.ncand = r[5]; o.wave0 = r[6]; o.axis = r[7];
    return (o.axis == 0 || o.axis == 1) && (o.k == 2 || o.k == 3) && o.m >= o.k + 1 && o.row0 >= 0 && (int64_t)o.row0 + o.m <= R && o.ncap >= 2 * o.k + 2 &&
           o.ncap <= N && o.ncap <= o.m + o.k + 1 && o.cand0 >= 0 && o.ncand >= 0 && (int64_t)o.cand0 + o.ncand <= NC && o.wave0 >= 0 &&
           (int64_t)o.wave0 + (o.ncand + RN_WAVE - 1) / RN_WAVE <= NW;
}

__global__ void __launch_bounds__(RN_WAVE) sp_fit_kernel(const int32_t *__restrict__ grp, int64_t G, const int32_t *__restrict__ waves,
                                                         int64_t NW, const double *__restrict__ tx, const double *__restrict__ val,
                                                         const double *__restrict__ wt, int64_t R, const double *__restrict__ sfac,
                                                         int64_t NC, int N, double *__restrict__ ws, int32_t *__restrict__ out_n,
                                                         int32_t *__restrict__ out_ier, double *__restrict__ out_fp,
                                                         int32_t *__restrict__ out_iter, int32_t *__restrict__ status) {
    const int64_t wv = blockIdx.x, NL = NW * RN_WAVE, lane = wv * RN_WAVE + threadIdx.x;
    const int g = waves[wv * 2], c0 = waves[wv * 2 + 1];
    out_n[lane] = 0;
    out_ier[lane] = RN_SPLINE_UNUSED;
    out_fp[lane] = 0.0;
    out_iter[lane] = 0;
    SpGroup q;
    if (g < 0 || g >= G || !sp_group(grp, g, R, NC, NW, N, q) || c0 < 0 || c0 % RN_WAVE || q.wave0 + c0 / RN_WAVE != wv) {
        if (threadIdx.x == 0) rn_flag(status, RN_SPLINE_BAD_TABLE);
        return;
    }
    const int c = c0 + (int)threadIdx.x;
    if (c >= q.ncand) return;
    const double s = sfac[q.cand0 + c];
    const SpLane L{ws + lane, NL, N};
    int n, ier, iters;
    double fp;
    if (q.k == 2) sp_fit<2>(L, tx + q.row0, val + q.row0, wt + q.row0, q.m, s, q.ncap, n, ier, fp, iters);
    else sp_fit<3>(L, tx + q.row0, val + q.row0, wt + q.row0, q.m, s, q.ncap, n, ier, fp, iters);
    out_n[lane] = n;
    out_ier[lane] = ier;
    out_fp[lane] = fp;
    out_iter[lane] = iters;
}

template <typename TA, typename CA>
__device__ __forceinline__ double sp_value_k(int k, const TA &t, const CA &c, int n, double x) {
    return k == 2 ? sp_value<2>(t, c, n, x) : sp_value<3>(t, c, n, x);
}

// metric 0 ("ape"): sqrt(mean); otherwise sqrt(max) on the x axis and the plain max on the y axis, :1252, :1275
__device__ __forceinline__ double sp_score(double sum, double mx, int m, int metric, int axis) {
    if (metric == 0) return sqrt(sum / (double)m);
    return axis == 0 ? sqrt(mx) : mx;
}

__global__ void __launch_bounds__(SP_THREADS) sp_select_kernel(const int32_t *__restrict__ grp, int64_t G, const double *__restrict__ tx,
                                                               const double *__restrict__ val, const double *__restrict__ wt,
                                                               const double *__restrict__ wsc, int64_t R, int64_t NC, int64_t NW, int N,
                                                               const double *__restrict__ ws, const int32_t *__restrict__ out_n,
                                                               const int32_t *__restrict__ out_ier, const double *__restrict__ out_fp,
                                                               int metric, double *__restrict__ scores, int32_t *__restrict__ win,
                                                               double *__restrict__ wfig, double *__restrict__ wt_out,
                                                               double *__restrict__ wc_out, int32_t *__restrict__ status) {
    __shared__ double s_best[SP_THREADS / RN_WAVE];
    __shared__ int s_idx[SP_THREADS / RN_WAVE];
    const int64_t g = blockIdx.x, NL = NW * RN_WAVE;
    const int tid = threadIdx.x;
    SpGroup q;
    if (!sp_group(grp, g, R, NC, NW, N, q)) {
        if (tid == 0) {
            rn_flag(status, RN_SPLINE_BAD_TABLE);
            win[g * 3] = -1; win[g * 3 + 1] = 0; win[g * 3 + 2] = RN_SPLINE_UNUSED;
        }
        return;
    }
    const double *x = tx + q.row0, *y = val + q.row0, *w2 = wsc + q.row0, *w = wt + q.row0;
    double best = INFINITY;
    int bidx = RN_NO_INDEX;
    for (int c = tid; c < q.ncand; c += SP_THREADS) {
        const int64_t lane = (int64_t)q.wave0 * RN_WAVE + c;
        const int n = out_n[lane], ier = out_ier[lane];
        double sc = NAN;
        if (ier <= 3 && n >= 2 * q.k + 2 && n <= q.ncap) {
            const SpCArr T{ws + lane, NL}, C{ws + (int64_t)N * NL + lane, NL};
            if (!isnan(sp_value_k(q.k, T, C, n, 0.0))) {                        // :1238
                double sum = 0.0, mx = -INFINITY;
                for (int i = 0; i < q.m; ++i) {
                    const double d = w2[i] * (sp_value_k(q.k, T, C, n, x[i]) - y[i]);
                    const double e = d * d;
                    sum = sum + e;
                    mx = (e > mx || isnan(e)) ? e : mx;                         // np.max: NaN propagates
                    if (isnan(mx)) break;
                }
                sc = isnan(mx) ? NAN : sp_score(sum, mx, q.m, metric, q.axis);
            }
        }
        scores[q.cand0 + c] = sc;
        if (sc < best) {
            best = sc;
            bidx = c;
        }
    }
    block_arg_first<SP_THREADS / RN_WAVE>(best, bidx, rn_lt_first<double>(), s_best, s_idx);
    const int wi = bidx;
    const bool found = wi != RN_NO_INDEX;
    const int64_t lane = (int64_t)q.wave0 * RN_WAVE + (found ? wi : 0);
    const int n = found ? out_n[lane] : 0;
    for (int i = tid; i < N; i += SP_THREADS) {
        wt_out[g * N + i] = (found && i < n) ? ws[(int64_t)i * NL + lane] : 0.0;
        wc_out[g * N + i] = (found && i < n - q.k - 1) ? ws[((int64_t)N + i) * NL + lane] : 0.0;   // c(n-k .. n) is never written
    }
    if (tid == 0) {
        win[g * 3] = found ? wi : -1;
        win[g * 3 + 1] = n;
        win[g * 3 + 2] = found ? out_ier[lane] : RN_SPLINE_UNUSED;
        double *f = wfig + g * RN_SPLINE_FIGS;
        f[0] = found ? out_fp[lane] : NAN;
        f[1] = found ? best : NAN;
        double se = 0.0, pe = 0.0, mx = -INFINITY;
        if (found) {
            const SpCArr T{ws + lane, NL}, C{ws + (int64_t)N * NL + lane, NL};
            for (int i = 0; i < q.m; ++i) {                                     // :1282-1294
                const double r = sp_value_k(q.k, T, C, n, x[i]) - y[i];
                const double d = w[i] * r, e = d * d;
                se = se + r * r;
                pe = pe + e;
                mx = (e > mx || isnan(e)) ? e : mx;
            }
        }
        f[2] = found ? sqrt(se / (double)q.m) : NAN;
        f[3] = found ? sqrt(pe / (double)q.m) : NAN;
        f[4] = found ? sqrt(mx) : NAN;
    }
}

// splines packed: st, sc fp64 [S, N], snk int32 [S, 2] = (n, k); n = 0: no spline (NaN)
__device__ __forceinline__ bool sp_packed(const int32_t *__restrict__ snk, int64_t S, int N, int64_t s, int &n, int &k) {
    if (s < 0 || s >= S) return false;
    n = snk[s * 2];
    k = snk[s * 2 + 1];
    return (k == 2 || k == 3) && n >= 2 * k + 2 && n <= N;
}

__global__ void sp_eval_kernel(const double *__restrict__ st, const double *__restrict__ sc, const int32_t *__restrict__ snk, int64_t S,
                               int N, const int32_t *__restrict__ qs, const double *__restrict__ qt, int64_t Q, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= Q) return;
    const int64_t s = qs[i];
    int n, k;
    double v = NAN;
    if (sp_packed(snk, S, N, s, n, k)) v = sp_value_k(k, SpCArr{st + s * N, 1}, SpCArr{sc + s * N, 1}, n, qt[i]);
    out[i] = v;
}

// one wave per (frame, camera) entry: rows [off[e], off[e+1]) = its kept objects in ascending id: rs the spline, rx the label x
__global__ void __launch_bounds__(SP_THREADS) sp_shift_kernel(const double *__restrict__ st, const double *__restrict__ sc,
                                                              const int32_t *__restrict__ snk, int64_t S, int N,
                                                              const int64_t *__restrict__ off, const int32_t *__restrict__ rs,
                                                              const double *__restrict__ rx, int64_t E, int64_t Rr,
                                                              const double *__restrict__ base, const double *__restrict__ run,
                                                              const double *__restrict__ shifts, int trials, int use_run, int metric,
                                                              double *__restrict__ best_t, double *__restrict__ errs,
                                                              int32_t *__restrict__ best_i, int32_t *__restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * (SP_THREADS / RN_WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= E) return;
    const int64_t lo = off[e], hi = off[e + 1];
    if (!(lo >= 0 && lo < hi && hi <= Rr)) {
        if (lane == 0) {
            rn_flag(status, RN_SPLINE_BAD_TABLE);
            best_t[e] = NAN; errs[e * 2] = NAN; errs[e * 2 + 1] = NAN; best_i[e] = -1;
        }
        return;
    }
    const double ts = base[e];
    double time = ts, err = NAN;
    if (lane <= trials) {
        if (lane < trials) {
            time = ts + shifts[lane];                                          // :1425-1427
            if (use_run) time = time + run[e];
        }
        double sum = 0.0, mx = -INFINITY;
        bool bad = false;
        for (int64_t r = lo; r < hi; ++r) {
            int n, k;
            if (!sp_packed(snk, S, N, rs[r], n, k)) { bad = true; break; }
            const int64_t s = rs[r];
            const float xs = (float)sp_value_k(k, SpCArr{st + s * N, 1}, SpCArr{sc + s * N, 1}, n, time);   // torch.tensor of floats: fp32
            const double d = (double)xs - rx[r], q = d * d;
            sum = sum + q;
            mx = (q > mx || isnan(q)) ? q : mx;
        }
        if (bad) rn_flag(status, RN_SPLINE_BAD_TABLE);
        else err = (metric == 0 || lane == trials) ? sqrt(sum / (double)(hi - lo)) : sqrt(mx);
    }
    const double init = __shfl(err, trials, RN_WAVE);
    double best = (lane < trials && err < INFINITY) ? err : INFINITY;
    int bi = (lane < trials && err < INFINITY) ? lane : RN_NO_INDEX;
    wave_arg_first(best, bi, rn_lt_first<double>());
    const double tbest = __shfl(time, bi == RN_NO_INDEX ? trials : bi, RN_WAVE);
    if (lane == 0) {
        best_t[e] = tbest;
        errs[e * 2] = best;
        errs[e * 2 + 1] = init;
        best_i[e] = bi == RN_NO_INDEX ? -1 : bi;
    }
}

// :1186-1196: out [n,4] = (x_weight, y_weight, x_diff, y_diff)
__global__ void sp_weights_kernel(const double *__restrict__ state6, const int32_t *__restrict__ cam, int64_t n,
                                  const double *__restrict__ P1, const double *__restrict__ P2, int n_cam, double *__restrict__ out,
                                  int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int m = cam[i];
    if (m < 0 || m >= n_cam) {
        rn_flag(status, RN_LABEL_BAD_CAMERA);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[i * 4 + k] = NAN;
        return;
    }
    float s[6], x[8], y[8], z[8];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = (float)state6[i * 6 + k];                // boxes.float()
    state_corners(s, x, y, z);
    double2 im[8];
    hg_project_to_im(x, y, z, P1, P2, m, im);
    // torch.mean over the two corner differences, then the norm
    const double yu = ((im[0].x - im[1].x) + (im[2].x - im[3].x)) / 2.0, yv = ((im[0].y - im[1].y) + (im[2].y - im[3].y)) / 2.0;
    const double xu = ((im[0].x - im[2].x) + (im[1].x - im[3].x)) / 2.0, xv = ((im[0].y - im[2].y) + (im[1].y - im[3].y)) / 2.0;
    const double y_diff = sqrt(yu * yu + yv * yv), x_diff = sqrt(xu * xu + xv * xv);
    out[i * 4] = x_diff / state6[i * 6 + 2];
    out[i * 4 + 1] = y_diff / state6[i * 6 + 3];
    out[i * 4 + 2] = x_diff;
    out[i * 4 + 3] = y_diff;
}

extern "C" int64_t rn_spline_fit_workspace_bytes(int64_t n_waves, int ncap) {
    if (n_waves < 0 || ncap < 0) return -1;
    return n_waves * RN_WAVE * (int64_t)ncap * SP_COLS * (int64_t)sizeof(double);
}

extern "C" int rn_label_box_weights(const double *state6, const int32_t *cam, int64_t n, const double *P1, const double *P2, int n_cam,
                                    double *out, int32_t *status, void *stream) {
    if (n < 0 || n >= SP_MAX || n_cam <= 0 || n_cam > RN_LABEL_MAX_CAMS || !status) return RN_EINVAL;
    if (n == 0) return RN_OK;
    if (!state6 || !cam || !P1 || !out) return RN_EINVAL;
    hipLaunchKernelGGL(sp_weights_kernel, dim3(rn_blocks(n, SP_THREADS)), dim3(SP_THREADS), 0, (hipStream_t)stream, state6, cam, n, P1, P2,
                       n_cam, out, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_spline_fit(const int32_t *grp, int64_t G, const int32_t *waves, int64_t NW, const double *tx, const double *val,
                             const double *wt, int64_t R, const double *s, int64_t NC, int ncap, void *workspace, int32_t *out_n,
                             int32_t *out_ier, double *out_fp, int32_t *out_iter, int32_t *status, void *stream) {
    if (G < 0 || NW < 0 || R < 0 || NC < 0 || G >= SP_MAX || NW >= SP_MAX / RN_WAVE || R >= SP_MAX || NC >= SP_MAX || ncap < 6 ||
        ncap > RN_SPLINE_MAX_NCAP || !status)
        return RN_EINVAL;
    if (NW == 0) return RN_OK;
    if (!grp || !waves || !tx || !val || !wt || !s || !workspace || !out_n || !out_ier || !out_fp || !out_iter) return RN_EINVAL;
    hipLaunchKernelGGL(sp_fit_kernel, dim3((unsigned)NW), dim3(RN_WAVE), 0, (hipStream_t)stream, grp, G, waves, NW, tx, val, wt, R, s, NC,
                       ncap, reinterpret_cast<double *>(workspace), out_n, out_ier, out_fp, out_iter, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_spline_select(const int32_t *grp, int64_t G, const double *tx, const double *val, const double *wt, const double *wscore,
                                int64_t R, int64_t NC, int64_t NW, int ncap, const void *workspace, const int32_t *out_n,
                                const int32_t *out_ier, const double *out_fp, int metric, double *scores, int32_t *win, double *wfig,
                                double *wt_out, double *wc_out, int32_t *status, void *stream) {
    if (G < 0 || NW < 0 || R < 0 || NC < 0 || G >= SP_MAX || NW >= SP_MAX / RN_WAVE || R >= SP_MAX || NC >= SP_MAX || ncap < 6 ||
        ncap > RN_SPLINE_MAX_NCAP || metric < 0 || metric > 1 || !status)
        return RN_EINVAL;
    if (G == 0) return RN_OK;
    if (!grp || !tx || !val || !wt || !wscore || !workspace || !out_n || !out_ier || !out_fp || !win || !wfig || !wt_out || !wc_out ||
        (NC > 0 && !scores))
        return RN_EINVAL;
    hipLaunchKernelGGL(sp_select_kernel, dim3((unsigned)G), dim3(SP_THREADS), 0, (hipStream_t)stream, grp, G, tx, val, wt, wscore, R, NC, NW,
                       ncap, reinterpret_cast<const double *>(workspace), out_n, out_ier, out_fp, metric, scores, win, wfig, wt_out, wc_out,
                       status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_spline_eval(const double *st, const double *sc, const int32_t *snk, int64_t S, int ncap, const int32_t *qs,
                              const double *qt, int64_t Q, double *out, void *stream) {
    if (S < 0 || Q < 0 || S >= SP_MAX || Q >= SP_MAX * SP_THREADS || ncap < 6 || ncap > RN_SPLINE_MAX_NCAP) return RN_EINVAL;
    if (Q == 0) return RN_OK;
    if (!qs || !qt || !out || (S > 0 && (!st || !sc || !snk))) return RN_EINVAL;
    hipLaunchKernelGGL(sp_eval_kernel, dim3(rn_blocks(Q, SP_THREADS)), dim3(SP_THREADS), 0, (hipStream_t)stream, st, sc, snk, S, ncap, qs, qt,
                       Q, out);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_label_ts_shift(const double *st, const double *sc, const int32_t *snk, int64_t S, int ncap, const int64_t *off,
                                 const int32_t *rs, const double *rx, int64_t E, int64_t Rr, const double *base, const double *run,
                                 const double *shifts, int trials, int use_run, int metric, double *best_t, double *errs, int32_t *best_i,
                                 int32_t *status, void *stream) {
    if (S < 0 || E < 0 || Rr < 0 || S >= SP_MAX || E >= SP_MAX || Rr >= SP_MAX || ncap < 6 || ncap > RN_SPLINE_MAX_NCAP || trials < 1 ||
        trials >= RN_WAVE || metric < 0 || metric > 1 || !status)
        return RN_EINVAL;
    if (E == 0) return RN_OK;
    if (!st || !sc || !snk || !off || !rs || !rx || !base || !run || !shifts || !best_t || !errs || !best_i) return RN_EINVAL;
    hipLaunchKernelGGL(sp_shift_kernel, dim3(rn_blocks(E, SP_THREADS / RN_WAVE)), dim3(SP_THREADS), 0, (hipStream_t)stream, st, sc, snk, S,
                       ncap, off, rs, rx, E, Rr, base, run, shifts, trials, use_run, metric, best_t, errs, best_i, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

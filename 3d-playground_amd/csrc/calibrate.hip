// Camera calibration on device: the set-up half of homography.py.
//
//   rn_vanishing_points  find_vanishing_point             homography.py:96-154    one workgroup per line set
//   rn_hg_reproj_error   test_transformation's arithmetic homography.py:581-587   one workgroup per candidate scale
//   rn_hg_scale_z        scale_Z, the whole search        homography.py:607-666   one workgroup iterating
//   rn_fit_homography    cv2.findHomography(src, dst)     homography.py:354-355   one workgroup per problem (parity unpinned)
//
// All arithmetic is fp64 in the reference's order (this file is built with -ffp-contract=off) except where the reference's
// own tensors are fp32: the state and its corners, through homography_dev.h.  No atomics, no host synchronisation; every
// reduction has a fixed order, restated in tests/calib_cases.py.
#include "common.h"
#include "homography_dev.h"
#include "wave_dev.h"

#define CAL_BLOCK 256
#define VP_LEVELS 16
#define VP_MAX_AXIS 32

// ------------------------------------------------------------------------------------------------ vanishing points
// np.arange(p - g*15, p + g*15, g): length ceil((stop - start) / g); element 0 is start, element 1 start + g, element i
// start + i * delta with delta = element 1 - element 0 (numpy's fill), which is not g once start + g has rounded.
struct vp_axis_t { double start, second, delta; int n; };

__device__ __forceinline__ vp_axis_t vp_axis(double p, double g) {
    vp_axis_t a;
    a.start = p - g * 15.0;
    const double stop = p + g * 15.0;
    const double q = ceil((stop - a.start) / g);
    a.second = a.start + g;
    a.delta = a.second - a.start;
    a.n = !(q > 0.0) ? 0 : (q > (double)VP_MAX_AXIS ? VP_MAX_AXIS + 1 : (int)q);
    return a;
}
__device__ __forceinline__ double vp_elem(const vp_axis_t &a, int i) {
    return i == 0 ? a.start : (i == 1 ? a.second : a.start + (double)i * a.delta);
}

__global__ __launch_bounds__(CAL_BLOCK) void vanishing_points_kernel(const double *__restrict__ lines,
                                                                     const int64_t *__restrict__ offsets, int64_t rows,
                                                                     double *__restrict__ out, double *__restrict__ trace,
                                                                     int32_t *__restrict__ status) {
    __shared__ double sh_d[CAL_BLOCK / RN_WAVE];
    __shared__ int sh_i[CAL_BLOCK / RN_WAVE];
    const int s = blockIdx.x, t = threadIdx.x;
    const int64_t lo = offsets[s], n = offsets[s + 1] - lo;
    double *o = out + (int64_t)s * 3;
    if (lo < 0 || n < 0 || lo > rows - n) {                                     // a row range outside lines: nothing is read
        if (t == 0) { o[0] = o[1] = __builtin_nan(""); o[2] = __builtin_inf(); status[s] = RN_VP_BAD_OFFSETS; }
        return;
    }
    const double *L = lines + lo * 4;
    if (n < 2) {                                                                // lines[1]: IndexError in the reference
        if (t == 0) { o[0] = o[1] = __builtin_nan(""); o[2] = __builtin_inf(); status[s] = RN_VP_FEW_LINES; }
        return;
    }
    // homography.py:113-122 as written, precedence slips included
    const double a = (L[3] - L[1]) / L[2] - L[0];
    const double b = (L[7] - L[5]) / L[6] - L[4];
    const double c = L[1] - a * L[0];
    const double d = L[5] - c * L[4];
    double px = (d - c) / (a - b);
    double py = a * (d - c) / (a - b) + c;
    double best = __builtin_inf();
    int st = 0;
    if (!isfinite(px) || !isfinite(py)) {                                       // np.arange raises on such a start
        if (t == 0) { o[0] = px; o[1] = py; o[2] = best; status[s] = RN_VP_BAD_START; }
        return;
    }
    double g = 1e16;
    for (int lvl = 0; lvl < VP_LEVELS; ++lvl) {
        if (t == 0) {
            double *tr = trace + ((int64_t)s * VP_LEVELS + lvl) * 3;
            tr[0] = px; tr[1] = py; tr[2] = best;
        }
        vp_axis_t ax = vp_axis(px, g), ay = vp_axis(py, g);
        if (ax.n > VP_MAX_AXIS || ay.n > VP_MAX_AXIS) {
            st |= RN_VP_LONG_AXIS;
            ax.n = min(ax.n, VP_MAX_AXIS);
            ay.n = min(ay.n, VP_MAX_AXIS);
        }
        const int cells = ax.n * ay.n;                                          // <= 1024; scan index = ix * ny + iy
        double bd = __builtin_inf();
        int bi = RN_NO_INDEX;
        for (int cell = t; cell < cells; cell += CAL_BLOCK) {
            const int ix = cell / ay.n, iy = cell - ix * ay.n;
            const double x = vp_elem(ax, ix), y = vp_elem(ay, iy);
            double acc = 0.0;
            for (int64_t k = 0; k < n; ++k) {                                   // line_to_point, homography.py:91-94
                const double x0 = L[4 * k], y0 = L[4 * k + 1], x1 = L[4 * k + 2], y1 = L[4 * k + 3];
                const double dx = x1 - x0, dy = y1 - y0;
                const double num = fabs(dx * (y0 - y) - dy * (x0 - x));
                const double q = num / (sqrt(dx * dx + dy * dy) + 1e-08);
                acc += q * q;
            }
            if (acc < bd) { bd = acc; bi = cell; }                              // ascending cells: the first minimum; NaN never
        }
        block_arg_first<CAL_BLOCK / RN_WAVE>(bd, bi, rn_lt_first<double>(), sh_d, sh_i);
        if (bd < best) {                                                        // strict, against the best carried across levels
            const int ix = bi / ay.n, iy = bi - ix * ay.n;
            px = vp_elem(ax, ix);
            py = vp_elem(ay, iy);
            best = bd;
        }
        g = g / 10.0;
    }
    if (t == 0) { o[0] = px; o[1] = py; o[2] = best; status[s] = st; }
}

extern "C" int rn_vanishing_points(const double *lines, int64_t rows, const int64_t *offsets, int64_t sets, double *out,
                                   double *trace, int32_t *status, void *stream) {
    if (sets <= 0 || sets > 0x7fffffff || rows < 0) return RN_EINVAL;
    hipLaunchKernelGGL(vanishing_points_kernel, dim3((unsigned)sets), dim3(CAL_BLOCK), 0, (hipStream_t)stream, lines, offsets,
                       rows, out, trace, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ------------------------------------------------------------------------------------------------ reprojection error
// image -> state (fp64 projection, fp32 state) -> space (fp32) -> image (fp64) of every box, the corner distances, and
// their two means.  Order: per box ((e0 + e1) + e2) + e3; box b into the partial of lane b % 256, ascending b; the
// partials fold pairwise, red[t] += red[t + s] for s = 128 .. 1; the mean is red[0] / (4 d).  Ends with a barrier.
__device__ __forceinline__ void reproj_means(const double *__restrict__ boxes, const float *__restrict__ heights,
                                             const double *__restrict__ H, const double *P, int64_t d, double *red,
                                             double &top, double &bot) {
    const int t = threadIdx.x;
    double pt_sum = 0.0, pb_sum = 0.0;
    for (int64_t b = t; b < d; b += CAL_BLOCK) {
        const double2 *src = reinterpret_cast<const double2 *>(boxes + b * 16);
        double2 pt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) pt[k] = src[k];
        double x[8], y[8], z[8];
        hg_project_from_im(pt, (double)heights[b], H, nullptr, 0, x, y, z);     // homography.py:581
        float st[6];
        corners_to_state<double>(x, y, z, st);
        float fx[8], fy[8], fz[8];
        state_corners(st, fx, fy, fz);                                          // homography.py:582
        double2 rp[8];
        hg_project_to_im(fx, fy, fz, P, nullptr, 0, rp);
        double e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double ex = fabs(pt[k].x - rp[k].x), ey = fabs(pt[k].y - rp[k].y);    // homography.py:585
            e[k] = sqrt(ex * ex + ey * ey);
        }
        pb_sum += ((e[0] + e[1]) + e[2]) + e[3];                                // homography.py:586
        pt_sum += ((e[4] + e[5]) + e[6]) + e[7];                                // homography.py:587
    }
    red[t] = pt_sum;
    red[CAL_BLOCK + t] = pb_sum;
    __syncthreads();
    for (int s = CAL_BLOCK / 2; s >= 1; s >>= 1) {
        if (t < s) {
            red[t] += red[t + s];
            red[CAL_BLOCK + t] += red[CAL_BLOCK + t + s];
        }
        __syncthreads();
    }
    const double cnt = (double)(4 * d);
    top = red[0] / cnt;
    bot = red[CAL_BLOCK] / cnt;
    __syncthreads();
}

__device__ __forceinline__ void scaled_P(const double *__restrict__ P_orig, double C, double P[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = P_orig[k];
    P[2] = P_orig[2] * C; P[6] = P_orig[6] * C; P[10] = P_orig[10] * C;         // P[:,2] *= C, homography.py:645
}

__global__ __launch_bounds__(CAL_BLOCK) void reproj_error_kernel(const double *__restrict__ boxes,
                                                                 const float *__restrict__ heights,
                                                                 const double *__restrict__ H,
                                                                 const double *__restrict__ P_orig,
                                                                 const double *__restrict__ C, int64_t d,
                                                                 double *__restrict__ out) {
    __shared__ double red[2 * CAL_BLOCK];
    double P[12], top, bot;
    scaled_P(P_orig, C[blockIdx.x], P);
    reproj_means(boxes, heights, H, P, d, red, top, bot);
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = top; out[2 * blockIdx.x + 1] = bot; }
}

extern "C" int rn_hg_reproj_error(const double *boxes, const float *heights, const double *H, const double *P_orig,
                                  const double *C, int64_t d, int64_t K, double *out, void *stream) {
    if (d <= 0 || K <= 0 || K > 0x7fffffff || d > (1 << 28)) return RN_EINVAL;
    hipLaunchKernelGGL(reproj_error_kernel, dim3((unsigned)K), dim3(CAL_BLOCK), 0, (hipStream_t)stream, boxes, heights, H,
                       P_orig, C, d, out);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ------------------------------------------------------------------------------------------------ scale_Z
// np.linspace(lo, hi, 10): step = (hi - lo) / 9, y[i] = i * step + lo, y[9] = hi.
__device__ __forceinline__ void linspace10(double lo, double hi, double y[10]) {
    const double step = (hi - lo) / 9.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) y[i] = (double)i * step + lo;
    y[9] = hi;
}

__global__ __launch_bounds__(CAL_BLOCK) void scale_z_kernel(const double *__restrict__ boxes, const float *__restrict__ heights,
                                                            const double *__restrict__ H, const double *__restrict__ P_orig,
                                                            int64_t d, double granularity, double max_scale, int max_iters,
                                                            double *__restrict__ trace, double *__restrict__ out,
                                                            int32_t *__restrict__ info) {
    __shared__ double red[2 * CAL_BLOCK];
    const int t = threadIdx.x;
    double grid[10];
    linspace10(granularity, max_scale, grid);                                   // homography.py:628-633
    double step = grid[1] - grid[0];
    const double nan = __builtin_nan("");
    double best_C = nan, best_err = __builtin_inf(), last_C = nan;
    int iters = 0, st = 0;
    if (!(step > granularity)) st |= RN_SZ_BAD_FIRST_STEP;                      // best_error is never bound: NameError there
    while (step > granularity) {                                                // every lane holds the same values
        if (iters == max_iters) { st |= RN_SZ_TOO_MANY; break; }
        best_err = __builtin_inf();
        int bi = -1;
        double cand = nan;
#pragma unroll 1
        for (int i = 0; i < 10; ++i) {
            double C = grid[0];
#pragma unroll
            for (int k = 1; k < 10; ++k) C = (k == i) ? grid[k] : C;
            double P[12], top, bot;
            scaled_P(P_orig, C, P);
            reproj_means(boxes, heights, H, P, d, red, top, bot);
            const double err = top + bot;                                       // homography.py:604
            if (t == 0) {
                double *tr = trace + ((int64_t)iters * 10 + i) * 2;
                tr[0] = C; tr[1] = err;
            }
            if (err < best_err) { best_err = err; bi = i; cand = C; }            // strict: the first of equal errors
        }
        last_C = grid[9];                                                       // P is left at this one, homography.py:646
        ++iters;
        if (bi < 0) { st |= RN_SZ_NO_WINNER; break; }                           // all NaN: best_C is None there
        best_C = cand;
        linspace10(best_C - step, best_C + step, grid);                         // homography.py:659-662
        step = grid[1] - grid[0];
    }
    if (t == 0) { out[0] = last_C; out[1] = best_C; out[2] = best_err; info[0] = iters; info[1] = st; }
}

extern "C" int rn_hg_scale_z(const double *boxes, const float *heights, const double *H, const double *P_orig, int64_t d,
                             double granularity, double max_scale, int max_iters, double *trace, double *out, int32_t *info,
                             void *stream) {
    if (d <= 0 || d > (1 << 28) || max_iters <= 0) return RN_EINVAL;
    hipLaunchKernelGGL(scale_z_kernel, dim3(1), dim3(CAL_BLOCK), 0, (hipStream_t)stream, boxes, heights, H, P_orig, d,
                       granularity, max_scale, max_iters, trace, out, info);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ------------------------------------------------------------------------------------------------ homography fit
#define FIT_BLOCK 64
#define FIT_SWEEPS 12
#define FIT_GN_STEPS 10

// mean and sqrt(2) / mean distance of n points (Hartley), sums in point order
__device__ void fit_hartley(const double *__restrict__ p, int64_t n, double *o) {
    double mx = 0.0, my = 0.0;
    for (int64_t k = 0; k < n; ++k) { mx = mx + p[2 * k]; my = my + p[2 * k + 1]; }
    mx = mx / (double)n; my = my / (double)n;
    double md = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const double dx = p[2 * k] - mx, dy = p[2 * k + 1] - my;
        md = md + sqrt(dx * dx + dy * dy);
    }
    md = md / (double)n;
    o[0] = mx; o[1] = my;
    o[2] = md > 0.0 ? sqrt(2.0) / md : __builtin_inf();
}

// entry i of the two DLT rows of a normalised pair (x, y) -> (u, v)
__device__ __forceinline__ double dlt_row(int row, int i, double x, double y, double u, double v) {
    const double w = row == 0 ? u : v;
    const int base = row == 0 ? 0 : 3;
    if (i >= 6) return i == 6 ? w * x : (i == 7 ? w * y : w);
    if (i < base || i >= base + 3) return 0.0;
    return i == base ? -x : (i == base + 1 ? -y : -1.0);
}

// entry i of the Jacobian rows of the transfer (pu, pv) with respect to h0..h7
__device__ __forceinline__ double gn_row(int row, int i, double x, double y, double w, double pu, double pv) {
    const double p = row == 0 ? pu : pv;
    const int base = row == 0 ? 0 : 3;
    if (i >= 6) return i == 6 ? -p * x / w : -p * y / w;
    if (i < base || i >= base + 3) return 0.0;
    return i == base ? x / w : (i == base + 1 ? y / w : 1.0 / w);
}

__device__ double fit_cost(const double *h, const double *__restrict__ src, const double *__restrict__ dst, int64_t n,
                           const double *ns, const double *nt) {
    double c = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const double x = (src[2 * k] - ns[0]) * ns[2], y = (src[2 * k + 1] - ns[1]) * ns[2];
        const double u = (dst[2 * k] - nt[0]) * nt[2], v = (dst[2 * k + 1] - nt[1]) * nt[2];
        const double w = h[6] * x + h[7] * y + 1.0;
        const double ru = (h[0] * x + h[1] * y + h[2]) / w - u, rv = (h[3] * x + h[4] * y + h[5]) / w - v;
        c = c + (ru * ru + rv * rv);
    }
    return c;
}

// Gaussian elimination with partial pivoting on an 8x8 (the first largest pivot); false if a pivot is zero or not finite
__device__ bool fit_solve8(double *M, double *r, double *x) {
    for (int c = 0; c < 8; ++c) {
        int p = c;
        for (int k = c + 1; k < 8; ++k) if (fabs(M[k * 8 + c]) > fabs(M[p * 8 + c])) p = k;
        if (!(fabs(M[p * 8 + c]) > 0.0) || !isfinite(M[p * 8 + c])) return false;
        if (p != c) {
            for (int k = 0; k < 8; ++k) { const double tmp = M[c * 8 + k]; M[c * 8 + k] = M[p * 8 + k]; M[p * 8 + k] = tmp; }
            const double tmp = r[c]; r[c] = r[p]; r[p] = tmp;
        }
        for (int k = c + 1; k < 8; ++k) {
            const double f = M[k * 8 + c] / M[c * 8 + c];
            for (int j = c; j < 8; ++j) M[k * 8 + j] = M[k * 8 + j] - f * M[c * 8 + j];
            r[k] = r[k] - f * r[c];
        }
    }
    for (int c = 7; c >= 0; --c) {
        double acc = r[c];
        for (int k = c + 1; k < 8; ++k) acc = acc - M[c * 8 + k] * x[k];
        x[c] = acc / M[c * 8 + c];
    }
    return true;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_homography_kernel(const double *__restrict__ src_all,
                                                                   const double *__restrict__ dst_all,
                                                                   const int64_t *__restrict__ offsets, int64_t rows, int refine,
                                                                   double *__restrict__ H_out, int32_t *__restrict__ status) {
    __shared__ double N[81], V[81], ns[3], nt[3], h[9], JtJ[64], Jtr[8], M[64], rhs[8], delta[8], trial[9];
    __shared__ int st_sh;
    const int t = threadIdx.x, prob = blockIdx.x;
    const int64_t lo = offsets[prob], n = offsets[prob + 1] - lo;
    double *Ho = H_out + (int64_t)prob * 9;
    if (t < 9) Ho[t] = __builtin_nan("");
    if (lo < 0 || n < 0 || lo > rows - n) {                                     // a row range outside src / dst: nothing is read
        if (t == 0) status[prob] = RN_FIT_BAD_OFFSETS;
        return;
    }
    const double *src = src_all + lo * 2, *dst = dst_all + lo * 2;
    if (n < 4) {
        if (t == 0) status[prob] = RN_FIT_FEW_POINTS;
        return;
    }
    if (t == 0) { fit_hartley(src, n, ns); st_sh = 0; }
    if (t == 1) fit_hartley(dst, n, nt);
    __syncthreads();
    if (!isfinite(ns[2]) || !isfinite(nt[2])) {
        if (t == 0) status[prob] = RN_FIT_DEGENERATE;
        return;
    }
    // the 9x9 normal matrix: each entry takes the rows in order (point 0 row u, point 0 row v, point 1 row u, ...)
    for (int e = t; e < 81; e += FIT_BLOCK) {
        const int i = e / 9, j = e - i * 9;
        double acc = 0.0;
        for (int64_t k = 0; k < n; ++k) {
            const double x = (src[2 * k] - ns[0]) * ns[2], y = (src[2 * k + 1] - ns[1]) * ns[2];
            const double u = (dst[2 * k] - nt[0]) * nt[2], v = (dst[2 * k + 1] - nt[1]) * nt[2];
            acc = acc + dlt_row(0, i, x, y, u, v) * dlt_row(0, j, x, y, u, v);
            acc = acc + dlt_row(1, i, x, y, u, v) * dlt_row(1, j, x, y, u, v);
        }
        N[e] = acc;
        V[e] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    if (t == 0) {
        // cyclic Jacobi, a fixed number of sweeps
        for (int sweep = 0; sweep < FIT_SWEEPS; ++sweep)
            for (int p = 0; p < 8; ++p)
                for (int q = p + 1; q < 9; ++q) {
                    const double apq = N[p * 9 + q];
                    if (apq == 0.0) continue;
                    const double theta = (N[q * 9 + q] - N[p * 9 + p]) / (2.0 * apq);
                    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                    for (int k = 0; k < 9; ++k) {
                        const double akp = N[k * 9 + p], akq = N[k * 9 + q];
                        N[k * 9 + p] = c * akp - s * akq; N[k * 9 + q] = s * akp + c * akq;
                    }
                    for (int k = 0; k < 9; ++k) {
                        const double apk = N[p * 9 + k], aqk = N[q * 9 + k];
                        N[p * 9 + k] = c * apk - s * aqk; N[q * 9 + k] = s * apk + c * aqk;
                    }
                    for (int k = 0; k < 9; ++k) {
                        const double vkp = V[k * 9 + p], vkq = V[k * 9 + q];
                        V[k * 9 + p] = c * vkp - s * vkq; V[k * 9 + q] = s * vkp + c * vkq;
                    }
                }
        int i0 = 0, i1 = -1, i8 = 0;
        bool finite = true;
        for (int k = 0; k < 9; ++k) {
            finite = finite && isfinite(N[k * 9 + k]);
            if (N[k * 9 + k] < N[i0 * 9 + i0]) i0 = k;
            if (N[k * 9 + k] > N[i8 * 9 + i8]) i8 = k;
        }
        for (int k = 0; k < 9; ++k) if (k != i0 && (i1 < 0 || N[k * 9 + k] < N[i1 * 9 + i1])) i1 = k;
        if (!finite || !(N[i1 * 9 + i1] > 1e-12 * N[i8 * 9 + i8])) {
            st_sh = RN_FIT_DEGENERATE;                                          // a second null direction: collinear points
        } else {
            bool ok = V[8 * 9 + i0] != 0.0;
            for (int k = 0; k < 9; ++k) ok = ok && isfinite(V[k * 9 + i0]);
            if (!ok) st_sh = RN_FIT_NOT_FINITE;
            else for (int k = 0; k < 9; ++k) h[k] = V[k * 9 + i0] / V[8 * 9 + i0];
        }
    }
    __syncthreads();
    if (st_sh != 0) {
        if (t == 0) status[prob] = st_sh;
        return;
    }
    if (refine && n > 4) {
        // damped Gauss-Newton on the forward transfer error over h0..h7, in the normalised frame
        double lm = 1e-3, cost = 0.0;
        if (t == 0) cost = fit_cost(h, src, dst, n, ns, nt);
        for (int step = 0; step < FIT_GN_STEPS; ++step) {
            __syncthreads();
            for (int e = t; e < 72; e += FIT_BLOCK) {
                const int i = e < 64 ? e / 8 : e - 64, j = e < 64 ? e - (e / 8) * 8 : -1;
                double acc = 0.0;
                for (int64_t k = 0; k < n; ++k) {
                    const double x = (src[2 * k] - ns[0]) * ns[2], y = (src[2 * k + 1] - ns[1]) * ns[2];
                    const double u = (dst[2 * k] - nt[0]) * nt[2], v = (dst[2 * k + 1] - nt[1]) * nt[2];
                    const double w = h[6] * x + h[7] * y + 1.0;
                    const double pu = (h[0] * x + h[1] * y + h[2]) / w, pv = (h[3] * x + h[4] * y + h[5]) / w;
                    if (j >= 0) {
                        acc = acc + gn_row(0, i, x, y, w, pu, pv) * gn_row(0, j, x, y, w, pu, pv);
                        acc = acc + gn_row(1, i, x, y, w, pu, pv) * gn_row(1, j, x, y, w, pu, pv);
                    } else {
                        acc = acc + gn_row(0, i, x, y, w, pu, pv) * (pu - u);
                        acc = acc + gn_row(1, i, x, y, w, pu, pv) * (pv - v);
                    }
                }
                if (j >= 0) JtJ[e] = acc; else Jtr[i] = acc;
            }
            __syncthreads();
            if (t == 0) {
                for (int e = 0; e < 64; ++e) M[e] = JtJ[e] + ((e / 8 == e % 8) ? lm * JtJ[e] : 0.0);
                for (int k = 0; k < 8; ++k) rhs[k] = -Jtr[k];
                if (!fit_solve8(M, rhs, delta)) {
                    lm = lm * 10.0;
                } else {
                    for (int k = 0; k < 8; ++k) trial[k] = h[k] + delta[k];
                    trial[8] = h[8];
                    const double c2 = fit_cost(trial, src, dst, n, ns, nt);
                    if (c2 < cost) {
                        for (int k = 0; k < 8; ++k) h[k] = trial[k];
                        cost = c2; lm = lm * 0.1;
                    } else {
                        lm = lm * 10.0;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        // H = Td^-1 Hn Ts, then H[2,2] = 1
        const double Ts[9] = {ns[2], 0.0, -ns[2] * ns[0], 0.0, ns[2], -ns[2] * ns[1], 0.0, 0.0, 1.0};
        const double Ti[9] = {1.0 / nt[2], 0.0, nt[0], 0.0, 1.0 / nt[2], nt[1], 0.0, 0.0, 1.0};
        double A[9], Hm[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double acc = 0.0;
                for (int k = 0; k < 3; ++k) acc = acc + h[i * 3 + k] * Ts[k * 3 + j];
                A[i * 3 + j] = acc;
            }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double acc = 0.0;
                for (int k = 0; k < 3; ++k) acc = acc + Ti[i * 3 + k] * A[k * 3 + j];
                Hm[i * 3 + j] = acc;
            }
        const double h22 = Hm[8];
        bool ok = h22 != 0.0;
        for (int k = 0; k < 9; ++k) {
            Hm[k] = Hm[k] / h22;
            ok = ok && isfinite(Hm[k]);
        }
        if (ok) for (int k = 0; k < 9; ++k) Ho[k] = Hm[k];
        status[prob] = ok ? 0 : RN_FIT_NOT_FINITE;
    }
}

extern "C" int rn_fit_homography(const double *src, const double *dst, int64_t rows, const int64_t *offsets, int64_t problems,
                                 int refine, double *H, int32_t *status, void *stream) {
    if (problems <= 0 || problems > 0x7fffffff || rows < 0) return RN_EINVAL;
    hipLaunchKernelGGL(fit_homography_kernel, dim3((unsigned)problems), dim3(FIT_BLOCK), 0, (hipStream_t)stream, src, dst,
                       offsets, rows, refine, H, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

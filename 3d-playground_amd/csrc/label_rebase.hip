// The passes of the reference's annotator (seems_to_be_working.py) that ACT on what the label audit measured:
//   Annotator.replace_homgraphy (:1629-1730) re-expresses every manually drawn box under a re-fitted calibration,
//   Annotator.offset_box_y (:1779-1805), through replace_y (:1733-1776), applies the road-curvature polynomial or takes it out.
//
// The reference searches the new box centre with three torch calls per box: per round an 11 x 11 grid of shifted boxes goes
// through the NEW homography, and the centre whose bottom footprint lands nearest the old box's image footprint starts the next
// round at a fifth of the radius.  Here:
//   lr_rebase_kernel    one wave per box.  Every lane projects the old box once (fp32 state, state_corners, the old matrices),
//                       then the wave runs label_grid_search (label_search_dev.h) in fp64: the kernel's own part is the error
//                       of one candidate centre.
//   lr_offset_y_kernel  one thread per box.
//
// Arithmetic: fp64, one rounding per operation in the reference's order (this file is in the Makefile's EXACT list: no fma
// contraction).  The candidate's corners are the mixed form of state_corners_mixed: fp64 sums, each rounded once to fp32.
//
// The camera index is the only index read from memory.  It is checked before use; a bad one sets a bit of *status and the box is
// left out (its outputs keep the launcher's fill: NaN and -1).  No kernel spins or asserts.
#include <math.h>

#include "common.h"
#include "homography_dev.h"
#include "label_search_dev.h"

#define LR_THREADS 256
#define LR_WAVES (LR_THREADS / RN_WAVE)
#define LR_MAX ((int64_t)1 << 31)

__global__ void __launch_bounds__(LR_THREADS) lr_rebase_kernel(const double *__restrict__ state6, const int32_t *__restrict__ cam,
                                                               int64_t n, const double *__restrict__ P1_old,
                                                               const double *__restrict__ P2_old, const double *__restrict__ P1_new,
                                                               const double *__restrict__ P2_new, int n_cam,
                                                               const double *__restrict__ radii, int rounds, int grid,
                                                               double *__restrict__ centre, double *__restrict__ err_out,
                                                               int32_t *__restrict__ idx_out, int32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * LR_WAVES + (threadIdx.x >> 6);     // wave-uniform, like every exit below
    if (b >= n) return;
    const int m = cam[b];
    if (m < 0 || m >= n_cam) {
        if (lane == 0) rn_flag(status, RN_LABEL_BAD_CAMERA);
        return;
    }
    double s[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = state6[b * 6 + k];
    float fx[8], fy[8], fz[8];
    double2 old_im[8], im[8];
    {                                                                           // :1677-1678: the old box is a float32 tensor
        float s32[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) s32[k] = (float)s[k];
        state_corners(s32, fx, fy, fz);
        hg_project_to_im(fx, fy, fz, P1_old, P2_old, m, old_im);
    }
    double cx = s[0], cy = s[1], win_err = 0.0;
    const auto score = [&](double x, double y) {                                // :1685-1701: one shifted box
        s[0] = x;
        s[1] = y;
        state_corners_mixed(s, fx, fy, fz);
        hg_project_to_im(fx, fy, fz, P1_new, P2_new, m, im);                    // the wrapper switch is per candidate
        double mk[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                           // :1701: the four bottom corners
            const double dx = im[k].x - old_im[k].x, dy = im[k].y - old_im[k].y;
            mk[k] = (dx * dx + dy * dy) / 2.0;
        }
        return (((mk[0] + mk[1]) + mk[2]) + mk[3]) / 4.0;
    };
    if (!label_grid_search<double>(cx, cy, win_err, radii, rounds, grid, idx_out + b * rounds, status, score)) return;
    if (lane == 0) {
        centre[b * 2] = cx;
        centre[b * 2 + 1] = cy;
        err_out[b] = win_err;                                                   // :1709: the last round's minimum
    }
}

__global__ void __launch_bounds__(LR_THREADS) lr_offset_y_kernel(const double *__restrict__ xy, const double *__restrict__ coef,
                                                                 const double *__restrict__ y_straight,
                                                                 const int32_t *__restrict__ direction, int64_t n, int reverse,
                                                                 double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (i >= n) return;
    const double x = xy[i * 2], y = xy[i * 2 + 1];
    const double p2 = coef[i * 3], p1 = coef[i * 3 + 1], p0 = coef[i * 3 + 2];
    double y_offset = (x * x * p2 + x * p1) + p0;                               // :1792
    if (direction[i] == -1) y_offset -= y_straight[i];                          // :1795-1797
    out[i] = reverse ? y + y_offset : y - y_offset;                             // :1799-1802
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rn_label_rebase(const double *state6, const int32_t *cam, int64_t n, const double *P1_old, const double *P2_old,
                               const double *P1_new, const double *P2_new, int n_cam, const double *radii, int rounds, int grid,
                               double *centre, double *err, int32_t *idx, int32_t *status, void *stream) {
    if (n < 0 || n >= LR_MAX || n_cam < 0 || n_cam > RN_LABEL_MAX_CAMS || rounds < 1 || rounds > RN_LABEL_REBASE_MAX_ROUNDS ||
        grid < 2 || grid > RN_LABEL_REBASE_MAX_GRID || !status)
        return RN_EINVAL;
    if (n == 0) return RN_OK;
    if (!state6 || !cam || !radii || !centre || !err || !idx || (n_cam > 0 && (!P1_old || !P1_new))) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(centre, 0xFF, (size_t)n * 2 * sizeof(double), s);        // NaN / -1: a box that was left out
    if (e == hipSuccess) e = hipMemsetAsync(err, 0xFF, (size_t)n * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(idx, 0xFF, (size_t)n * rounds * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lr_rebase_kernel, dim3(rn_blocks(n, LR_WAVES)), dim3(LR_THREADS), 0, s, state6, cam, n, P1_old, P2_old, P1_new,
                       P2_new, n_cam, radii, rounds, grid, centre, err, idx, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_label_offset_y(const double *xy, const double *coef, const double *y_straight, const int32_t *direction,
                                 int64_t n, int reverse, double *out, void *stream) {
    if (n < 0 || n >= LR_MAX * LR_THREADS) return RN_EINVAL;
    if (n == 0) return RN_OK;
    if (!xy || !coef || !y_straight || !direction || !out) return RN_EINVAL;
    hipLaunchKernelGGL(lr_offset_y_kernel, dim3(rn_blocks(n, LR_THREADS)), dim3(LR_THREADS), 0, (hipStream_t)stream, xy, coef,
                       y_straight, direction, n, reverse != 0, out);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

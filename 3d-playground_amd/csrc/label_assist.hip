// The detector-assisted labelling path of the reference's annotator (manual_annotator_state_v3.py; seems_to_be_working.py has
// the same code at other line numbers):
//   Annotator.automate (:644-697) crops around a box, Annotator.crop_detect (:699-741) runs the 112 x 112 localiser on the crop
//   and keeps its best anchor, Annotator.paste_in_2D_bbox (:588-642) slides the copied 3D template until its image footprint
//   fits the detected 2D box.
//
// The reference does this for one box per key press.  Here, for n boxes at once:
//   as_windows_kernel  one thread per box: state -> image corners -> 2D extent, the edge test of :672, the square crop window.
//   as_anchor_kernel   one wave per crop: lanes stride the anchors, a wave reduction on (confidence, anchor) picks torch.argmax's
//                      winner (a NaN counts as largest, equal values go to the lower index), lane 0 moves the winner's box into
//                      frame coordinates.
//   as_fit_kernel      one wave per box: label_grid_search (label_search_dev.h) in fp32; the kernel's own part is the error of one
//                      candidate centre.
//
// Arithmetic (this file is in the Makefile's EXACT list: no fma contraction, one rounding per operation).  With today's numpy and
// torch the reference's search runs in float32 throughout, unlike replace_homgraphy's: the centre is a float32 tensor,
// np.linspace of float32 torch scalars is evaluated by torch in float32 (arange * step + start, the last element stop),
// torch.tensor of the candidate is float32, so the corners are state_corners' float32 sums.  Only state_to_im is float64: the
// corners are widened, projected with the float64 camera matrices (hg_project_to_im, the wrapper switch per candidate), the
// min / max over the eight float64 image points is rounded once to float32 on assignment into the float32 `boxes_new`.  The
// difference to the target, its square, the sum of the four squares in index order and the division by 4 are float32.  The radii
// arrive as float64 (ops.label_rebase_radii) and are rounded to float32 first, as torch does with a Python scalar beside a
// float32 tensor.  tests/golden/label_assist.npz, written by the reference's own methods, agrees with every statement here.
//
// A box whose byte of the optional `skip` array is set (the edge test of as_windows_kernel) is left out of the fit without a
// status bit, as the reference returns silently.
//
// Indices read from memory: the camera index, checked before use; a bad one sets a bit of *status and the box is left out (its
// outputs keep the launcher's fill: NaN and -1).  No kernel spins or asserts.
#include <math.h>

#include "common.h"
#include "homography_dev.h"
#include "label_search_dev.h"

#define AS_THREADS 256
#define AS_WAVES (AS_THREADS / RN_WAVE)
#define AS_MAX ((int64_t)1 << 31)

// :620-623 / :665-668: torch.min / torch.max over the eight float64 image points (a NaN wins both), then one rounding to float32
__device__ __forceinline__ void as_extent(const float s[6], const double *__restrict__ P1, const double *__restrict__ P2, int m,
                                          float ext[4]) {
    float fx[8], fy[8], fz[8];
    double2 im[8];
    state_corners(s, fx, fy, fz);
    hg_project_to_im(fx, fy, fz, P1, P2, m, im);
    double x1 = im[0].x, y1 = im[0].y, x2 = im[0].x, y2 = im[0].y;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const double u = im[k].x, v = im[k].y;
        x1 = (u < x1 || u != u) ? u : x1;
        x2 = (u > x2 || u != u) ? u : x2;
        y1 = (v < y1 || v != v) ? v : y1;
        y2 = (v > y2 || v != v) ? v : y2;
    }
    ext[0] = (float)x1;
    ext[1] = (float)y1;
    ext[2] = (float)x2;
    ext[3] = (float)y2;
}

__global__ void __launch_bounds__(AS_THREADS) as_fit_kernel(const float *__restrict__ tmpl, const int32_t *__restrict__ cam,
                                                            const float *__restrict__ centre0, const float *__restrict__ target,
                                                            const uint8_t *__restrict__ skip, int64_t n,
                                                            const double *__restrict__ P1, const double *__restrict__ P2, int n_cam,
                                                            const double *__restrict__ radii, int rounds, int grid,
                                                            float *__restrict__ centre, float *__restrict__ err_out,
                                                            int32_t *__restrict__ idx_out, int32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * AS_WAVES + (threadIdx.x >> 6);     // wave-uniform, like every exit below
    if (b >= n) return;
    if (skip != nullptr && skip[b]) return;                                     // as_windows_kernel's edge test: no status bit
    const int m = cam[b];
    if (m < 0 || m >= n_cam) {
        if (lane == 0) rn_flag(status, RN_LABEL_BAD_CAMERA);
        return;
    }
    float s[6], t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s[2 + k] = tmpl[b * 4 + k];                                            // :611: (l, w, h, direction)
        t[k] = target[b * 4 + k];
    }
    float cx = centre0[b * 2], cy = centre0[b * 2 + 1], win_err = 0.f;
    const auto score = [&](float x, float y) {                                  // :606-627: one shifted template
        s[0] = x;
        s[1] = y;
        float ext[4], sq[4];
        as_extent(s, P1, P2, m, ext);                                           // :616-623, the wrapper switch is per candidate
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                           // :627
            const float d = ext[k] - t[k];
            sq[k] = d * d;
        }
        return (((sq[0] + sq[1]) + sq[2]) + sq[3]) / 4.0f;
    };
    if (!label_grid_search<float>(cx, cy, win_err, radii, rounds, grid, idx_out + b * rounds, status, score)) return;
    if (lane == 0) {
        centre[b * 2] = cx;
        centre[b * 2 + 1] = cy;
        err_out[b] = win_err;                                                   // the last round's minimum
    }
}

__global__ void __launch_bounds__(AS_THREADS) as_anchor_kernel(const float *__restrict__ cls, const float *__restrict__ reg,
                                                               const float *__restrict__ win, int64_t n, int A, int C, float cs,
                                                               float *__restrict__ box, int32_t *__restrict__ anchor,
                                                               float *__restrict__ conf, int32_t *__restrict__ klass) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * AS_WAVES + (threadIdx.x >> 6);     // wave-uniform
    if (b >= n) return;
    const float *cb = cls + b * A * C;
    const torch_argmax_before<float> above;
    float best = -INFINITY;
    int best_a = RN_NO_INDEX, best_k = 0;
    for (int a = lane; a < A; a += RN_WAVE) {                                   // ascending per lane
        const float *row = cb + (int64_t)a * C;
        float v = row[0];                                                       // :731: torch.max over the classes
        int vk = 0;
        for (int k = 1; k < C; ++k) {
            const float w = row[k];
            if (above(w, k, v, vk)) { v = w; vk = k; }
        }
        if (above(v, a, best, best_a)) { best = v; best_a = a; best_k = vk; }
    }
    // Written in place, not wave_arg_first: the winner's class index travels along as a third value, and behind a helper that
    // carries it this launch measured 1 us slower than before (profiles/wave_primitives_refactor.txt).  As is: the same code.
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                                          // :734: torch.argmax over the anchors
        const float ov = __shfl_xor(best, o, RN_WAVE);
        const int oa = __shfl_xor(best_a, o, RN_WAVE);
        const int ok = __shfl_xor(best_k, o, RN_WAVE);
        if (above(ov, oa, best, best_a)) { best = ov; best_a = oa; best_k = ok; }
    }
    if (lane != 0 || best_a >= A) return;                                       // A >= 1: lane 0 always holds an anchor
    const float minx = win[b * 3], miny = win[b * 3 + 1], scale = win[b * 3 + 2];
    const float *rb = reg + (b * A + best_a) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) box[b * 4 + k] = rb[k] * scale / cs + ((k & 1) ? miny : minx);   // :738-740
    anchor[b] = best_a;
    conf[b] = best;
    klass[b] = best_k;
}

__global__ void __launch_bounds__(AS_THREADS) as_windows_kernel(const float *__restrict__ state6, const int32_t *__restrict__ cam,
                                                                int64_t n, const double *__restrict__ P1,
                                                                const double *__restrict__ P2, int n_cam, float ber, float width,
                                                                float height, float *__restrict__ crop_box,
                                                                float *__restrict__ rois, float *__restrict__ win,
                                                                uint8_t *__restrict__ skipped, int32_t *status) {
    const int64_t b = (int64_t)blockIdx.x * AS_THREADS + threadIdx.x;
    if (b >= n) return;
    skipped[b] = 1;
    const int m = cam[b];
    if (m < 0 || m >= n_cam) {
        rn_flag(status, RN_LABEL_BAD_CAMERA);
        return;
    }
    float s[6], ext[4];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = state6[b * 6 + k];                       // :662
    as_extent(s, P1, P2, m, ext);
#pragma unroll
    for (int k = 0; k < 4; ++k) crop_box[b * 4 + k] = ext[k];
    if (ext[0] < 0.f || ext[1] < 0.f || ext[2] > width || ext[3] > height) return;      // :672
    const float w = ext[2] - ext[0], h = ext[3] - ext[1];                       // :707-709; Python's max(w, h): w unless h > w
    const float scale = (h > w ? h : w) * ber;
    const float half = scale / 2.0f;
    const float mx = (ext[2] + ext[0]) / 2.0f, my = (ext[3] + ext[1]) / 2.0f;   // :713-716
    const float minx = mx - half, miny = my - half;
    skipped[b] = 0;
    rois[b * 5] = (float)m;
    rois[b * 5 + 1] = minx;
    rois[b * 5 + 2] = miny;
    rois[b * 5 + 3] = mx + half;
    rois[b * 5 + 4] = my + half;
    win[b * 3] = minx;
    win[b * 3 + 1] = miny;
    win[b * 3 + 2] = scale;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rn_label_fit_box2d(const float *tmpl, const int32_t *cam, const float *centre0, const float *target,
                                  const uint8_t *skip, int64_t n, const double *P1, const double *P2, int n_cam,
                                  const double *radii, int rounds, int grid,
                                  float *centre, float *err, int32_t *idx, int32_t *status, void *stream) {
    if (n < 0 || n >= AS_MAX || n_cam < 0 || n_cam > RN_LABEL_MAX_CAMS || rounds < 1 || rounds > RN_LABEL_REBASE_MAX_ROUNDS ||
        grid < 2 || grid > RN_LABEL_REBASE_MAX_GRID || !status)
        return RN_EINVAL;
    if (n == 0) return RN_OK;
    if (!tmpl || !cam || !centre0 || !target || !radii || !centre || !err || !idx || (n_cam > 0 && !P1)) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(centre, 0xFF, (size_t)n * 2 * sizeof(float), s);         // NaN / -1: a box that was left out
    if (e == hipSuccess) e = hipMemsetAsync(err, 0xFF, (size_t)n * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(idx, 0xFF, (size_t)n * rounds * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(as_fit_kernel, dim3(rn_blocks(n, AS_WAVES)), dim3(AS_THREADS), 0, s, tmpl, cam, centre0, target, skip, n, P1,
                       P2, n_cam, radii, rounds, grid, centre, err, idx, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_label_best_anchor(const float *cls, const float *reg, const float *win, int64_t n, int A, int C, float cs,
                                    float *box, int32_t *anchor, float *conf, int32_t *klass, void *stream) {
    if (n < 0 || n >= AS_MAX || A < 1 || C < 1 || (int64_t)A * C >= AS_MAX) return RN_EINVAL;
    if (n == 0) return RN_OK;
    if (!cls || !reg || !win || !box || !anchor || !conf || !klass) return RN_EINVAL;
    hipLaunchKernelGGL(as_anchor_kernel, dim3(rn_blocks(n, AS_WAVES)), dim3(AS_THREADS), 0, (hipStream_t)stream, cls, reg, win, n,
                       A, C, cs, box, anchor, conf, klass);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_label_crop_windows(const float *state6, const int32_t *cam, int64_t n, const double *P1, const double *P2,
                                     int n_cam, float ber, float width, float height, float *crop_box, float *rois, float *win,
                                     uint8_t *skipped, int32_t *status, void *stream) {
    if (n < 0 || n >= AS_MAX || n_cam < 0 || n_cam > RN_LABEL_MAX_CAMS || !status) return RN_EINVAL;
    if (n == 0) return RN_OK;
    if (!state6 || !cam || !crop_box || !rois || !win || !skipped || (n_cam > 0 && !P1)) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(crop_box, 0xFF, (size_t)n * 4 * sizeof(float), s);       // NaN: a box that was left out
    if (e == hipSuccess) e = hipMemsetAsync(rois, 0xFF, (size_t)n * 5 * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(win, 0xFF, (size_t)n * 3 * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(as_windows_kernel, dim3(rn_blocks(n, AS_THREADS)), dim3(AS_THREADS), 0, s, state6, cam, n, P1, P2, n_cam, ber,
                       width, height, crop_box, rois, win, skipped, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

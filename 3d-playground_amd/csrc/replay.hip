// Data_Reader.plot_in / Camera_Wrapper / test_integrity (datareader.py:24-89, 253-399, 586-653) without cv2: a tracking CSV
// laid back over the camera frames, on the device.  The painters are render.hip's (a bit of the mask plane is just a number to
// them); what only the replay needs is here:
//
//   rn_replay_boxes    every object of one label instant in every camera: the constant-velocity shift (:344-345, fp32 as
//                      torch does it) and rn_state_to_im's projection, one lane per (camera, object)
//   rn_replay_compose  uint8 frames + mask plane -> the uint8 RGB mosaic, column-major tiles (:364-374), written directly at the
//                      output size (bilinear, half-pixel centres, exact integers); four output pixels of a row per lane
//   rn_frame_absdiff   sum |a - b| over a window of two uint8 frames (:617) as one exact integer, two stages
//   rn_running_frame   0.95 running + 0.05 frame in fp64, in place (:74-77)
//
// Everything but the projection is integer arithmetic or one fp rounding per operation: this file is in the Makefile's EXACT
// list (no fma contraction).  No floating-point atomics, no integer ones either: results are the same from run to run.
#include "homography_dev.h"

#define RP_THREADS 256

// ---------------------------------------------------------------------------------------------- boxes
__global__ void __launch_bounds__(RP_THREADS) rp_boxes_kernel(const float *__restrict__ state7, int64_t n, const double *__restrict__ dt,
                                                              const double *__restrict__ P1, const double *__restrict__ P2, int C,
                                                              float *__restrict__ views, double *__restrict__ im,
                                                              int32_t *__restrict__ side, int32_t *__restrict__ cam) {
    const int64_t t = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
    if (t >= n * C) return;
    const int c = (int)(t / n);
    const float *s = state7 + (t % n) * 7;
    float v[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = s[k];
    const float dtf = (float)dt[c];                                   // the Python scalar enters the fp32 product as fp32
    float shift = v[6] * dtf;                                         // datareader.py:345, left to right, one rounding each
    shift = shift * v[5];
    v[0] = v[0] + shift;
#pragma unroll
    for (int k = 0; k < 7; ++k) views[t * 7 + k] = v[k];
    side[t] = v[1] > 60.0f ? 1 : 0;                                   // plot_state_boxes (homography.py:874)
    cam[t] = c;
    float x[8], y[8], z[8];
    state_corners(v, x, y, z);
    double2 pt[8];
    hg_project_to_im(x, y, z, P1, P2, c, pt);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        im[t * 16 + 2 * k] = pt[k].x;
        im[t * 16 + 2 * k + 1] = pt[k].y;
    }
}

// ---------------------------------------------------------------------------------------------- compose
// one channel of one composed pixel: include/retinanet_mi355x.h, rn_replay_compose.  Layers lowest to highest.
__device__ __forceinline__ unsigned rp_channel(unsigned v, unsigned m, int ch) {
    if (m & RN_REPLAY_PRIMARY) v = ch == 2 ? 255u : 0u;
    if (m & RN_REPLAY_SECONDARY) v = ch == 1 ? 255u : 0u;
    if (m & RN_REPLAY_LABEL) v = (7u * v + 3u * 255u + 5u) / 10u;
    if (m & RN_REPLAY_LABEL_TEXT) v = 0u;
    return v;
}

struct rp_geom {
    int n_cam, H, W, R, C, swap_rb;                                   // R x C tiles of H x W; camera i in tile (i % R, i / R)
};

// floor(a / b) for 0 <= a < 2^52, b > 0 and a quotient below 2^21, without the 64-bit integer division: an fp64 estimate
// (a is exact in fp64, inv_b = 1.0 / b: the estimate is within 2^-30 of the quotient) corrected by at most one.
__device__ __forceinline__ int64_t rp_div(int64_t a, int64_t b, double inv_b) {
    const int64_t q = (int64_t)((double)a * inv_b);
    const int64_t r = a - q * b;
    return r < 0 ? q - 1 : (r >= b ? q + 1 : q);
}

// the composed pixel at canvas position (cx, cy), both inside the canvas; an unused tile is black
__device__ __forceinline__ void rp_pixel(const uint8_t *__restrict__ frames, const uint16_t *__restrict__ mask, const rp_geom &g, int cx,
                                         int tc, int cy, int tr, unsigned px[3]) {
    const int i = tc * g.R + tr;                                      // tr = cy / H, tc = cx / W
    if (i >= g.n_cam) {
        px[0] = px[1] = px[2] = 0u;
        return;
    }
    const int64_t p = ((int64_t)i * g.H + (cy - tr * g.H)) * g.W + (cx - tc * g.W);
    const uint8_t *f = frames + p * 3;
    const unsigned m = mask[p];
    px[0] = rp_channel(f[g.swap_rb ? 2 : 0], m, 0);
    px[1] = rp_channel(f[1], m, 1);
    px[2] = rp_channel(f[g.swap_rb ? 0 : 2], m, 2);
}

// twelve bytes out, as three dwords when the address allows it
__device__ __forceinline__ void rp_store4(uint8_t *__restrict__ dst, const unsigned px[4][3], int n) {
    if (n == 4 && ((uintptr_t)dst & 3) == 0) {
        unsigned *d = reinterpret_cast<unsigned *>(dst);
        d[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
        d[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
        d[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                dst[3 * j] = (uint8_t)px[j][0];
                dst[3 * j + 1] = (uint8_t)px[j][1];
                dst[3 * j + 2] = (uint8_t)px[j][2];
            }
    }
}

// The canvas itself: a lane takes four consecutive pixels of one row of one tile, twelve frame bytes as three dwords and eight
// mask bytes as one load when the addresses allow it (always when W is a multiple of 4), single loads otherwise and for the
// row's tail.  Tiles past n_cam are written as zeros.
__global__ void __launch_bounds__(RP_THREADS) rp_compose_kernel(const uint8_t *__restrict__ frames, const uint16_t *__restrict__ mask,
                                                                uint8_t *__restrict__ out, rp_geom g, int64_t groups, int gpr) {
    const int64_t q = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
    if (q >= groups) return;
    const int64_t row = q / gpr;                                      // tile * H + y
    const int x0 = (int)(q % gpr) * 4;
    const int tile = (int)(row / g.H), y = (int)(row % g.H);          // tile = tc * R + tr: the camera's own index
    const int tr = tile % g.R, tc = tile / g.R;
    const int n = min(4, g.W - x0);
    unsigned px[4][3];
    if (tile >= g.n_cam) {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j][0] = px[j][1] = px[j][2] = 0u;
    } else {
        const int64_t p = ((int64_t)tile * g.H + y) * g.W + x0;
        const uint8_t *f = frames + p * 3;
        const uint16_t *mp = mask + p;
        unsigned b[12], m[4];
        if (n == 4 && ((uintptr_t)f & 3) == 0) {
            const unsigned *w = reinterpret_cast<const unsigned *>(f);
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b[k] = (w0 >> (8 * k)) & 255u;
                b[4 + k] = (w1 >> (8 * k)) & 255u;
                b[8 + k] = (w2 >> (8 * k)) & 255u;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) b[k] = k < 3 * n ? f[k] : 0u;
        }
        if (n == 4 && ((uintptr_t)mp & 7) == 0) {
            const uint2 t = *reinterpret_cast<const uint2 *>(mp);
            m[0] = t.x & 0xFFFFu; m[1] = t.x >> 16; m[2] = t.y & 0xFFFFu; m[3] = t.y >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = j < n ? mp[j] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            px[j][0] = rp_channel(b[3 * j + (g.swap_rb ? 2 : 0)], m[j], 0);
            px[j][1] = rp_channel(b[3 * j + 1], m[j], 1);
            px[j][2] = rp_channel(b[3 * j + (g.swap_rb ? 0 : 2)], m[j], 2);
        }
    }
    rp_store4(out + ((((int64_t)tr * g.H + y) * g.C + tc) * g.W + x0) * 3, px, n);
}

struct rp_recip {
    double inv_2ow, inv_2oh, inv_full, inv_w, inv_h;                  // 1 / (2 OW), 1 / (2 OH), 1 / (4 OW OH), 1 / W, 1 / H
};

// one axis of the resampling rule: output index X of O samples over a canvas of S -> the two taps and their weights
// (w0 + w1 = 2 O).  S, O <= 2^20: num < 2^42.
__device__ __forceinline__ void rp_axis(int X, int O, int S, double inv_2o, int &i0, int &i1, int64_t &w0, int64_t &w1) {
    int64_t num = (int64_t)(2 * X + 1) * S - O;
    const int64_t top = (int64_t)2 * O * (S - 1);
    num = num < 0 ? 0 : (num > top ? top : num);
    i0 = (int)rp_div(num, (int64_t)2 * O, inv_2o);
    w1 = num - (int64_t)2 * O * i0;
    w0 = (int64_t)2 * O - w1;
    i1 = min(i0 + 1, S - 1);                                          // its weight is 0 where it is clamped
}

// The mosaic at another size: a lane takes four consecutive output pixels of one output row; every tap is composed from the
// frame and the mask where it is read, so the full-size canvas never exists.  Sum of the four weights = 4 OW OH <= 2^42, times
// 255: int64.
__global__ void __launch_bounds__(RP_THREADS) rp_resample_kernel(const uint8_t *__restrict__ frames, const uint16_t *__restrict__ mask,
                                                                 uint8_t *__restrict__ out, rp_geom g, int OW, int OH, int64_t groups,
                                                                 int gpr, rp_recip rc) {
    const int64_t q = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
    if (q >= groups) return;
    const int Y = (int)(q / gpr), X0 = (int)(q % gpr) * 4;
    const int n = min(4, OW - X0);
    const int CW = g.C * g.W, CH = g.R * g.H;
    int y0, y1;
    int64_t wy0, wy1;
    rp_axis(Y, OH, CH, rc.inv_2oh, y0, y1, wy0, wy1);
    const int tr0 = (int)rp_div(y0, g.H, rc.inv_h), tr1 = (int)rp_div(y1, g.H, rc.inv_h);
    const int64_t half = (int64_t)2 * OW * OH, full = 2 * half;
    unsigned px[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        px[j][0] = px[j][1] = px[j][2] = 0u;
        if (j >= n) continue;
        int x0, x1;
        int64_t wx0, wx1;
        rp_axis(X0 + j, OW, CW, rc.inv_2ow, x0, x1, wx0, wx1);
        const int tc0 = (int)rp_div(x0, g.W, rc.inv_w), tc1 = (int)rp_div(x1, g.W, rc.inv_w);
        unsigned a[3], b[3], c[3], d[3];
        rp_pixel(frames, mask, g, x0, tc0, y0, tr0, a);
        rp_pixel(frames, mask, g, x1, tc1, y0, tr0, b);
        rp_pixel(frames, mask, g, x0, tc0, y1, tr1, c);
        rp_pixel(frames, mask, g, x1, tc1, y1, tr1, d);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int64_t s = wx0 * wy0 * a[ch] + wx1 * wy0 * b[ch] + wx0 * wy1 * c[ch] + wx1 * wy1 * d[ch];
            px[j][ch] = (unsigned)rp_div(s + half, full, rc.inv_full);
        }
    }
    rp_store4(out + ((int64_t)Y * OW + X0) * 3, px, n);
}

// ---------------------------------------------------------------------------------------------- window sum
// Stage 1: a workgroup sums a contiguous share of the window's bytes (row-major over the window, so neighbouring lanes read
// neighbouring bytes) into partial[block]; stage 2: one workgroup adds the partials.  Integer adds: any order gives the same sum.
__device__ __forceinline__ uint64_t rp_block_sum(uint64_t v, uint64_t *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = RP_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(RP_THREADS) rp_absdiff_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int W, int y0,
                                                                int x0, int64_t row_bytes, int64_t items, uint64_t *__restrict__ partial) {
    __shared__ uint64_t red[RP_THREADS];
    uint64_t sum = 0;
    for (int64_t it = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * RP_THREADS) {
        const int64_t r = it / row_bytes, k = it - r * row_bytes;
        const int64_t at = ((int64_t)(y0 + r) * W + x0) * 3 + k;
        const int d = (int)a[at] - (int)b[at];
        sum += (uint64_t)(d < 0 ? -d : d);
    }
    sum = rp_block_sum(sum, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(RP_THREADS) rp_absdiff_final_kernel(const uint64_t *__restrict__ partial, int n, int64_t *__restrict__ out) {
    __shared__ uint64_t red[RP_THREADS];
    uint64_t sum = 0;
    for (int i = threadIdx.x; i < n; i += RP_THREADS) sum += partial[i];
    sum = rp_block_sum(sum, red);
    if (threadIdx.x == 0) out[0] = (int64_t)sum;
}

// ---------------------------------------------------------------------------------------------- running frame
__global__ void __launch_bounds__(RP_THREADS) rp_running_kernel(double *__restrict__ running, const uint8_t *__restrict__ frame, int64_t n,
                                                                int first) {
    const int64_t i = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
    if (i >= n) return;
    const double f = (double)frame[i];
    if (first) {
        running[i] = f;
        return;
    }
    const double a = 0.95 * running[i];                               // datareader.py:77, one rounding per operation
    const double b = 0.05 * f;
    running[i] = a + b;
}

// ---------------------------------------------------------------------------------------------- entry points
extern "C" int rn_replay_boxes(const float *state7, int64_t n, const double *dt, const double *P1, const double *P2, int n_cam,
                               float *views, double *im, int32_t *side, int32_t *cam, void *stream) {
    if (n < 0 || n_cam < 1 || n_cam > 65535 || n > (int64_t)0x7FFFFFFF / n_cam || dt == nullptr || P1 == nullptr) return RN_EINVAL;
    if (n > 0) {
        if (state7 == nullptr || views == nullptr || im == nullptr || side == nullptr || cam == nullptr) return RN_EINVAL;
        hipLaunchKernelGGL(rp_boxes_kernel, dim3((unsigned)rn_blocks(n * n_cam, RP_THREADS)), dim3(RP_THREADS), 0, (hipStream_t)stream, state7,
                           n, dt, P1, P2, n_cam, views, im, side, cam);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

extern "C" int rn_replay_compose(const uint8_t *frames, int swap_rb, const uint16_t *mask, uint8_t *out, int n_cam, int H, int W, int R,
                                 int OW, int OH, void *stream) {
    if (frames == nullptr || mask == nullptr || out == nullptr || n_cam < 1 || n_cam > 65535 || H < 1 || W < 1 ||
        H > RN_RENDER_MAX_DIM || W > RN_RENDER_MAX_DIM || R < 1 || R > n_cam || OW < 1 || OH < 1 || OW > RN_RENDER_MAX_DIM ||
        OH > RN_RENDER_MAX_DIM)
        return RN_EINVAL;
    const int C = (n_cam + R - 1) / R;
    if ((int64_t)C * W > RN_REPLAY_MAX_CANVAS || (int64_t)R * H > RN_REPLAY_MAX_CANVAS) return RN_EINVAL;
    const rp_geom g = {n_cam, H, W, R, C, swap_rb ? 1 : 0};
    if (OW == C * W && OH == R * H) {
        const int gpr = (W + 3) / 4;
        const int64_t groups = (int64_t)R * C * H * gpr;
        if (groups > (int64_t)0x7FFFFFFF * RP_THREADS) return RN_EINVAL;
        hipLaunchKernelGGL(rp_compose_kernel, dim3((unsigned)rn_blocks(groups, RP_THREADS)), dim3(RP_THREADS), 0, (hipStream_t)stream, frames,
                           mask, out, g, groups, gpr);
    } else {
        const int gpr = (OW + 3) / 4;
        const int64_t groups = (int64_t)OH * gpr;
        const rp_recip rc = {1.0 / (2.0 * OW), 1.0 / (2.0 * OH), 1.0 / (4.0 * OW * OH), 1.0 / W, 1.0 / H};
        hipLaunchKernelGGL(rp_resample_kernel, dim3((unsigned)rn_blocks(groups, RP_THREADS)), dim3(RP_THREADS), 0, (hipStream_t)stream, frames,
                           mask, out, g, OW, OH, groups, gpr, rc);
    }
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_frame_absdiff(const uint8_t *a, const uint8_t *b, int H, int W, int y0, int y1, int x0, int x1, int64_t *partial,
                                int64_t *out, void *stream) {
    if (a == nullptr || b == nullptr || partial == nullptr || out == nullptr || H < 1 || W < 1 || H > RN_RENDER_MAX_DIM ||
        W > RN_RENDER_MAX_DIM)
        return RN_EINVAL;
    y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0;                       // the window clipped to the frame
    y1 = y1 > H ? H : y1; x1 = x1 > W ? W : x1;
    const int64_t row_bytes = x1 > x0 ? (int64_t)(x1 - x0) * 3 : 0;
    const int64_t items = y1 > y0 ? (int64_t)(y1 - y0) * row_bytes : 0;
    int blocks = 0;
    if (items > 0) {
        const int64_t want = (items + RP_THREADS - 1) / RP_THREADS;
        blocks = want > RN_REPLAY_ABSDIFF_BLOCKS ? RN_REPLAY_ABSDIFF_BLOCKS : (int)want;
        hipLaunchKernelGGL(rp_absdiff_kernel, dim3((unsigned)blocks), dim3(RP_THREADS), 0, (hipStream_t)stream, a, b, W, y0, x0, row_bytes,
                           items, reinterpret_cast<uint64_t *>(partial));
        RN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rp_absdiff_final_kernel, dim3(1), dim3(RP_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint64_t *>(partial), blocks, out);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_running_frame(double *running, const uint8_t *frame, int64_t n, int first, void *stream) {
    if (n < 0 || n > (int64_t)0x7FFFFFFF * RP_THREADS || (n > 0 && (running == nullptr || frame == nullptr))) return RN_EINVAL;
    if (n > 0) {
        hipLaunchKernelGGL(rp_running_kernel, dim3((unsigned)rn_blocks(n, RP_THREADS)), dim3(RP_THREADS), 0, (hipStream_t)stream, running,
                           frame, n, first);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

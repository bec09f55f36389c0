// Crop-detector training batches on device: the image chain of the reference's Detection_Dataset.__getitem__ with CROP > 0
// (corrected_3D_dataset.py:330-390, 501-594).  The reference resizes, pads, flips and rotates the whole frame with Pillow on one
// host thread and then keeps a window of a few hundred pixels; here only the window is evaluated, byte for byte what Pillow
// computes:
//
//   crop_window        one lane per window pixel at frame coordinate (minx + x, miny + y): 0 outside the frame (Pillow's crop
//                      fills with zero); inside, Pillow's AFFINE + BILINEAR sample (double, truncated, fill 0) of the flipped,
//                      padded image, whose four taps are made on the fly: the noise byte outside min(rh,H) x min(rw,W), else the
//                      vertical resize pass over horizontal-pass bytes, clip8((2^21 + sum k p) >> 22) each
//   crop_resize_h      the second resize, horizontal: cw -> crop with K runtime taps from the host's table
//   crop_resize_v      ... vertical: ch -> crop
//   crop_contrast_sum  sum of L over the crop x crop image as it stands when the contrast op is reached
//   crop_finish        the jitter ops in the drawn order; (byte / 255 - mean) / std; inside the occlusion region the raw value of
//                      the caller's tensor, or mean + std z from the device generator, replaces the normalised one; fp32 NCHW
//
// One launch per stage for the whole batch (image in blockIdx.y), sized by the batch's largest window or by crop^2, never by the
// frame; lanes beyond an image's own window leave.  No host synchronisation.  Compiled with -ffp-contract=off.  Every index that
// comes from a record or a table is clamped before it is used, so a bad record gives wrong pixels, never an access outside the
// buffers.
#include <stdint.h>

#include "augment_dev.h"

struct CropArgs {
    const uint8_t *frames;                   // [B,H,W,3]
    const rn_augment_crop_params *params;    // [B]
    const int32_t *table_x, *table_y;        // [B,W,AUG_ROW], [B,H,AUG_ROW]: the first resize
    const int32_t *table_cx, *table_cy;      // [B,crop,1+K] each: the second resize
    const uint8_t *noise;                    // [B,H,W,3] or null
    const float *occlusion;                  // [B,3,crop,crop] or null
    uint8_t *win, *hbuf, *fin;               // [B][win_max*win_max*3], [B][win_max*crop*3], [B][crop*crop*3]
    unsigned long long *sums;                // [B]
    float *out;                              // [B,3,crop,crop]
    uint64_t seed;
    int B, H, W, K, win_max, crop;
    float mean[3], stdv[3];
};

// an image's own window size, never beyond what the workspace holds
__device__ __forceinline__ int crop_cw(const CropArgs &a, const rn_augment_crop_params &q) { return aug_clampi(q.win[2], 0, a.win_max); }
__device__ __forceinline__ int crop_ch(const CropArgs &a, const rn_augment_crop_params &q) { return aug_clampi(q.win[3], 0, a.win_max); }

// the resized image's pixel (yy, xx), 0 <= yy < min(rh, H), 0 <= xx < min(rw, W): the vertical pass over horizontal-pass bytes.
// Taps whose coefficient is zero (a table row's tail) add nothing and are not fetched.
__device__ __forceinline__ void crop_resized(const CropArgs &a, const rn_augment_crop_params &q, int b, int yy, int xx, int out[3]) {
    const uint8_t *img = a.frames + (int64_t)b * a.H * a.W * 3;
    const bool hskip = q.rw == a.W, vskip = q.rh == a.H;                     // a pass whose size does not change is skipped
    int kx[RN_AUG_TAPS], ky[RN_AUG_TAPS], x0 = xx, y0 = yy;
    if (!hskip) {
        const int32_t *t = a.table_x + ((int64_t)b * a.W + xx) * AUG_ROW;
        x0 = t[0];
#pragma unroll
        for (int j = 0; j < RN_AUG_TAPS; ++j) kx[j] = t[1 + j];
    }
    if (!vskip) {
        const int32_t *t = a.table_y + ((int64_t)b * a.H + yy) * AUG_ROW;
        y0 = t[0];
#pragma unroll
        for (int j = 0; j < RN_AUG_TAPS; ++j) ky[j] = t[1 + j];
    }
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
    for (int i = 0; i < RN_AUG_TAPS; ++i) {
        if (vskip ? i > 0 : ky[i] == 0) continue;
        const uint8_t *row = img + (int64_t)aug_clampi(y0 + i, 0, a.H - 1) * a.W * 3;
        int h[3];
        if (hskip) {
            const uint8_t *s = row + 3 * aug_clampi(xx, 0, a.W - 1);
            h[0] = s[0]; h[1] = s[1]; h[2] = s[2];
        } else {
            int hacc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
            for (int j = 0; j < RN_AUG_TAPS; ++j) {
                if (kx[j] == 0) continue;
                const uint8_t *s = row + 3 * aug_clampi(x0 + j, 0, a.W - 1);
                hacc[0] += kx[j] * (int)s[0]; hacc[1] += kx[j] * (int)s[1]; hacc[2] += kx[j] * (int)s[2];
            }
            h[0] = (int)aug_clip8(hacc[0]); h[1] = (int)aug_clip8(hacc[1]); h[2] = (int)aug_clip8(hacc[2]);
        }
        if (vskip) { out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; return; }
        acc[0] += ky[i] * h[0]; acc[1] += ky[i] * h[1]; acc[2] += ky[i] * h[2];
    }
    out[0] = (int)aug_clip8(acc[0]); out[1] = (int)aug_clip8(acc[1]); out[2] = (int)aug_clip8(acc[2]);
}

// the padded image's pixel (yy, xx), 0 <= yy < H, 0 <= xx < W: the resized image over the noise image (:338-342)
__device__ __forceinline__ void crop_padded(const CropArgs &a, const rn_augment_crop_params &q, int b, int yy, int xx, int out[3]) {
    if (yy < q.rh && xx < q.rw) { crop_resized(a, q, b, yy, xx, out); return; }
    const int64_t e = (((int64_t)b * a.H + yy) * a.W + xx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = a.noise ? (int)a.noise[e + c] : (int)aug_noise(a.seed, (uint64_t)(e + c));
}

// F.crop of the rotated image (:536): Pillow's affine_transform + bilinear_filter32RGB (Geometry.c) at the window's pixels only
__global__ __launch_bounds__(256) void crop_window(const CropArgs a) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.sums[b] = 0ull;               // read by crop_contrast_sum, three launches later
    const rn_augment_crop_params &q = a.params[b];
    const int cw = crop_cw(a, q), ch = crop_ch(a, q);
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)cw * ch) return;
    const int wy = (int)(p / cw), wx = (int)(p - (int64_t)wy * cw);
    uint8_t *o = a.win + ((int64_t)b * a.win_max * a.win_max + p) * 3;
    const int64_t X = (int64_t)q.win[0] + wx, Y = (int64_t)q.win[1] + wy;    // the frame coordinate; may lie outside the frame
    o[0] = 0; o[1] = 0; o[2] = 0;
    if (X < 0 || X >= a.W || Y < 0 || Y >= a.H) return;
    const double xin = (double)X + 0.5, yin = (double)Y + 0.5;
    const double sx = q.affine[0] * xin + q.affine[1] * yin + q.affine[2];
    const double sy = q.affine[3] * xin + q.affine[4] * yin + q.affine[5];
    if (!(sx >= 0.0 && sx < (double)a.W && sy >= 0.0 && sy < (double)a.H)) return;
    const double fx = sx - 0.5, fy = sy - 0.5;
    const double x0f = floor(fx), y0f = floor(fy);
    const double dx = fx - x0f, dy = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;                                  // in [-1, W-1] and [-1, H-1]
    int xa = aug_clampi(x0, 0, a.W - 1), xb = aug_clampi(x0 + 1, 0, a.W - 1);
    const int ya = aug_clampi(y0, 0, a.H - 1), yb = aug_clampi(y0 + 1, 0, a.H - 1);
    if (q.flip) { xa = a.W - 1 - xa; xb = a.W - 1 - xb; }
    int s1[3], s2[3], s3[3], s4[3];
    crop_padded(a, q, b, ya, xa, s1);
    crop_padded(a, q, b, ya, xb, s2);
    crop_padded(a, q, b, yb, xa, s3);
    crop_padded(a, q, b, yb, xb, s4);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v1 = (double)s1[c], v2 = (double)s2[c], v3 = (double)s3[c], v4 = (double)s4[c];
        const double t = v1 + (v2 - v1) * dx;
        const double u = v3 + (v4 - v3) * dx;
        o[c] = (uint8_t)(int)(t + (u - t) * dy);
    }
}

// F.resize(im_crop, (CROP, CROP)) (:556), horizontal pass: [ch, cw] -> [ch, crop]
__global__ __launch_bounds__(256) void crop_resize_h(const CropArgs a) {
    const int b = blockIdx.y;
    const rn_augment_crop_params &q = a.params[b];
    const int cw = crop_cw(a, q), ch = crop_ch(a, q);
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cw < 1 || p >= (int64_t)ch * a.crop) return;
    const int y = (int)(p / a.crop), x = (int)(p - (int64_t)y * a.crop);
    const uint8_t *row = a.win + ((int64_t)b * a.win_max * a.win_max + (int64_t)y * cw) * 3;
    uint8_t *o = a.hbuf + ((int64_t)b * a.win_max * a.crop + p) * 3;
    if (cw == a.crop) {                                                      // a pass whose size does not change is skipped
        o[0] = row[3 * x]; o[1] = row[3 * x + 1]; o[2] = row[3 * x + 2];
        return;
    }
    const int32_t *t = a.table_cx + ((int64_t)b * a.crop + x) * (1 + a.K);
    const int first = t[0];
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
    for (int j = 0; j < a.K; ++j) {
        const int k = t[1 + j];
        const uint8_t *s = row + 3 * aug_clampi(first + j, 0, cw - 1);
        acc[0] += k * (int)s[0]; acc[1] += k * (int)s[1]; acc[2] += k * (int)s[2];
    }
    o[0] = (uint8_t)aug_clip8(acc[0]); o[1] = (uint8_t)aug_clip8(acc[1]); o[2] = (uint8_t)aug_clip8(acc[2]);
}

// ... vertical pass: [ch, crop] -> [crop, crop]
__global__ __launch_bounds__(256) void crop_resize_v(const CropArgs a) {
    const int b = blockIdx.y;
    const rn_augment_crop_params &q = a.params[b];
    const int cw = crop_cw(a, q), ch = crop_ch(a, q);
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)a.crop * a.crop) return;
    const int y = (int)(p / a.crop), x = (int)(p - (int64_t)y * a.crop);
    const uint8_t *img = a.hbuf + (int64_t)b * a.win_max * a.crop * 3;
    uint8_t *o = a.fin + ((int64_t)b * a.crop * a.crop + p) * 3;
    if (cw < 1 || ch < 1) { o[0] = 0; o[1] = 0; o[2] = 0; return; }          // an empty window: the reference raises
    if (ch == a.crop) {
        const uint8_t *s = img + p * 3;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        return;
    }
    const int32_t *t = a.table_cy + ((int64_t)b * a.crop + y) * (1 + a.K);
    const int first = t[0];
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
    for (int j = 0; j < a.K; ++j) {
        const int k = t[1 + j];
        const uint8_t *s = img + ((int64_t)aug_clampi(first + j, 0, ch - 1) * a.crop + x) * 3;
        acc[0] += k * (int)s[0]; acc[1] += k * (int)s[1]; acc[2] += k * (int)s[2];
    }
    o[0] = (uint8_t)aug_clip8(acc[0]); o[1] = (uint8_t)aug_clip8(acc[1]); o[2] = (uint8_t)aug_clip8(acc[2]);
}

__global__ __launch_bounds__(256) void crop_contrast_sum(const CropArgs a) {
    __shared__ int red[4];
    const int64_t n = (int64_t)a.crop * a.crop;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const rn_augment_crop_params &q = a.params[b];
    if (!q.apply) return;                                                    // uniform over the block
    int l = 0;
    if (p < n) {
        const uint8_t *s = a.fin + ((int64_t)b * n + p) * 3;
        int px[3] = {s[0], s[1], s[2]};
        aug_jitter(px, q, true, 0);
        l = aug_luma(px);
    }
    l = wave_sum(l);                                                         // <= 64 * 255
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&a.sums[b], (unsigned long long)(red[0] + red[1] + red[2] + red[3]));
}

// the occlusion generator: z of Box-Muller in fp32 from two 24-bit uniforms of one splitmix64 word, keyed by (seed, the
// element's index in [B,3,crop,crop] with bit 63 set, which no pad-noise element has)
__device__ __forceinline__ float crop_normal(uint64_t seed, uint64_t element) {
    const uint64_t r = aug_mix(seed, element | (1ull << 63));
    const float u1 = ((float)(unsigned)(r >> 40) + 1.0f) * 5.9604644775390625e-8f;          // (0, 1]
    const float u2 = (float)(unsigned)((r >> 16) & 0xFFFFFFull) * 5.9604644775390625e-8f;   // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795865f * u2);
}

__global__ __launch_bounds__(256) void crop_finish(const CropArgs a) {
    const int64_t n = (int64_t)a.crop * a.crop;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= n) return;
    const int y = (int)(p / a.crop), x = (int)(p - (int64_t)y * a.crop);
    const rn_augment_crop_params &q = a.params[b];
    const uint8_t *s = a.fin + ((int64_t)b * n + p) * 3;
    int px[3] = {s[0], s[1], s[2]};
    if (q.apply) {
        const unsigned long long S = a.sums[b], N = (unsigned long long)n;
        aug_jitter(px, q, false, (int)((2ull * S + N) / (2ull * N)));        // floor(S / N + .5)
    }
    const bool hidden = q.occluded && x >= q.occlude[0] && x < q.occlude[2] && y >= q.occlude[1] && y < q.occlude[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t e = ((int64_t)b * 3 + c) * n + p;
        float v;
        if (hidden) {                                                        // :588-592: the raw value, not normalised
            v = a.occlusion ? a.occlusion[e] : a.mean[c] + a.stdv[c] * crop_normal(a.seed, (uint64_t)e);
        } else {
            const float t = (float)px[c] / 255.0f;                           // to_tensor
            v = (t - a.mean[c]) / a.stdv[c];                                 // normalize: sub_, div_
        }
        a.out[e] = v;
    }
}

#define RN_CROP_WIN_LIMIT 16384
#define RN_CROP_TAPS_LIMIT 8193

extern "C" int64_t rn_augment_crops_workspace_bytes(int B, int win_max, int crop) {
    if (B <= 0 || win_max <= 0 || crop <= 0 || win_max > RN_CROP_WIN_LIMIT || crop > RN_CROP_WIN_LIMIT) return 0;
    return aug_align((int64_t)B * win_max * win_max * 3) + aug_align((int64_t)B * win_max * crop * 3) +
           aug_align((int64_t)B * crop * crop * 3) + aug_align((int64_t)B * 8);
}

extern "C" int rn_augment_crops(const uint8_t *frames, int B, int H, int W, const rn_augment_crop_params *params,
                                const int32_t *table_x, const int32_t *table_y, const int32_t *table_cx, const int32_t *table_cy,
                                int K, int win_max, int crop, const uint8_t *noise, const float *occlusion, uint64_t seed,
                                float mean0, float mean1, float mean2, float std0, float std1, float std2, void *workspace,
                                float *out, void *stream) {
    if (!frames || !params || !table_x || !table_y || !table_cx || !table_cy || !workspace || !out) return RN_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || (int64_t)H * W > (int64_t)1 << 30) return RN_EINVAL;
    if (K < 1 || K > RN_CROP_TAPS_LIMIT || win_max <= 0 || win_max > RN_CROP_WIN_LIMIT || crop <= 0 || crop > RN_CROP_WIN_LIMIT) return RN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(params) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return RN_EINVAL;
    CropArgs a;
    a.frames = frames; a.params = params; a.table_x = table_x; a.table_y = table_y; a.table_cx = table_cx; a.table_cy = table_cy;
    a.noise = noise; a.occlusion = occlusion;
    a.win = static_cast<uint8_t *>(workspace);
    a.hbuf = a.win + aug_align((int64_t)B * win_max * win_max * 3);
    a.fin = a.hbuf + aug_align((int64_t)B * win_max * crop * 3);
    a.sums = reinterpret_cast<unsigned long long *>(a.fin + aug_align((int64_t)B * crop * crop * 3));
    a.out = out; a.seed = seed; a.B = B; a.H = H; a.W = W; a.K = K; a.win_max = win_max; a.crop = crop;
    a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
    a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    const dim3 grid_win(rn_blocks((int64_t)win_max * win_max, 256), B), grid_h(rn_blocks((int64_t)win_max * crop, 256), B);
    const dim3 grid_out(rn_blocks((int64_t)crop * crop, 256), B);
    hipLaunchKernelGGL(crop_window, grid_win, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_resize_h, grid_h, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_resize_v, grid_out, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_contrast_sum, grid_out, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_finish, grid_out, block, 0, s, a);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// Training-batch augmentation on device: the image chain of the reference's Detection_Dataset.__getitem__
// (corrected_3D_dataset.py:330-478, CROP == 0), which there is a PIL resize, a torch.rand noise pad, a flip, a bilinear rotation, up to
// three ImageEnhance passes, to_tensor, normalize and a tile swap per 1080p image on one host thread.  Here the uint8 frame travels (as
// in ingest.hip) and the pixel work is five HBM passes over the batch, byte for byte what Pillow computes:
//
//   aug_resize_h      Pillow's ImagingResample, horizontal pass: out = clip8((2^21 + sum k p) >> 22), coefficients from the host's table
//   aug_resize_v_pad  the vertical pass over those bytes; outside the resized region the noise byte floor(fp32(k 2^-24) 255)
//   aug_rotate        AFFINE + BILINEAR with fill 0, in double, truncated; the flip is a mirrored column in its reads
//   aug_contrast_sum  sum of L over the image as it stands when the contrast op is reached (exact: integers, 64-bit atomic adds)
//   aug_finish        the jitter ops in the drawn order, t = a + f (p - a) in fp32 each; (byte / 255 - mean) / std as ingest_one;
//                     the tile swap as a roll of the source index; fp32 NCHW
//
// One launch per stage for the whole batch (image in blockIdx.y), no host synchronisation, no trigonometry: the six affine
// coefficients come from the host.  Compiled with -ffp-contract=off: one rounding per operation.  Every index that comes from a
// parameter record or a table is clamped before it is used, so a bad record gives wrong pixels, never an access outside the buffers.
#include <stdint.h>

#include "augment_dev.h"

struct AugArgs {
    const uint8_t *frames;                   // [B,H,W,3]
    const rn_augment_params *params;         // [B]
    const int32_t *table_x, *table_y;        // [B,W,AUG_ROW], [B,H,AUG_ROW]
    const uint8_t *noise;                    // [B,H,W,3] or null
    uint8_t *buf0, *buf1;                    // [B,H,W,3] each
    unsigned long long *sums;                // [B]
    float *out;                              // [B,3,H,W]
    uint64_t seed;
    int B, H, W;
    float mean[3], stdv[3];
};

__global__ __launch_bounds__(256) void aug_resize_h(const AugArgs a) {
    const int64_t hw = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.sums[b] = 0ull;               // read by aug_contrast_sum, three launches later
    if (p >= hw) return;
    const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
    const rn_augment_params &q = a.params[b];
    const uint8_t *row = a.frames + ((int64_t)b * hw + (int64_t)y * a.W) * 3;
    uint8_t *o = a.buf0 + ((int64_t)b * hw + p) * 3;
    if (q.rw == a.W) {                                                       // a pass whose size does not change is skipped
        o[0] = row[3 * x]; o[1] = row[3 * x + 1]; o[2] = row[3 * x + 2];
        return;
    }
    if (x >= q.rw) { o[0] = 0; o[1] = 0; o[2] = 0; return; }                 // pad, filled by the next stage
    const int32_t *t = a.table_x + ((int64_t)b * a.W + x) * AUG_ROW;
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
    for (int j = 0; j < RN_AUG_TAPS; ++j) {
        const int k = t[1 + j];
        const uint8_t *s = row + 3 * aug_clampi(t[0] + j, 0, a.W - 1);
        acc[0] += k * (int)s[0]; acc[1] += k * (int)s[1]; acc[2] += k * (int)s[2];
    }
    o[0] = (uint8_t)aug_clip8(acc[0]); o[1] = (uint8_t)aug_clip8(acc[1]); o[2] = (uint8_t)aug_clip8(acc[2]);
}

__global__ __launch_bounds__(256) void aug_resize_v_pad(const AugArgs a) {
    const int64_t hw = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= hw) return;
    const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
    const rn_augment_params &q = a.params[b];
    const uint8_t *img = a.buf0 + (int64_t)b * hw * 3;
    uint8_t *o = a.buf1 + ((int64_t)b * hw + p) * 3;
    if (y < q.rh && x < q.rw) {                                              // inside the resized image (y < H, x < W anyway)
        if (q.rh == a.H) {
            const uint8_t *s = img + p * 3;
            o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
            return;
        }
        const int32_t *t = a.table_y + ((int64_t)b * a.H + y) * AUG_ROW;
        int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
        for (int j = 0; j < RN_AUG_TAPS; ++j) {
            const int k = t[1 + j];
            const uint8_t *s = img + ((int64_t)aug_clampi(t[0] + j, 0, a.H - 1) * a.W + x) * 3;
            acc[0] += k * (int)s[0]; acc[1] += k * (int)s[1]; acc[2] += k * (int)s[2];
        }
        o[0] = (uint8_t)aug_clip8(acc[0]); o[1] = (uint8_t)aug_clip8(acc[1]); o[2] = (uint8_t)aug_clip8(acc[2]);
        return;
    }
    const int64_t e = ((int64_t)b * hw + p) * 3;
    if (a.noise) {
        o[0] = a.noise[e]; o[1] = a.noise[e + 1]; o[2] = a.noise[e + 2];
    } else {
        o[0] = (uint8_t)aug_noise(a.seed, (uint64_t)e); o[1] = (uint8_t)aug_noise(a.seed, (uint64_t)e + 1);
        o[2] = (uint8_t)aug_noise(a.seed, (uint64_t)e + 2);
    }
}

// Pillow's affine_transform + bilinear_filter32RGB (Geometry.c), reading the flipped image
__global__ __launch_bounds__(256) void aug_rotate(const AugArgs a) {
    const int64_t hw = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= hw) return;
    const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
    const rn_augment_params &q = a.params[b];
    const uint8_t *img = a.buf1 + (int64_t)b * hw * 3;
    uint8_t *o = a.buf0 + ((int64_t)b * hw + p) * 3;
    const double xin = (double)x + 0.5, yin = (double)y + 0.5;
    const double sx = q.affine[0] * xin + q.affine[1] * yin + q.affine[2];
    const double sy = q.affine[3] * xin + q.affine[4] * yin + q.affine[5];
    if (!(sx >= 0.0 && sx < (double)a.W && sy >= 0.0 && sy < (double)a.H)) { o[0] = 0; o[1] = 0; o[2] = 0; return; }
    const double fx = sx - 0.5, fy = sy - 0.5;
    const double x0f = floor(fx), y0f = floor(fy);
    const double dx = fx - x0f, dy = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;                                  // in [-1, W-1] and [-1, H-1]
    int xa = aug_clampi(x0, 0, a.W - 1), xb = aug_clampi(x0 + 1, 0, a.W - 1);
    const int ya = aug_clampi(y0, 0, a.H - 1), yb = aug_clampi(y0 + 1, 0, a.H - 1);
    if (q.flip) { xa = a.W - 1 - xa; xb = a.W - 1 - xb; }
    const uint8_t *s1 = img + ((int64_t)ya * a.W + xa) * 3, *s2 = img + ((int64_t)ya * a.W + xb) * 3;
    const uint8_t *s3 = img + ((int64_t)yb * a.W + xa) * 3, *s4 = img + ((int64_t)yb * a.W + xb) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v1 = (double)s1[c], v2 = (double)s2[c], v3 = (double)s3[c], v4 = (double)s4[c];
        const double t = v1 + (v2 - v1) * dx;
        const double u = v3 + (v4 - v3) * dx;
        o[c] = (uint8_t)(int)(t + (u - t) * dy);
    }
}

__global__ __launch_bounds__(256) void aug_contrast_sum(const AugArgs a) {
    __shared__ int red[4];
    const int64_t hw = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const rn_augment_params &q = a.params[b];
    if (!q.apply) return;                                                    // uniform over the block
    int l = 0;
    if (p < hw) {
        const uint8_t *s = a.buf0 + ((int64_t)b * hw + p) * 3;
        int px[3] = {s[0], s[1], s[2]};
        aug_jitter(px, q, true, 0);
        l = aug_luma(px);
    }
    l = wave_sum(l);                                                         // <= 64 * 255
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&a.sums[b], (unsigned long long)(red[0] + red[1] + red[2] + red[3]));
}

__global__ __launch_bounds__(256) void aug_finish(const AugArgs a) {
    const int64_t hw = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= hw) return;
    const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
    const rn_augment_params &q = a.params[b];
    const int sy = (int)(((int64_t)y + q.dy % a.H + a.H) % a.H), sx = (int)(((int64_t)x + q.dx % a.W + a.W) % a.W);
    const uint8_t *s = a.buf0 + ((int64_t)b * hw + (int64_t)sy * a.W + sx) * 3;
    int px[3] = {s[0], s[1], s[2]};
    if (q.apply) {
        const unsigned long long S = a.sums[b], N = (unsigned long long)hw;
        aug_jitter(px, q, false, (int)((2ull * S + N) / (2ull * N)));        // floor(S / N + .5)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = (float)px[c] / 255.0f;                               // to_tensor
        a.out[((int64_t)b * 3 + c) * hw + p] = (t - a.mean[c]) / a.stdv[c];  // normalize: sub_, div_
    }
}

extern "C" int64_t rn_augment_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * aug_align((int64_t)B * H * W * 3) + aug_align((int64_t)B * 8);
}

extern "C" int rn_augment_frames(const uint8_t *frames, int B, int H, int W, const rn_augment_params *params,
                                 const int32_t *table_x, const int32_t *table_y, const uint8_t *noise, uint64_t seed,
                                 float mean0, float mean1, float mean2, float std0, float std1, float std2, void *workspace,
                                 float *out, void *stream) {
    if (!frames || !params || !table_x || !table_y || !workspace || !out || B <= 0 || H <= 0 || W <= 0 || B > 65535) return RN_EINVAL;
    if ((int64_t)H * W > (int64_t)1 << 30) return RN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(params) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return RN_EINVAL;
    AugArgs a;
    const int64_t plane = aug_align((int64_t)B * H * W * 3);
    a.frames = frames; a.params = params; a.table_x = table_x; a.table_y = table_y; a.noise = noise;
    a.buf0 = static_cast<uint8_t *>(workspace); a.buf1 = a.buf0 + plane;
    a.sums = reinterpret_cast<unsigned long long *>(a.buf0 + 2 * plane);
    a.out = out; a.seed = seed; a.B = B; a.H = H; a.W = W;
    a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
    a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(rn_blocks((int64_t)H * W, 256), B), block(256);
    hipLaunchKernelGGL(aug_resize_h, grid, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(aug_resize_v_pad, grid, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(aug_rotate, grid, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(aug_contrast_sum, grid, block, 0, s, a);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(aug_finish, grid, block, 0, s, a);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

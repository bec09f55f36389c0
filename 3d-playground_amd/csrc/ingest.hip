// Frame ingest: uint8 HWC video frames -> normalised fp32 detector input, on device.
//
// Replaces F.to_tensor + F.normalize of the reference's loaders (util_track/mp_loader.py:239-243,
// perform_3D_detection_on_video_sequences.py:51-58), which run per frame on the host and ship a 24.9 MB fp32 CHW
// tensor per 1080p camera over PCIe; here the 6.2 MB uint8 frame is what travels and the conversion is one HBM pass:
//   v = (float(u8) / 255 - mean[c]) / std[c]        three separate fp32 operations, as torchvision performs them
//   (this file is compiled with -ffp-contract=off; a true division, not a reciprocal multiply: bit-identical to the CPU)
// layout 0: NCHW [B,3,H,W]  -- exactly the tensor the reference hands to the model
// layout 1: NHWC4 [B,H,W,4] -- what the stem convolution consumes (4th channel 0), skipping rn_nchw_to_nhwc4
// swap_rb: source channel 2-c feeds output channel c (the cvtColor(BGR2RGB) of the second caller).
//
// Roofline: HBM.  Per pixel 3 B read, 12 B (NCHW) or 16 B (NHWC4) written.  A lane takes 4 consecutive pixels: three
// dword loads (12 B) and three float4 stores, one per plane (NCHW); for NHWC4 a lane takes 4 pixels 256 apart so
// that each store instruction of a wave writes 1 KiB contiguously.
#include <stdint.h>

#include "common.h"

struct IngestArgs {
    const uint8_t *src;
    float *dst;
    int64_t hw;              // pixels per image
    int B, swap_rb, layout;
    float mean[3], stdv[3];
};

__device__ __forceinline__ float ingest_one(unsigned u8, float mean, float stdv) {
    const float t = (float)u8 / 255.0f;          // to_tensor
    return (t - mean) / stdv;                    // normalize: sub_, div_
}

// hw % 4 == 0: every image starts dword-aligned in the byte stream and float4-aligned in every output plane.
__global__ __launch_bounds__(256) void ingest_kernel4(const IngestArgs a) {
    const int64_t groups = a.hw >> 2;                                   // 4-pixel groups per image
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (g >= groups) return;
    const uint32_t *s = reinterpret_cast<const uint32_t *>(a.src + ((int64_t)b * a.hw + 4 * g) * 3);
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];                    // bytes p0c0 p0c1 p0c2 p1c0 | p1c1 p1c2 p2c0 p2c1 | p2c2 p3c0 p3c1 p3c2
    unsigned px[4][3] = {{w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u},
                         {w0 >> 24, w1 & 255u, (w1 >> 8) & 255u},
                         {(w1 >> 16) & 255u, w1 >> 24, w2 & 255u},
                         {(w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24}};
    float v[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[p][c] = ingest_one(px[p][a.swap_rb ? 2 - c : c], a.mean[c], a.stdv[c]);
    if (a.layout == 1) {
        float4 *o = reinterpret_cast<float4 *>(a.dst) + (int64_t)b * a.hw + 4 * g;
#pragma unroll
        for (int p = 0; p < 4; ++p) o[p] = make_float4(v[p][0], v[p][1], v[p][2], 0.f);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            reinterpret_cast<float4 *>(a.dst + ((int64_t)b * 3 + c) * a.hw)[g] = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
    }
}

// NHWC4: the output is 16 B per pixel, so the store is already a full float4 per pixel; what matters is that the 64
// lanes of a store instruction write 1 KiB contiguously.  A lane therefore takes pixels tid, tid+256, tid+512, tid+768
// of its block's 1024 (byte loads: the reads are 16 % of the traffic and every 64-B line is shared by ~21 lanes).
__global__ __launch_bounds__(256) void ingest_nhwc4_kernel(const IngestArgs a) {
    const int64_t p0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int b = blockIdx.y;
    const uint8_t *s = a.src + (int64_t)b * a.hw * 3;
    float4 *o = reinterpret_cast<float4 *>(a.dst) + (int64_t)b * a.hw;
    unsigned u[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                       // all loads first
        const int64_t p = p0 + 256 * k;
        const int64_t q = p < a.hw ? p : a.hw - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) u[k][c] = s[q * 3 + c];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t p = p0 + 256 * k;
        if (p < a.hw)
            o[p] = make_float4(ingest_one(u[k][a.swap_rb ? 2 : 0], a.mean[0], a.stdv[0]), ingest_one(u[k][1], a.mean[1], a.stdv[1]),
                               ingest_one(u[k][a.swap_rb ? 0 : 2], a.mean[2], a.stdv[2]), 0.f);
    }
}

// any size: one pixel per lane, byte loads
__global__ __launch_bounds__(256) void ingest_kernel1(const IngestArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= a.hw) return;
    const uint8_t *s = a.src + ((int64_t)b * a.hw + p) * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ingest_one(s[a.swap_rb ? 2 - c : c], a.mean[c], a.stdv[c]);
    if (a.layout == 1) {
        reinterpret_cast<float4 *>(a.dst)[(int64_t)b * a.hw + p] = make_float4(v[0], v[1], v[2], 0.f);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.dst[((int64_t)b * 3 + c) * a.hw + p] = v[c];
    }
}

// ------------------------------------------------------------------------------------------------
// 4K frames: the loader's cv2.resize(frame, (1920, 1080)) of a 3840x2160 frame fused in front of the ingest
// (util_track/mp_loader.py:237-243).  An exact halving of 8-bit data is the area average of the 2x2 block, rounded:
// OpenCV's linear path hands exact 2x reductions to it.  Restated here in ONE place; cv2 is not installed where this
// project is built, so parity with cv2 itself is unpinned ("4K frames").  ingest_one is used unchanged, so the
// result equals rn_frame_ingest of the reduced bytes bit for bit.
//
// Roofline: HBM.  Per OUTPUT pixel 12 B read and 16 B (NHWC4) / 12 B (NCHW) written, + 3 B with the reduced frame kept.
// Pair path (W even, everything dword-aligned): a lane takes two neighbouring output pixels = 12 consecutive bytes in
// each of two input rows, three dword loads per row.  For NHWC4 the two results are packed to a word each and exchanged
// across the wave, so that each of the two store instructions of a wave writes 64 consecutive pixels = 1 KiB.
__device__ __forceinline__ unsigned half_avg(unsigned a, unsigned b, unsigned c, unsigned d) { return (a + b + c + d + 2u) >> 2; }

struct HalfArgs {
    const uint8_t *src;
    float *dst;
    uint8_t *dst_u8;         // may be null
    int H, W;                // OUTPUT size; the input is 2H x 2W
    int B, swap_rb, layout;
    float mean[3], stdv[3];
};

__device__ __forceinline__ unsigned byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 255u; }

#define HALF_PAIRS 2         // pairs per lane
__global__ __launch_bounds__(256) void ingest_half_pair_kernel(const HalfArgs a) {
    const unsigned wp = (unsigned)a.W >> 1;                              // pairs per output row
    const unsigned pairs = (unsigned)a.H * wp;                           // per image (< 2^30, checked by the entry point)
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint8_t *s = a.src + (int64_t)b * a.H * a.W * 12;
    const unsigned q0 = (blockIdx.x * 4u + wv) * (64u * HALF_PAIRS);     // the wave's first pair
    uint32_t r0[HALF_PAIRS][3], r1[HALF_PAIRS][3];
#pragma unroll
    for (int k = 0; k < HALF_PAIRS; ++k) {                               // all loads first
        const unsigned q = q0 + 64u * k + lane;
        const unsigned qc = q < pairs ? q : pairs - 1;                   // a mapped address in every lane; the store is masked
        const unsigned y = qc / wp, xh = qc - y * wp;
        const uint32_t *t = reinterpret_cast<const uint32_t *>(s + ((int64_t)(2 * y) * (2 * a.W) + 4 * (int64_t)xh) * 3);
        const uint32_t *u = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(t) + (int64_t)a.W * 6);
#pragma unroll
        for (int i = 0; i < 3; ++i) { r0[k][i] = t[i]; r1[k][i] = u[i]; }
    }
#pragma unroll
    for (int k = 0; k < HALF_PAIRS; ++k) {
        const unsigned q = q0 + 64u * k + lane;
        // bytes of a row: p0c0 p0c1 p0c2 p1c0 | p1c1 p1c2 p2c0 p2c1 | p2c2 p3c0 p3c1 p3c2
        unsigned px[2][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int i0 = c, i1 = 3 + c, i2 = 6 + c, i3 = 9 + c;
            px[0][c] = half_avg(byte_of(r0[k][i0 >> 2], i0 & 3), byte_of(r0[k][i1 >> 2], i1 & 3),
                                byte_of(r1[k][i0 >> 2], i0 & 3), byte_of(r1[k][i1 >> 2], i1 & 3));
            px[1][c] = half_avg(byte_of(r0[k][i2 >> 2], i2 & 3), byte_of(r0[k][i3 >> 2], i3 & 3),
                                byte_of(r1[k][i2 >> 2], i2 & 3), byte_of(r1[k][i3 >> 2], i3 & 3));
        }
        const bool act = q < pairs;
        if (a.dst_u8 && act) {                                           // 6 bytes at 6 q: three halfwords
            uint16_t *o = reinterpret_cast<uint16_t *>(a.dst_u8 + ((int64_t)b * pairs + q) * 6);
            o[0] = (uint16_t)(px[0][0] | (px[0][1] << 8));
            o[1] = (uint16_t)(px[0][2] | (px[1][0] << 8));
            o[2] = (uint16_t)(px[1][1] | (px[1][2] << 8));
        }
        if (a.layout == 1) {
            // lane L holds pixels 2L, 2L+1 of the wave's 128; store h writes pixel 64 h + L, held by lane 32 h + L / 2
            const unsigned w0 = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16), w1 = px[1][0] | (px[1][1] << 8) | (px[1][2] << 16);
            float4 *o = reinterpret_cast<float4 *>(a.dst) + (int64_t)b * pairs * 2;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int from = 32 * h + (lane >> 1);
                const unsigned e = (unsigned)__shfl((int)w0, from, RN_WAVE), d = (unsigned)__shfl((int)w1, from, RN_WAVE);
                const unsigned w = (lane & 1) ? d : e;
                const int64_t p = 2 * ((int64_t)q0 + 64 * k) + 64 * h + lane;
                if (p < 2 * (int64_t)pairs)
                    o[p] = make_float4(ingest_one(byte_of(w, a.swap_rb ? 2 : 0), a.mean[0], a.stdv[0]), ingest_one(byte_of(w, 1), a.mean[1], a.stdv[1]),
                                       ingest_one(byte_of(w, a.swap_rb ? 0 : 2), a.mean[2], a.stdv[2]), 0.f);
            }
        } else if (act) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int sc = a.swap_rb ? 2 - c : c;
                reinterpret_cast<float2 *>(a.dst + ((int64_t)b * 3 + c) * pairs * 2)[q] =
                    make_float2(ingest_one(px[0][sc], a.mean[c], a.stdv[c]), ingest_one(px[1][sc], a.mean[c], a.stdv[c]));
            }
        }
    }
}

// any even input size and any alignment: one output pixel per lane, byte loads and stores
__global__ __launch_bounds__(256) void ingest_half_kernel1(const HalfArgs a) {
    const int64_t hw = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= hw) return;
    const int64_t y = p / a.W, x = p - y * a.W;
    const uint8_t *t = a.src + (int64_t)b * hw * 12 + ((2 * y) * (2 * (int64_t)a.W) + 2 * x) * 3;
    const uint8_t *u = t + (int64_t)a.W * 6;
    unsigned px[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = half_avg(t[c], t[3 + c], u[c], u[3 + c]);
    if (a.dst_u8) {
        uint8_t *o = a.dst_u8 + ((int64_t)b * hw + p) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)px[c];
    }
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ingest_one(px[a.swap_rb ? 2 - c : c], a.mean[c], a.stdv[c]);
    if (a.layout == 1) {
        reinterpret_cast<float4 *>(a.dst)[(int64_t)b * hw + p] = make_float4(v[0], v[1], v[2], 0.f);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.dst[((int64_t)b * 3 + c) * hw + p] = v[c];
    }
}

extern "C" int rn_frame_ingest_half(const uint8_t *frames, int B, int H2, int W2, int swap_rb, float mean0, float mean1,
                                    float mean2, float std0, float std1, float std2, int layout, float *out,
                                    uint8_t *out_u8, void *stream) {
    if (!frames || !out || B <= 0 || H2 <= 0 || W2 <= 0 || (H2 & 1) || (W2 & 1) || B > 65535 || (layout != 0 && layout != 1)) return RN_EINVAL;
    HalfArgs a;
    a.src = frames; a.dst = out; a.dst_u8 = out_u8; a.H = H2 / 2; a.W = W2 / 2; a.B = B; a.swap_rb = swap_rb ? 1 : 0; a.layout = layout;
    a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
    a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
    const int64_t hw = (int64_t)a.H * a.W;
    if (hw >= ((int64_t)1 << 30)) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // rows are 6 W bytes and a pair starts at a multiple of 12: dword loads need W even and a dword-aligned base; the
    // float2 / float4 stores follow from W even, the halfword stores need an even base
    const bool pair = (a.W & 1) == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(out_u8) & 1) == 0;
    if (pair)
        hipLaunchKernelGGL(ingest_half_pair_kernel, dim3(rn_blocks(hw >> 1, 256 * HALF_PAIRS), B), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(ingest_half_kernel1, dim3(rn_blocks(hw, 256), B), dim3(256), 0, s, a);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_frame_ingest(const uint8_t *frames, int B, int H, int W, int swap_rb, float mean0, float mean1,
                               float mean2, float std0, float std1, float std2, int layout, float *out, void *stream) {
    if (!frames || !out || B <= 0 || H <= 0 || W <= 0 || B > 65535 || (layout != 0 && layout != 1)) return RN_EINVAL;
    IngestArgs a;
    a.src = frames; a.dst = out; a.hw = (int64_t)H * W; a.B = B; a.swap_rb = swap_rb ? 1 : 0; a.layout = layout;
    a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
    a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
    hipStream_t s = (hipStream_t)stream;
    const bool aligned = (a.hw & 3) == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0;
    if (layout == 1)
        hipLaunchKernelGGL(ingest_nhwc4_kernel, dim3(rn_blocks(a.hw, 1024), B), dim3(256), 0, s, a);
    else if (aligned)
        hipLaunchKernelGGL(ingest_kernel4, dim3(rn_blocks(a.hw >> 2, 256), B), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(ingest_kernel1, dim3(rn_blocks(a.hw, 256), B), dim3(256), 0, s, a);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

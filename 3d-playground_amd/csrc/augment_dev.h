// Device functions shared by the two augmentation chains (augment.hip: full frames; augment_crop.hip: crop windows).
#pragma once
#include <stdint.h>

#include "common.h"

#define AUG_ROW (1 + RN_AUG_TAPS)            // int32 per table row: first source index, then the taps

__device__ __forceinline__ int aug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned aug_clip8(int acc) {
    const int v = acc >> 22;
    return (unsigned)aug_clampi(v, 0, 255);
}

// the counter-based generator: splitmix64 of (seed, element index)
__device__ __forceinline__ uint64_t aug_mix(uint64_t seed, uint64_t element) {
    uint64_t z = element + seed * 0x9E3779B97F4A7C15ull;
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// ... -> 24 bits -> floor(fp32(k 2^-24) 255)
__device__ __forceinline__ unsigned aug_noise(uint64_t seed, uint64_t element) {
    const float u = (float)(unsigned)(aug_mix(seed, element) >> 40) * 5.9604644775390625e-8f;   // k * 2^-24, exact
    return (unsigned)(u * 255.0f);
}

__device__ __forceinline__ int aug_luma(const int px[3]) { return (19595 * px[0] + 38470 * px[1] + 7471 * px[2] + 32768) >> 16; }

// Image.blend(degenerate, image, f)
__device__ __forceinline__ int aug_blend(int d, int p, float f) {
    const float t = (float)d + f * (float)(p - d);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// The ImageEnhance passes in the drawn order, on one pixel.  until_contrast: stop in front of the contrast op (for its mean).
// P: a record with order[4] and factors[3] (rn_augment_params, rn_augment_crop_params).
template <class P>
__device__ __forceinline__ void aug_jitter(int px[3], const P &q, bool until_contrast, int mean) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int op = q.order[i];
        if (op == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = aug_blend(0, px[c], q.factors[0]);
        } else if (op == 1) {
            if (until_contrast) return;
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = aug_blend(mean, px[c], q.factors[1]);
        } else if (op == 2) {
            const int l = aug_luma(px);
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = aug_blend(l, px[c], q.factors[2]);
        }                                                                   // 3 = hue: draws nothing, changes nothing
    }
}

static inline int64_t aug_align(int64_t n) { return (n + 255) / 256 * 256; }

// Shared by the two fp8 convolution files (conv_fp8.hip, conv_fp8_p8.hip): the e4m3 pack and the epilogue's per-tensor scales.
#pragma once
#include "common.h"

#define F8_MAX 448.0f            // largest finite e4m3fn

// four floats -> four e4m3 in one dword (round to nearest even, saturating by the clamp in front)
__device__ __forceinline__ float f8_clamp(float a) { return fminf(fmaxf(a, -F8_MAX), F8_MAX); }
__device__ __forceinline__ int f8_pack4(float a, float b, float c, float d) {
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(a), f8_clamp(b), 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(c), f8_clamp(d), lo, true);
}

struct Fp8Args {
    float add_scale;             // the addend's per-tensor scale (its values are fp8)
    float out_inv_scale;         // 1 / the result's per-tensor scale (fp8 result), unused for an fp32 result
};

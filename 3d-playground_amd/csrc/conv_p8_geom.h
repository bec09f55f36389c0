// Geometry shared by the two eight-wave phased kernels (conv_bf16_p8.hip, conv_fp8_p8.hip): both stage a 256-row pixel tile of a
// flat [M][Cin] tensor as 128-byte rows, 64 channels of one filter tap at a time.  Only bookkeeping lives here.  The K loops, fragment
// reads, swizzles and epilogues are each file's own: their register budgets differ (see the files' comments), and a shared template
// would be a different kernel.  Two small pieces that look alike stay in the files as well, because behind a function the compiler
// orders them differently and re-allocates the whole kernel's registers (profiles/conv_launch_refactor_isa.txt): the per-lane validity
// bits `pk`, and the advance of the tap cursor (branches in the bf16 kernel, selects in the fp8 one, whose K loop must stay one block).
#pragma once
#include "common.h"

struct P8Tap { int r, s, c; };                   // filter row, filter column, first channel of a 64-channel step (wave-uniform)

// Pixel rows in front of a tile that a tap can reach back to (the pixels' buffer descriptor starts there).  One expression for the
// kernels (I = int) and for the launchers' 32-bit range checks (I = int64_t).
template <class I>
__host__ __device__ __forceinline__ I p8_halo(const rn_conv_desc &d) {
    const I ab = d.b < 0 ? -(I)d.b : (I)d.b;
    return ((d.p < 0 ? -(I)d.p : (I)d.p) + (d.kh - 1) * ab) * d.Wi + (d.p_w < 0 ? -(I)d.p_w : (I)d.p_w) + (d.kw - 1) * ab;
}

// A buffer descriptor the compiler knows to be wave-uniform (it goes into scalar registers of an asm statement).
__device__ __forceinline__ v4i32 p8_uniform(const v4i32 r) {
    v4i32 o;
    o.x = __builtin_amdgcn_readfirstlane(r.x); o.y = __builtin_amdgcn_readfirstlane(r.y);
    o.z = __builtin_amdgcn_readfirstlane(r.z); o.w = __builtin_amdgcn_readfirstlane(r.w);
    return o;
}

// What both kernels need of a problem (elem_bytes per activation / weight element): a dense low-precision result without sigmoid or
// upsampled addend, batch-dense NHWC operands, Cin in whole 64-channel steps, at most 4 x 4 taps (the validity bits), and every
// buffer offset of a tile within 32 bits.  Each file adds its own rules: rn_bf16_p8_legal, rn_fp8_p8_legal.
static inline bool p8_common_legal(const rn_conv_desc *d, int y_is_f32, int elem_bytes) {
    if (y_is_f32 || d->div_shift != 0 || d->act == 2) return false;
    if (d->Cin < 64 || (d->Cin & 63) || d->kh > 4 || d->kw > 4) return false;
    const int64_t plane = (int64_t)d->Hi * d->Wi, oplane = (int64_t)d->Ho * d->Wo;
    if (d->x_batch_stride != plane * d->Cin || d->y_batch_stride != oplane * d->Cout) return false;
    if (d->os != 1 || d->oo_h != 0 || d->oo_w != 0 || d->Hy != d->Ho || d->Wy != d->Wo || d->add_mode == 2) return false;
    if (d->add_mode == 1 && d->add_batch_stride != d->y_batch_stride) return false;
    const int64_t K = (int64_t)d->kh * d->kw * d->Cin, M = (int64_t)d->N * oplane, halo = p8_halo<int64_t>(*d);
    return M + 256 <= 0x7fffffffLL && (256 + 2 * halo + 64) * d->Cin * elem_bytes <= 0x7fffffffLL &&
           ((int64_t)d->Cout + 256) * K * elem_bytes <= 0x7fffffffLL;
}

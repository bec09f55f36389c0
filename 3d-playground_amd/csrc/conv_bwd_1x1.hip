// Backward of a 1x1 stride-1 convolution 64 -> 256 in ONE pass over dy (RN_FP32_SPLIT3).
//
// The data gradient (conv_igemm_tile.h, 256 x 64 tile) and the weight gradient (conv_wgrad.hip, 256 x 64 tile) of such a layer are
// two launches that each stream the same dy -- at layer1's resolution 1.06 GB -- with nothing in between that needs the first one's
// result.  Here a workgroup owns ALL 256 output and all 64 input channels for a K slice of pixels (16-pixel K-steps) and forms both
// products from one copy of the operands:
//   dx[p][ci] = mask(p, ci) * unscale * sum_co dy[p][co] * Wd[ci][co]         stored once, with its amax bytes and, if asked, sign bits
//   dw[co][ci] += sum_p dy[p][co] * x[p][ci],   colsum[co] += sum_p dy[p][co]  fp32 atomics into the caller's zeroed accumulators
// dy and x are loaded into registers two K-steps ahead, split into fp16 hi / lo terms ONCE per workgroup and stored as plane images in
// LDS (conv_bwd_1x1_geom.h; conv_wgrad_once_kernel's scheme).  The weight gradient reads the planes through the transposing LDS read
// (pixels are its reduction: v_mfma_f32_32x32x16_f16, wave w owns channels 64 w .. 64 w + 63 of dy: 64 accumulators).  The data
// gradient reads the SAME dy planes untransposed, as the A operand of v_mfma_f32_16x16x32_f16 (channels are its reduction), against
// the layer's pre-split data-gradient weights (rn_conv_desc.w_format 3), of which wave w keeps rows 16 w .. 16 w + 15 -- 256 channels,
// hi and lo: 64 registers -- for the whole kernel; its 16 x 16 result of a K-step crosses a small LDS stage so that the workgroup
// stores the K-step's 4 KiB of dx contiguously, 16 bytes per thread, one step later (mask, sign bits and amax in that layout).
//
// Scales: ONE split serves both products, so both take the data gradient's rule -- a power of two per IMAGE, from the image's amax
// table -- and a K slice lies inside one image (the launcher cuts slices at image boundaries).  An image's dx therefore does not
// depend on its neighbours in the batch, and the weight gradient's tile is multiplied by that image's inverse scales before its
// atomics; a per-image scale is never coarser than the tensor-wide one conv_wgrad.hip uses.
//
// Per K-step and wave: 12 MFMAs 32x32x16 + 24 MFMAs 16x16x32 (768 matrix cycles) against 24.5 KB of HBM traffic per workgroup
// (2400 cycles of a CU's share of 6.3 TB/s): the kernel is bound by bytes, two workgroups per CU (registers) keep 40-80 KB in flight.
#include <type_traits>

#include "common.h"
#include "conv_bwd_1x1_geom.h"
#include "mfma_split.h"

// RN_BF_KO (RN_EXPERIMENT builds; timing only, wrong results): 1 = no dx stores, 2 = no dw atomics, 4 = no data-gradient MFMAs
#if !RN_EXPERIMENT
#undef RN_BF_KO
#endif
#ifndef RN_BF_KO
#define RN_BF_KO 0
#endif
// RN_BF_ND (RN_EXPERIMENT builds): accumulator chains of the data gradient's 24 MFMAs per K-step (1 or 2)
#if !RN_EXPERIMENT
#undef RN_BF_ND
#endif
#ifndef RN_BF_ND
#define RN_BF_ND 1
#endif

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef short s16x4w __attribute__((ext_vector_type(4)));
typedef short s16x8w __attribute__((ext_vector_type(8)));

struct Bwd1x1Args {
    const float *dy, *x;
    const char *wd;                  // pre-split data-gradient weights [64 rows][256 / 16 records of (16 hi, 16 lo) fp16]
    const float *w_unscale;          // [64] inverse row scales of wd
    float *dx, *dw, *colsum;
    const void *mask;                // MASK 1: fp32 [pixels][64] (> 0 passes), MASK 2: its sign bits
    unsigned *sign_out;              // sign bits of dx, or NULL
    const void *dy_amax, *x_amax;    // amax tables, one per image
    void *dx_amax;                   // ... of the result, or NULL
    int HW, spi, per;                // pixels per image, K slices per image, pixels per slice (a multiple of 16)
};

// 8 consecutive pixels of one column per lane, through two transposing reads
__device__ __forceinline__ f16x8 bf_tr_operand(const char *img, unsigned a0, unsigned a1) {
    typedef __attribute__((address_space(3))) s16x4w *lp;
    const s16x4w lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(__attribute__((address_space(3))) char *)(img + a0));
    const s16x4w hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(__attribute__((address_space(3))) char *)(img + a1));
    const s16x8w v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(f16x8, v);
}

template <int MASK>
__global__ __launch_bounds__(256, 2) void conv_bwd_1x1_kernel(const Bwd1x1Args p) {
    using G = Bwd1x1Geom;
    __shared__ __attribute__((aligned(16))) char lds[2 * G::BUF];
    __shared__ __attribute__((aligned(16))) char stage[2 * G::STAGE];
    static_assert(4 * G::CO * 4 <= G::BUF, "the column-sum reduction fits a buffer");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = (int)(blockIdx.x / (unsigned)p.spi), slice = (int)blockIdx.x - n * p.spi;
    const int k0 = slice * p.per;
    const int npx = (k0 + p.per < p.HW ? k0 + p.per : p.HW) - k0;         // pixels of this slice: all in image n
    if (npx <= 0) return;
    const int nks = (npx + G::WK - 1) / G::WK;
    const int64_t pix0 = (int64_t)n * p.HW + k0;
    // buffer descriptors of the slice alone: pixels past its end read as zero (the launcher keeps a slice below 2 GiB of dy)
    const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.dy + pix0 * G::CO), (short)0,
                                                                           (int)((unsigned)npx * (unsigned)(G::CO * 4)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x + pix0 * G::CI), (short)0,
                                                                          (int)((unsigned)npx * (unsigned)(G::CI * 4)), 0x00020000);
    // the image's scales (wave-uniform)
    const int se_dy = rn_f16_scale_exp_of(rn_amax_exp(p.dy_amax, n)), se_x = rn_f16_scale_exp_of(rn_amax_exp(p.x_amax, n));
    const float s_dy = rn_exp_to_float(se_dy), u_dy = rn_exp_to_float(254 - se_dy);
    const float s_x = rn_exp_to_float(se_x), u_x = rn_exp_to_float(254 - se_x);

    // data-gradient weights of this wave's 16 input channels: B operand [k = 8 (lane >> 4) ..][j = lane & 15] of every 32-channel k-block
    f16x8 wh[8], wl[8];
    {
        const char *wrow = p.wd + (16 * wave + (lane & 15)) * (G::CO * 4) + (lane >> 5) * 64 + ((lane >> 4) & 1) * 16;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            wh[kb] = *reinterpret_cast<const f16x8 *>(wrow + kb * 128);
            wl[kb] = *reinterpret_cast<const f16x8 *>(wrow + kb * 128 + 32);
        }
    }
    __shared__ __attribute__((aligned(16))) float wus[G::CI];        // inverse weight-row scales (read back per K-step: four registers less to hold)
    if (tid < G::CI) wus[tid] = p.w_unscale[tid];

    struct Regs { f32x4v a[4], b; };
    const unsigned dy_voff = (unsigned)(((tid >> 6) * G::CO + 4 * lane) * 4);      // pixel (tid >> 6) + 4 i: + i * 4 pixels (immediate)
    const unsigned x_voff = (unsigned)(tid * 16);
    auto load_step = [&](int ks, Regs &r) {
        const unsigned so = (unsigned)ks * (unsigned)(G::WK * G::CO * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            r.a[i] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, (int)(dy_voff + i * (4 * G::CO * 4)), (int)so, 0));
        r.b = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)x_voff, (int)((unsigned)ks * (unsigned)(G::WK * G::CI * 4)), 0));
    };
    unsigned wr_dy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wr_dy[i] = (unsigned)G::dy_wr(tid, i);
    const unsigned wr_x = (unsigned)G::x_wr(tid);
    float cs4[4] = {0.f, 0.f, 0.f, 0.f};                     // column sums of this thread's 4 dy channels over its pixels
    auto split_store = [&](int buf, const Regs &r) {
        char *B = &lds[buf * G::BUF];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned h[2], l[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) cs4[j] += r.a[i][j];
            split_pair_h(r.a[i][0], r.a[i][1], s_dy, h[0], l[0]);
            split_pair_h(r.a[i][2], r.a[i][3], s_dy, h[1], l[1]);
            *reinterpret_cast<uint2 *>(B + wr_dy[i]) = make_uint2(h[0], h[1]);
            *reinterpret_cast<uint2 *>(B + G::DY_IMG + wr_dy[i]) = make_uint2(l[0], l[1]);
        }
        unsigned h[2], l[2];
        split_pair_h(r.b[0], r.b[1], s_x, h[0], l[0]);
        split_pair_h(r.b[2], r.b[3], s_x, h[1], l[1]);
        *reinterpret_cast<uint2 *>(B + 2 * G::DY_IMG + wr_x) = make_uint2(h[0], h[1]);
        *reinterpret_cast<uint2 *>(B + 2 * G::DY_IMG + G::X_IMG + wr_x) = make_uint2(l[0], l[1]);
    };

    // The dx chunk this thread finishes in a K-step: channels 4 (tid & 15) .. + 3 of pixel tid >> 4 = elements 4 tid .. 4 tid + 3 of the
    // K-step's 1024, counted from the slice's first pixel (a multiple of 64 elements: sign-bit words and their shifts carry over).  Its
    // mask is fetched a step ahead and waits as it came: four floats, or the word that holds its four sign bits.
    const int e_px = tid >> 4;
    float *dx_s = p.dx + pix0 * G::CI;
    unsigned *sign_s = p.sign_out != nullptr ? p.sign_out + pix0 * (G::CI / 32) : nullptr;
    const float *maskf_s = reinterpret_cast<const float *>(p.mask) + (MASK == 1 ? pix0 * G::CI : 0);
    const unsigned *maskb_s = reinterpret_cast<const unsigned *>(p.mask) + (MASK == 2 ? pix0 * (G::CI / 32) : 0);
    struct MaskF { float4 q; };
    struct MaskB { unsigned w; };
    typedef typename std::conditional<MASK == 1, MaskF, MaskB>::type MaskT;
    auto mask_load = [&](int ks) -> MaskT {
        MaskT m;
        const int off = ks * (G::WK * G::CI) + 4 * tid;
        const bool in = ks * G::WK + e_px < npx;
        if constexpr (MASK == 1) m.q = in ? *reinterpret_cast<const float4 *>(maskf_s + off) : make_float4(0.f, 0.f, 0.f, 0.f);
        else if constexpr (MASK == 2) m.w = in ? maskb_s[off >> 5] : 0u;
        else m.w = 0u;
        return m;
    };
    float am = 0.f;                                          // largest |dx| this thread stored
    const unsigned st_rd = (unsigned)G::st_rd(tid);
    auto dx_store = [&](int ks, int sbuf, const MaskT mk) {
        const float4 t = *reinterpret_cast<const float4 *>(&stage[sbuf * G::STAGE + st_rd]);
        const float4 wu = *reinterpret_cast<const float4 *>(&wus[4 * (tid & 15)]);
        if (ks * G::WK + e_px < npx) {
            float v[4] = {t.x * u_dy * wu.x, t.y * u_dy * wu.y, t.z * u_dy * wu.z, t.w * u_dy * wu.w};
            const int off = ks * (G::WK * G::CI) + 4 * tid;
            if constexpr (MASK == 1) {
                const float m[4] = {mk.q.x, mk.q.y, mk.q.z, mk.q.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = m[j] > 0.f ? v[j] : 0.f;
            } else if constexpr (MASK == 2) {
                const unsigned nib = mk.w >> ((unsigned)off & 28u);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (nib >> j) & 1u ? v[j] : 0.f;
            }
#if !(RN_BF_KO & 1)
            *reinterpret_cast<float4 *>(dx_s + off) = make_float4(v[0], v[1], v[2], v[3]);
#endif
            // (eight consecutive lanes = 32 channels of one pixel: the group rn_sign_store wants, and the bound above is uniform in it)
            if (sign_s != nullptr) rn_sign_store(sign_s, off, v[0], v[1], v[2], v[3]);
            am = fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
    };

    unsigned fa[2][2], fb[2][2];                             // transposing-read addresses: [32-column sub-tile][read 0 / 1]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            fa[t][rd] = (unsigned)G::dy_tr(wave, t, rd, lane);
            fb[t][rd] = (unsigned)(2 * G::DY_IMG + G::x_tr(t, rd, lane));
        }
    const unsigned da0 = (unsigned)G::dy_a(lane, 0);         // k-block kb: da0 ^ (kb << 6)
    unsigned st_wr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) st_wr[r] = (unsigned)G::st_wr(wave, lane, r);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e_ = 0; e_ < 16; ++e_) acc[i][j][e_] = 0.f;

    Regs r0, r1;
    load_step(0, r0);
    split_store(0, r0);
    load_step(1, r0);                                        // step 1 waits in registers for iteration 0
    MaskT mk = mask_load(0);                                 // (replaced before its first use)
    __syncthreads();
    // One K-step: `cur` holds step ks + 1 (loaded an iteration ago), `nxt` receives step ks + 2; steps past the slice load zeros.
    // The dx of step ks - 1 leaves from the stage its MFMAs filled before the last barrier.
    auto k_step = [&](int ks, int buf, Regs &cur, Regs &nxt) {
        const char *S = &lds[buf * G::BUF];
        SplitH8 sa[2], sb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            sa[t].h = bf_tr_operand(S, fa[t][0], fa[t][1]);
            sa[t].l = bf_tr_operand(S + G::DY_IMG, fa[t][0], fa[t][1]);
            sb[t].h = bf_tr_operand(S, fb[t][0], fb[t][1]);
            sb[t].l = bf_tr_operand(S + G::X_IMG, fb[t][0], fb[t][1]);
        }
        const MaskT mk_next = mask_load(ks);
        if (ks > 0) dx_store(ks - 1, buf ^ 1, mk);
        mk = mk_next;
        f32x4v dd[RN_BF_ND];
#pragma unroll
        for (int c = 0; c < RN_BF_ND; ++c) dd[c] = f32x4v{0.f, 0.f, 0.f, 0.f};
#if !(RN_BF_KO & 4)
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            const f16x8 ah = *reinterpret_cast<const f16x8 *>(S + (da0 ^ (unsigned)(kb << 6)));
            const f16x8 al = *reinterpret_cast<const f16x8 *>(S + G::DY_IMG + (da0 ^ (unsigned)(kb << 6)));
            f32x4v &d = dd[kb % RN_BF_ND];
            d = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wh[kb], d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wl[kb], d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wh[kb], d, 0, 0, 0);
        }
#endif
        f32x4v d = dd[0];
#pragma unroll
        for (int c = 1; c < RN_BF_ND; ++c) d += dd[c];
        split_store(buf ^ 1, cur);
        load_step(ks + 2, nxt);
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) RN_SPLITH_MFMA(acc[tm][tn], sa[tm], sb[tn]);
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<float *>(&stage[buf * G::STAGE + st_wr[r]]) = d[r];
        __syncthreads();
    };
    for (int ks = 0; ks < nks; ks += 2) {
        k_step(ks, 0, r0, r1);
        if (ks + 1 < nks) k_step(ks + 1, 1, r1, r0);
    }
    dx_store(nks - 1, (nks - 1) & 1, mk);
    rn_amax_note(p.dx_amax, n, am);

    if (p.colsum != nullptr) {                               // 4 waves hold partial sums of the same 256 channels: through LDS
        float (*csred)[G::CO] = reinterpret_cast<float (*)[G::CO]>(&lds[0]);      // (the planes are done with: the loop ended in a barrier)
#pragma unroll
        for (int j = 0; j < 4; ++j) csred[wave][4 * lane + j] = cs4[j];
        __syncthreads();
        atomicAdd(p.colsum + tid, csred[0][tid] + csred[1][tid] + csred[2][tid] + csred[3][tid]);
    }
    const float us = u_dy * u_x;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = tn * 32 + (lane & 31);           // contiguous: an atomic instruction covers two full 128-byte row segments
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wave * 64 + tm * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
#if RN_BF_KO & 2
                if (acc[tm][tn][e] == 1.2345e-30f)
#endif
                atomicAdd(p.dw + row * G::CI + col, acc[tm][tn][e] * us);
            }
        }
}

// dy [N, H, W, 256], x [N, H, W, 64], dx [N, H, W, 64] dense fp32; see include/retinanet_mi355x.h
extern "C" int rn_conv_bwd_1x1(const float *dy, const float *x, const void *w_split, const float *w_unscale, float *dx, float *dw,
                               float *colsum, const void *mask, int mask_mode, const float *add, void *sign_out, const void *dy_amax,
                               const void *x_amax, void *dx_amax, int N, int H, int W, int Cin, int Cout, int stride, void *stream) {
    using G = Bwd1x1Geom;
    // what is built: 64 -> 256, stride 1, no addend, two-term fp16 products with both operands' amax tables, atomic accumulation
    if (Cin != G::CI || Cout != G::CO || stride != 1 || add != nullptr) return RN_EINVAL;
    if (rn_get_fp32_mfma() != RN_FP32_SPLIT3 || rn_get_option(RN_OPT_DETERMINISTIC) != 0) return RN_EINVAL;
    if (!dy || !x || !w_split || !w_unscale || !dx || !dw || !dy_amax || !x_amax) return RN_EINVAL;
    if (mask_mode < 0 || mask_mode > 2 || (mask_mode != 0) != (mask != nullptr)) return RN_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || N > 65535 || (int64_t)H * W > 0x7fffffff / 64) return RN_EINVAL;
    if ((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dx | (uintptr_t)w_split) & 15) || (((uintptr_t)dw | (uintptr_t)colsum | (uintptr_t)w_unscale) & 3))
        return RN_EINVAL;
    if (((uintptr_t)mask & (mask_mode == 1 ? 15 : 3)) || ((uintptr_t)sign_out & 3)) return RN_EINVAL;
    Bwd1x1Args a;
    a.dy = dy; a.x = x; a.wd = reinterpret_cast<const char *>(w_split); a.w_unscale = w_unscale;
    a.dx = dx; a.dw = dw; a.colsum = colsum; a.mask = mask; a.sign_out = reinterpret_cast<unsigned *>(sign_out);
    a.dy_amax = dy_amax; a.x_amax = x_amax; a.dx_amax = dx_amax;
    a.HW = H * W;
    // K slices: about RN_BWD_FUSED_WGS workgroups in all (three rounds of the two per CU the registers allow), each slice inside one
    // image, at least 128 pixels long and a whole number of 16-pixel K-steps
    static const int wgs = rn_env_int("RN_BWD_FUSED_WGS", 1536);
    int spi = wgs / N < 1 ? 1 : wgs / N;
    int per = ((a.HW + spi - 1) / spi + G::WK - 1) / G::WK * G::WK;
    if (per < 128) per = 128;
    if (per > (1 << 20)) per = 1 << 20;                      // 1 GiB of dy: the kernel's byte offsets into a slice stay below 2^31
    a.per = per;
    a.spi = (a.HW + per - 1) / per;
    const dim3 grid((unsigned)(a.spi * N));
    if (mask_mode == 0) hipLaunchKernelGGL(conv_bwd_1x1_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else if (mask_mode == 1) hipLaunchKernelGGL(conv_bwd_1x1_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(conv_bwd_1x1_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

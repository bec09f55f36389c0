// Weight gradient of the convolutions on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulation): conv_wgrad.hip's
// reduction for the bf16 engine (conv_bf16.hip; BASELINE configs[2]).
//
// dW[co][k] = sum over pixels of dY[pixel][co] * X[pixel + tap][ci] has the REDUCTION index (pixels) as the row of both NHWC
// operands, while a 32x32x16 operand wants 8 consecutive reduction elements per lane.  The tiles are staged as they lie
// ([pixel][channel], direct-to-LDS like conv_wgrad.hip) and read through ds_read_b64_tr_b16, gfx950's transposing LDS read: per 16
// lanes a 4-pixel x 16-channel block comes back channel-major, two of them make one operand.  fp32 atomics into the same packed fp32
// [Cout][Kpad] gradient buffer the fp32 path uses.  K slices, placement, pixel table and taps: conv_wgrad_geom.h, shared with
// conv_wgrad.hip; the slice plan: conv_wgrad_plan.h.
//
// Roofline: MFMA by FLOPs (2.5 PF dense); in practice the staging bandwidth and the tile-sized atomics, for the 1x1 layers HBM.
#include "common.h"
#include "conv_wgrad_geom.h"
#include "conv_wgrad_plan.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// kk = packed-row index (tap-major, channel-minor).  Tile 128 (co) x 128 (kk), 32 pixels per K-step, K split over the grid.
struct WgradBf16Args {
    const __bf16 *dy, *x;
    float *dw;
    float *colsum;               // [Cout] += sum over pixels of dy, or NULL
    int ldy, N, Hi, Wi, Cin, Ho, Wo, Cout, kh, kw, stride, pad;
    int Kflat, Kpad;             // kh*kw*Cin and its round-up to 32
    int tiles_n, tiles, splits;
    int xcd_map;                 // 1: whole K slices per XCD (the kernel)
    int64_t pixels, per_split;   // K extent and K per slice (multiple of 32)
};

// LDS image of a staged [32 pixels][128 columns] bf16 tile (WgradBf16Geom): 256-byte rows whose 16 chunks of 16 bytes are XOR-permuted
// by fx(row), the image that serves gfx950's transposing read without bank conflicts (cdna_hip_programming.md T10 (b); operand
// addressing verified by tools/probes/tr_probe.hip).  The direct-to-LDS load fills rows linearly, so the permutation is applied on the
// load's SOURCE: the lane filling position cp of row r fetches logical chunk cp ^ fx(r).
// bid: the workgroup's id within ITS problem's range of the grid (a grouped launch holds several problems' ranges one after the other)
__device__ __forceinline__ void conv_wgrad_bf16_body(const WgradBf16Args &p, const int bid) {
    using G = WgradBf16Geom;
    constexpr int BM = 128, BN = 128, WK = G::WK, WG_ROWB = G::ROWB;
    constexpr int TB = G::TB, IA = G::IA, IB = G::IB;        // K-steps per pixel-table batch; DMA instructions per wave per K-step
    __shared__ __attribute__((aligned(16))) char lds[2][WK * (BM + BN) * 2];   // per buffer: dY [32][128], then X [32][128]
    __shared__ int4 pixtab[2][TB * WK];                      // (x byte offset of input pixel (ih0, iw0), ih0, iw0, -)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const WgradPlace place = wgrad_place(bid, p.tiles, p.splits, p.xcd_map);
    if (!place.live) return;                                 // padding of the last group of 8 slices, or of a grouped range
    const int slice = place.slice, tile = place.tile;
    const int m0 = (tile / p.tiles_n) * BM, n0 = (tile % p.tiles_n) * BN;
    WgradSlice<2, WK> sl(slice, p.per_split, p.pixels);
    const int64_t kbeg = sl.kbeg, kend = sl.kend;
    const int nks = sl.nks;
    if (nks <= 0) return;
    const int HoWo = p.Ho * p.Wo;
    const int64_t img = (int64_t)p.Hi * p.Wi * p.Cin;
    sl.locate(HoWo, p.N, img);
    // buffer descriptors: dY = this K slice only, X from the first image the slice touches (WgradSlice)
    const v4i32 rs_a = make_rsrc(p.dy + kbeg * p.ldy, (unsigned)((kend - kbeg) * p.ldy * 2));
    const v4i32 rs_b = make_rsrc(p.x + (int64_t)sl.n_first * img, (unsigned)sl.xbytes);

    // staging geometry: instruction j of wave w fills pixel rows (w*I + j)*4 + lane/16; the lane fills chunk position cp
    const int cp = lane & 15, rq = lane >> 4;
    unsigned a_voff[IA];
    WgradTap b_tap[IB];
#pragma unroll
    for (int j = 0; j < IA; ++j) {
        const int row = G::dma_row(wave, j) + rq;
        const int col = m0 + 8 * (cp ^ G::fx(row));
        a_voff[j] = col < p.ldy ? (unsigned)((row * p.ldy + col) * 2) : 0x80000000u;
    }
#pragma unroll
    for (int j = 0; j < IB; ++j) {
        const int row = G::dma_row(wave, j) + rq;
        b_tap[j] = wgrad_tap<2>(n0 + 8 * (cp ^ G::fx(row)), p.Cin, p.kw, p.Wi, p.Kflat);   // the chunk fixes (tap, first input channel)
    }

    auto fill_batch = [&](int j) {
        int4 e = make_int4(0, WGRAD_PIXEL_DEAD, 0, 0);       // past the slice: fails the row test
        if (kbeg + (int64_t)j * (TB * WK) + tid < kend) {
            const WgradPixel q = wgrad_pixel<2>(sl.rel0 + j * (TB * WK) + tid, HoWo, p.Wo, p.stride, p.pad, p.Hi, p.Wi, p.Cin);
            e = make_int4(q.off, q.ih0, q.iw0, 0);
        }
        pixtab[j & 1][tid] = e;
    };
    unsigned b_voff[IB];
    auto make_offsets = [&](int ks) {
        const int4 *tab = pixtab[(ks / TB) & 1];
#pragma unroll
        for (int j = 0; j < IB; ++j) {
            const int4 e = tab[G::tab_index(ks, wave, lane, j)];
            const bool ok = wgrad_tap_inside(e.y, e.z, b_tap[j].fr_t, b_tap[j].fs, p.Hi, p.Wi);
            b_voff[j] = ok ? (unsigned)(e.x + b_tap[j].off) : 0xFFFFFFFFu;
        }
    };
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const unsigned lds0 = lds_addr(&lds[0][0]);
    constexpr unsigned BUFB = WK * (BM + BN) * 2;
    auto dma_step = [&](int ks, int buf) {
        const unsigned A = lds0 + (unsigned)(buf * BUFB + wave_u * IA * 4 * WG_ROWB);
        const unsigned B = lds0 + (unsigned)(buf * BUFB + WK * WG_ROWB + wave_u * IB * 4 * WG_ROWB);
        const unsigned so = (unsigned)ks * (unsigned)(WK * 2) * (unsigned)p.ldy;     // scalar: the K-step advance of dY
#pragma unroll
        for (int j = 0; j < IA; ++j) dma16(rs_a, A + j * (4 * WG_ROWB), a_voff[j], so);   // a_voff[j] holds instruction j's rows
#pragma unroll
        for (int j = 0; j < IB; ++j) dma16(rs_b, B + j * (4 * WG_ROWB), b_voff[j], 0u);
    };

    // fragment read addresses (bytes within a buffer): block row r0 + q, chunk c0 + (pp >> 1), half pp & 1 (conv_wgrad_geom.h)
    unsigned fa[2][2], fb[2][2];                             // [32-column sub-tile][read 0/1]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            fa[t][rd] = (unsigned)G::tr_addr(wm, t, rd, 0, lane);
            fb[t][rd] = (unsigned)(G::IMG + G::tr_addr(wn, t, rd, 0, lane));
        }

    f32x16 acc[2][2] = {};
    float cs[2] = {0.f, 0.f};
    const bool do_cs = p.colsum != nullptr && (tile % p.tiles_n) == 0 && wn == 0;

    fill_batch(0);
    __syncthreads();
    make_offsets(0);
    dma_step(0, 0);
    rn_wait_dma();
    __syncthreads();
    for (int ks = 0; ks < nks; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nks) {
            // the table batch of step ks+1 was published by an earlier barrier: batch b is filled during step
            // b*TB - 4 (below) or before the loop (batch 0)
            make_offsets(ks + 1);
            dma_step(ks + 1, buf ^ 1);
        }
        const char *S = &lds[buf][0];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const bf16x8 a0 = wg_operand(S, fa[0][0], fa[0][1], kh), a1 = wg_operand(S, fa[1][0], fa[1][1], kh);
            const bf16x8 b0 = wg_operand(S, fb[0][0], fb[0][1], kh), b1 = wg_operand(S, fb[1][0], fb[1][1], kh);
            if (do_cs) {
#pragma unroll
                for (int e_ = 0; e_ < 8; ++e_) { cs[0] += (float)a0[e_]; cs[1] += (float)a1[e_]; }
            }
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
        // next table batch: needed from step (b+1)*TB - 1 on (make_offsets(ks + 1)); its slot held batch b-1, last read
        // for step b*TB - 1, i.e. during iteration b*TB - 2
        if ((ks % TB) == TB - 4 && (ks / TB + 1) * TB < nks) fill_batch(ks / TB + 1);
        rn_wait_dma();
        __syncthreads();
    }
    if (do_cs) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            cs[t] += __shfl_xor(cs[t], 32);                   // the two 8-pixel groups of the same channel
            const int c = m0 + wm * 64 + t * 32 + (lane & 31);
            if (lane < 32 && c < p.Cout) atomicAdd(p.colsum + c, cs[t]);
        }
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = n0 + wn * 64 + tn * 32 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wm * 64 + tm * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                if (row < p.Cout && col < p.Kflat) RN_WG_ATOMIC(p.dw + (int64_t)row * p.Kpad + col, acc[tm][tn][e]);
            }
        }
}

__global__ __launch_bounds__(256, 3) void conv_wgrad_bf16_kernel(const WgradBf16Args p) { conv_wgrad_bf16_body(p, (int)blockIdx.x); }

// Grouped launch: the pyramid levels of a head layer (D/model.py:110-205: one weight tensor convolves all five levels, so its gradient
// is the SUM over the levels) as ONE grid accumulating into one dw / colsum.  Alone, the small levels are launches of a few dozen
// microseconds at 60-270 TFLOP/s (8 x 9 x 15 ... 8 x 34 x 60 pixels); here they ride along with the big ones.
struct WgradBf16Group {
    int n;
    int block_end[RN_MAX_GROUP];         // running sum of the problems' workgroup counts (each a multiple of 8)
    WgradBf16Args p[RN_MAX_GROUP];
};
__global__ __launch_bounds__(256, 3) void conv_wgrad_bf16_grouped_kernel(const WgradBf16Group g) {
    int i = 0;
#pragma unroll
    for (int j = 0; j < RN_MAX_GROUP - 1; ++j) i += (j + 1 < g.n && (int)blockIdx.x >= g.block_end[j]) ? 1 : 0;
    i = __builtin_amdgcn_readfirstlane(i);
    conv_wgrad_bf16_body(g.p[i], (int)blockIdx.x - (i > 0 ? g.block_end[i - 1] : 0));
}

// Geometry, K slices and grid size of one weight-gradient problem; target_wgs: the workgroups it should bring to the grid.
// Returns the number of workgroups (> 0) or -RN_EINVAL.
static int64_t wgrad_bf16_fill(WgradBf16Args &a, const void *dy, int ldy, const void *x, float *dw, float *colsum, int N, int Hi, int Wi,
                               int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int target_wgs, bool pad8) {
    a.dy = reinterpret_cast<const __bf16 *>(dy); a.x = reinterpret_cast<const __bf16 *>(x); a.dw = dw; a.colsum = colsum; a.ldy = ldy;
    a.N = N; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout;
    a.kh = kh; a.kw = kw; a.stride = stride; a.pad = pad;
    a.Kflat = kh * kw * Cin;
    a.Kpad = (a.Kflat + 31) / 32 * 32;
    a.pixels = (int64_t)N * Ho * Wo;
    const int tiles_m = (Cout + 127) / 128;
    a.tiles_n = (a.Kflat + 127) / 128;
    a.tiles = tiles_m * a.tiles_n;
    static const int xcd_env = rn_env_int("RN_WGRAD_BF16_XCD", 1);
    const WgradPlanIn in = {a.pixels, a.tiles, target_wgs, WgradBf16Geom::WK, ldy, 2, (int64_t)Ho * Wo, (int64_t)Hi * Wi * Cin * 2, WGRAD_XCD_BF16, xcd_env != 0, pad8};
    WgradPlan pl;
    if (!wgrad_plan(in, pl)) return -RN_EINVAL;              // conv_wgrad_plan.h
    a.per_split = pl.per_split; a.splits = pl.splits; a.xcd_map = pl.xcd_map;
    return pl.grid;
}

// Workgroups a weight-gradient launch aims for (see rn_conv_wgrad_bf16); RN_WGRAD_BF16_WGS overrides.
static int wgrad_bf16_target_wgs() {
    static const int v = rn_env_int("RN_WGRAD_BF16_WGS", 0);
    return v > 0 ? v : 768;
}

extern "C" int rn_conv_wgrad_bf16(const void *dy, int ldy, const void *x, float *dw, float *colsum, int N, int Hi, int Wi,
                                  int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, void *stream) {
    if (N <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0 || Cin < 8 || (Cin & 7) || (ldy & 7) || ldy < Cout)
        return RN_EINVAL;
    if (((uintptr_t)dy & 15) || ((uintptr_t)x & 15)) return RN_EINVAL;
    // (A 256 x 256 eight-wave form of this reduction was built in round 4, correct and slower -- 0.51 against 0.40 ms on the head tower
    // layer, profiles/r04_wgrad_p8_knockouts.txt -- and now lives in tools/probes/quarantine_r05/.)
    const int target_wgs = wgrad_bf16_target_wgs();
    // K slices for ~768 workgroups = ONE resident round at three per CU.  Every slice ends in tile-sized fp32 atomics
    // (Cout x Kflat x slices of them per launch, ~1.3 TB/s chip-wide), and with the MFMAs eight times shorter than in the
    // fp32 kernel that tail weighs more: measured per training step (all weight gradients) 512: 11.6 ms, 768: 11.1,
    // 1024: 13.5, 1536: 13.2, 2048: 14.6, 3072: 15.2 (the fp32 kernel's optimum is 2048).  RN_WGRAD_BF16_WGS overrides.
    WgradBf16Args a;
    const int64_t blocks = wgrad_bf16_fill(a, dy, ldy, x, dw, colsum, N, Hi, Wi, Cin, Ho, Wo, Cout, kh, kw, stride, pad, target_wgs, false);
    if (blocks <= 0) return RN_EINVAL;
    hipLaunchKernelGGL(conv_wgrad_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// The weight gradients of n <= RN_MAX_GROUP problems that share ONE weight tensor (the pyramid levels of a head layer) as one launch:
// dw / colsum accumulate the sum over the problems.  Per problem i: dy[i] [N, H[i], W[i], ldy] and x[i] [N, H[i], W[i], Cin] (stride-1
// same-size geometry is NOT required: Ho / Wo follow from H, W, k, stride, pad as in rn_conv_wgrad_bf16).
extern "C" int rn_conv_wgrad_bf16_grouped(int n, const void *const *dy, int ldy, const void *const *x, float *dw, float *colsum, int N,
                                          const int *Hi, const int *Wi, int Cin, int Cout, int kh, int kw, int stride, int pad, void *stream) {
    if (n < 1 || n > RN_MAX_GROUP || N <= 0 || Cout <= 0 || Cin < 8 || (Cin & 7) || (ldy & 7) || ldy < Cout) return RN_EINVAL;
    const int target_wgs = wgrad_bf16_target_wgs();
    int Ho[RN_MAX_GROUP], Wo[RN_MAX_GROUP];
    int64_t total_pixels = 0;
    for (int i = 0; i < n; ++i) {
        if (Hi[i] <= 0 || Wi[i] <= 0 || ((uintptr_t)dy[i] & 15) || ((uintptr_t)x[i] & 15)) return RN_EINVAL;
        Ho[i] = (Hi[i] + 2 * pad - kh) / stride + 1;
        Wo[i] = (Wi[i] + 2 * pad - kw) / stride + 1;
        if (Ho[i] <= 0 || Wo[i] <= 0) return RN_EINVAL;
        total_pixels += (int64_t)N * Ho[i] * Wo[i];
    }
    WgradBf16Group g;
    g.n = n;
    int64_t end = 0;
    for (int i = 0; i < n; ++i) {
        // the problem's share of one resident round, by its pixels (at least one slice per tile: wgrad_bf16_fill)
        const int share = (int)((int64_t)target_wgs * ((int64_t)N * Ho[i] * Wo[i]) / total_pixels);
        const int64_t blocks = wgrad_bf16_fill(g.p[i], dy[i], ldy, x[i], dw, colsum, N, Hi[i], Wi[i], Cin, Ho[i], Wo[i], Cout, kh, kw, stride, pad,
                                               share, true);
        if (blocks <= 0) return RN_EINVAL;
        end += blocks;
        if (end > 0x7fffffff) return RN_EINVAL;
        g.block_end[i] = (int)end;
    }
    for (int i = n; i < RN_MAX_GROUP; ++i) g.block_end[i] = (int)end;
    hipLaunchKernelGGL(conv_wgrad_bf16_grouped_kernel, dim3((unsigned)end), dim3(256), 0, (hipStream_t)stream, g);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// Index arithmetic of the weight-gradient kernels' LDS structures, shared by the kernels (conv_wgrad.hip, conv_wgrad_bf16.hip) and
// by a HOST program (tests/test_wgrad_index_ranges.py compiles tests/wgrad_index_check.cpp with g++) that enumerates every
// lane / wave / K-step / instruction of every tile instance and checks that each index stays inside the structure it
// addresses.  Why: a logically inactive lane still forms an ADDRESS (DESIGN.md "Rules"): in round 1 a grouped-wgrad
// experiment let the lanes of the 256x64 instance index a 32-row LDS table at rows 32-63 -- a GPU memory fault on the first
// such shape.  Any change to these expressions is now checked on the host before it reaches a GPU.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RN_HD __host__ __device__ __forceinline__
#else
#define RN_HD inline
#endif

// fp32 kernel (conv_wgrad.hip): tile 64*WM x 64*WN, WK pixels per K-step, 256 threads = 4 waves.
template <int WM, int WN, int WK>
struct WgradGeom {
    static constexpr int BM = 64 * WM, BN = 64 * WN;
    static constexpr int TB = 256 / WK;                      // K-steps per pixel-table batch (one entry per thread)
    static constexpr int CA = BM / 4, CB = BN / 4;           // 16-byte chunks per tile row
    static constexpr int PA = 64 / CA, PB = 64 / CB;         // pixels one wave instruction (64 lanes x 16 B) covers
    static constexpr int IA = WK / PA / 4, IB = WK / PB / 4; // DMA instructions per wave per K-step
    static constexpr int TAB = TB * WK;                      // entries of one pixel-table half
    static constexpr int BUF = WK * (BM + BN);               // floats of one LDS buffer: A [WK][BM], then B [WK][BN]
    static_assert(PA >= 1 && PB >= 1 && IA >= 1 && IB >= 1 && TAB == 256, "tile shape");

    // pixel-table entry read by lane `lane` of wave `wave` for DMA instruction j of K-step ks (within its half)
    static RN_HD int tab_index(int ks, int wave, int lane, int j) { return (ks % TB) * WK + wave * IB * PB + lane / CB + j * PB; }
    // first float of the 256-float (1 KiB) block that DMA instruction j of wave `wave` fills, within a buffer
    static RN_HD int dma_a(int wave, int j) { return wave * (IA * PA) * BM + j * (PA * BM); }
    static RN_HD int dma_b(int wave, int j) { return WK * BM + wave * (IB * PB) * BN + j * (PB * BN); }
    // fragment reads of k-pair kp: A = 2 adjacent floats (ds_read_b64), B = floats +0 and +32 (ds_read2_b32), within a buffer
    static RN_HD int frag_a(int wm, int lane, int kp) { return ((lane >> 5) + 2 * kp) * BM + wm * 64 + 2 * (lane & 31); }
    static RN_HD int frag_b(int wn, int lane, int kp) { return WK * BM + ((lane >> 5) + 2 * kp) * BN + wn * 64 + (lane & 31); }
};

// bf16 kernel (conv_wgrad_bf16.hip): tile 128 x 128, 32 pixels per K-step, images of [32 pixels][128 columns] bf16 = 256-byte rows.
struct WgradBf16Geom {
    static constexpr int WK = 32, ROWB = 256, TB = 256 / WK, IA = WK / 4 / 4, IB = WK / 4 / 4, TAB = TB * WK;
    static constexpr int IMG = WK * ROWB;                    // bytes of one tile image; a buffer = dY image, then X image
    static RN_HD int fx(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
    static RN_HD int tab_index(int ks, int wave, int lane, int j) { return (ks % TB) * WK + wave * IB * 4 + (lane >> 4) + 4 * j; }
    static RN_HD int dma_row(int wave, int j) { return (wave * IA + j) * 4; }           // first of the 4 rows instruction j fills
    // byte address (within an image) a lane supplies to ds_read_b64_tr_b16 for read rd of 32-column sub-tile t, pixel half kh
    static RN_HD int tr_addr(int w2, int t, int rd, int kh, int lane) {
        const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
        const int row = 16 * kh + 8 * (g >> 1) + 4 * rd + q;
        const int ch = (w2 * 64 + t * 32 + 16 * (g & 1)) / 8 + (pp >> 1);
        return ROWB * row + 16 * (ch ^ fx(row)) + 8 * (pp & 1);
    }
};

#ifdef __HIPCC__
// One 32x32x16 operand from such an image (the bf16 kernel's, and the once kernel's plane): lane l <- 8 consecutive rows (pixels)
// 16*kh + 8*(l>>5) + 0..7 of column col0 + (l & 31), by two ds_read_b64_tr_b16 at tr_addr's addresses (each: a 4-row x 16-column
// block per 16 lanes, returned column-major).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 wg_operand(const char *img, unsigned a_rd0, unsigned a_rd1, int kh = 0) {
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    typedef __attribute__((address_space(3))) s16x4 *lp;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(__attribute__((address_space(3))) char *)(img + a_rd0 + kh * 16 * WgradBf16Geom::ROWB));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(__attribute__((address_space(3))) char *)(img + a_rd1 + kh * 16 * WgradBf16Geom::ROWB));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}
#endif

// fp32 split-operand kernel with the split done ONCE per workgroup (conv_wgrad.hip: conv_wgrad_once_kernel): tile 128 x 128, 16
// pixels per K-step; every thread loads two float4 (4 channels of pixels p and p + 8) of each operand into registers, splits them
// and stores the three bf16 terms into plane images [16 pixels][128 columns] bf16 -- WgradBf16Geom's image (256-byte rows, 16-byte
// chunks XOR-permuted by fx(row)) cut to 16 rows, so the MFMA operands come out of the same transposing reads (tr_addr, kh = 0).
struct WgradSplitGeom {
    static constexpr int WK = 16, ROWB = 256, TB = 256 / WK, TAB = TB * WK;
    static constexpr int IMG = WK * ROWB;                    // bytes of one plane image
    static constexpr int BUF = 6 * IMG;                      // bytes of one buffer: dY planes h, m, l, then X planes h, m, l
    static RN_HD int pixel(int tid, int half) { return (tid >> 5) + 8 * half; }          // the pixel of this thread's load `half`
    static RN_HD int chunk(int tid) { return tid & 31; }                                 // its 4-channel chunk (columns 4c .. 4c+3)
    // byte address (within a plane image) of the thread's 8-byte store of (pixel, columns 4c .. 4c+3)
    static RN_HD int wr_addr(int tid, int half) {
        const int row = pixel(tid, half), c = chunk(tid);
        return ROWB * row + 16 * ((c >> 1) ^ WgradBf16Geom::fx(row)) + 8 * (c & 1);
    }
    static RN_HD int tab_index(int ks, int tid, int half) { return (ks % TB) * WK + pixel(tid, half); }
    static RN_HD int tr_addr(int w2, int t, int rd, int lane) { return WgradBf16Geom::tr_addr(w2, t, rd, 0, lane); }
};

// ------------------------------------------------------------------------------------------------ K slices, pixels, taps
// What conv_wgrad_kernel, conv_wgrad_once_kernel and conv_wgrad_bf16_body share besides the structures above; the staging, the MFMA
// loops and the epilogues stay in the kernels.  EB = bytes per operand element (4 / 2): offsets are BYTE offsets into 32-bit buffer
// addressing, which the planner (conv_wgrad_plan.h) keeps below 2 GiB.

// Workgroup id -> (K slice, tile).  Ids are dealt round-robin to the 8 XCDs; all tiles of one K slice read the same dY / X slabs, so
// under xcd_map a slice is kept on ONE XCD (slice s on XCD s % 8, its tiles consecutive there) and the slabs stream through that L2
// once instead of through all eight; the plain order has consecutive ids = the tiles of one slice.  bid: the id within the problem's
// range of the grid, which starts at a multiple of 8 (bid & 7 is the XCD); Id: unsigned (blockIdx.x) or int (a grouped range's), the
// kernels' own types.  !live: padding of the last group of 8 slices, or of a grouped range.
struct WgradPlace { int slice, tile; bool live; };
template <class Id>
RN_HD WgradPlace wgrad_place(Id bid, int tiles, int splits, int xcd_map) {
    WgradPlace w;
    if (xcd_map) {
        const int xcd = bid & 7, wi = bid >> 3;
        w.slice = (wi / tiles) * 8 + xcd;
        w.tile = wi % tiles;
    } else {
        w.slice = bid / tiles;
        w.tile = bid % tiles;
    }
    w.live = w.slice < splits;
    return w;
}

// K slice `slice`: pixels [kbeg, kend) in nks K-steps of WK -- the dY descriptor covers exactly that range, so "pixel >= kend" is out
// of range by itself.  locate() (a second step: the kernels leave on nks <= 0 first, and the 64-bit division belongs behind that
// exit): the X descriptor starts at image n_first, the first the slice touches (pixel kbeg is its pixel rel0), and spans xbytes,
// clamped -- byte offsets are plain int32 and -1 is always out of range.  img = Hi * Wi * Cin.
template <int EB, int WK>
struct WgradSlice {
    int64_t kbeg, kend, xbytes;
    int nks, n_first, rel0;
    RN_HD WgradSlice(int slice, int64_t per_split, int64_t pixels) {
        kbeg = (int64_t)slice * per_split;
        kend = (kbeg + per_split < pixels) ? kbeg + per_split : pixels;
        nks = (int)((kend - kbeg + WK - 1) / WK);
    }
    RN_HD void locate(int HoWo, int N, int64_t img) {
        n_first = (int)(kbeg / HoWo);
        rel0 = (int)(kbeg - (int64_t)n_first * HoWo);
        xbytes = ((int64_t)N - n_first) * img * EB;
        if (xbytes > 0x7FFFFFFF) xbytes = 0x7FFFFFFF;
    }
};

// Pixel-table entry of pixel `rel` (counted from pixel 0 of image n_first): the byte offset of input pixel (ih0, iw0) channel 0 with
// ih0 = oh * stride - pad, and ih0, iw0 -- the two divisions of the (n, oh, ow) decomposition are done once per pixel for all lanes
// and taps.  A slot past the slice holds WGRAD_PIXEL_DEAD as ih0 (written in the kernels: behind this helper the fp32 instances took
// 2-4 more VGPRs), which fails the row test, also with a tap's fr_t added.
struct WgradPixel { int off, ih0, iw0; };
#define WGRAD_PIXEL_DEAD (-(1 << 28))
template <int EB>
RN_HD WgradPixel wgrad_pixel(int rel, int HoWo, int Wo, int stride, int pad, int Hi, int Wi, int Cin) {
    const unsigned n = (unsigned)rel / (unsigned)HoWo;
    const unsigned rem = (unsigned)rel - n * (unsigned)HoWo;
    const unsigned oh = rem / (unsigned)Wo, ow = rem - oh * (unsigned)Wo;
    const int ih0 = (int)oh * stride - pad, iw0 = (int)ow * stride - pad;
    const WgradPixel e = {(((int)n * Hi + ih0) * Wi + iw0) * Cin * EB, ih0, iw0};
    return e;
}
// The once kernel's 8-byte entry packs (ih0, iw0) into one word: both fit 16 bits (its launcher: Hi + pad, Wi + pad < 32000); past
// the slice ih0 = -32768.
#define WGRAD_PACKED_DEAD 0x8000
RN_HD int wgrad_pixel_pack(int ih0, int iw0) { return (int)((unsigned)(ih0 & 0xffff) | ((unsigned)iw0 << 16)); }
RN_HD int wgrad_packed_ih0(int w) { return (int)(short)(w & 0xffff); }
RN_HD int wgrad_packed_iw0(int w) { return w >> 16; }

// A 16-byte chunk of the packed row at column jcol fixes (tap, first input channel): fs, the byte offset the tap adds to a pixel's, and
// fr_t = fr, or 1 << 24 for a column past the matrix, which fails every row test.
struct WgradTap { int fr_t, fs, off; };
template <int EB>
RN_HD WgradTap wgrad_tap(int jcol, int Cin, int kw, int Wi, int Kflat) {
    const int tap = jcol / Cin;
    const int ci0 = jcol - tap * Cin;
    const int fr = tap / kw, fs = tap - fr * kw;
    WgradTap t = {jcol < Kflat ? fr : (1 << 24), fs, ((fr * Wi + fs) * Cin + ci0) * EB};
    return t;
}
// the tap's input pixel lies inside the image
RN_HD bool wgrad_tap_inside(int ih0, int iw0, int fr_t, int fs, int Hi, int Wi) {
    return ((unsigned)(ih0 + fr_t) < (unsigned)Hi) & ((unsigned)(iw0 + fs) < (unsigned)Wi);
}

// RN_WG_KO (RN_EXPERIMENT builds; timing only, wrong results): 1 = the tile-sized atomic accumulation left out, 2 = workgroup-scope atomics
#ifndef RN_WG_KO
#define RN_WG_KO 0
#endif
#if RN_WG_KO == 1
#define RN_WG_ATOMIC(P, V) do { if ((V) == 1.2345e-30f) atomicAdd((P), (V)); } while (0)
#elif RN_WG_KO == 2
#define RN_WG_ATOMIC(P, V) __hip_atomic_fetch_add((P), (V), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#else
#define RN_WG_ATOMIC(P, V) atomicAdd((P), (V))
#endif

// Split-operand implicit GEMM on 16x16x32 MFMAs (conv_igemm_mf16.hip): a staged weight plane is [rows][32 k] bf16 = 64-byte rows of
// four 16-byte chunks.  ds_read_b128 serves a wave in four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the
// same + 32 (MI355X_MICROARCH.md, LDS) -- one LDS cycle per group when its lanes hit 16 different 16-byte slots of the 256-byte bank
// row.  The first permutation of this kernel was conflict-free for 8 CONSECUTIVE lanes instead and cost half of its LDS cycles
// (SQ_LDS_BANK_CONFLICT 1.1e8 per launch): the host check enumerates the real groups.
struct Mf16Geom {
    static constexpr int ROWB = 64;
    static RN_HD int slot(int row, int chunk) { return chunk ^ (3 * ((row >> 3) & 1)); }      // where chunk (8 k values) of a row sits
    // byte address (within a plane) of the operand chunk lane `lane` reads for weight rows 16 t .. 16 t + 15: row 16 t + (lane & 15), chunk lane >> 4
    static RN_HD int read_addr(int lane, int t) { const int row = 16 * t + (lane & 15); return ROWB * row + 16 * slot(row, lane >> 4); }
    // the chunk a direct-to-LDS lane must FETCH so that it lands in its linear slot: lane -> row (lane >> 2) of a 16-row block, slot lane & 3
    static RN_HD int dma_chunk(int lane) { return (lane & 3) ^ (3 * ((lane >> 5) & 1)); }
};

// The ACTIVATION operand of the same kernel, staged (round 5): a wave's 32 tile rows x 32 fp32 values of a K-step = 128-byte rows of eight
// 16-byte chunks, filled by direct-to-LDS loads that are ROW-COALESCED -- eight consecutive lanes fetch one row's 128 bytes, a wave
// instruction eight rows -- because the vector-memory pipe pays per cache line a quarter-wave touches: the operand layout read straight
// from memory (16 lanes = 16 rows, 16 bytes each) runs at 9.2 TB/s chip-wide even out of the L2, this one at 31
// (tools/probes/a_pattern_probe.hip, profiles/r05_mf16_bounds.txt).  Lane (r = lane & 15, g = lane >> 4) then reads chunks 2g, 2g + 1 of
// row 16 sm + r by ds_read_b128; chunk c of row `row` sits at slot c ^ fz(row), chosen so that every 16-lane group of the instruction
// covers the 16 slots of the 256-byte bank row (two 128-byte rows) once.
struct Mf16AGeom {
    static constexpr int ROWB = 128, ROWS = 32, WAVE_BYTES = ROWS * ROWB;
    static RN_HD int fz(int row) { const int i = (row >> 1) & 7; return i ^ (((i + 2) & 4) >> 1); }
    // byte address (within the wave's stage) of the operand read `h` (0 / 1) of lane `lane` for row block sm
    static RN_HD int read_addr(int lane, int sm, int h) {
        const int row = 16 * sm + (lane & 15);
        return ROWB * row + 16 * ((2 * (lane >> 4) + h) ^ fz(row));
    }
    // direct-to-LDS instruction j (0 .. 3) of a wave fills rows 8 j .. 8 j + 7 linearly: lane -> row 8 j + (lane >> 3), slot lane & 7
    static RN_HD int dma_row(int lane, int j) { return 8 * j + (lane >> 3); }
    static RN_HD int dma_chunk(int lane, int j) { return (lane & 7) ^ fz(dma_row(lane, j)); }      // the chunk it must fetch
};

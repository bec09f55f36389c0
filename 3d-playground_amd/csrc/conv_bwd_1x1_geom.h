// Index arithmetic of the fused 1x1 backward kernel's LDS structures (conv_bwd_1x1.hip), shared with a HOST program
// (tests/test_bwd_fused_index_ranges.py compiles tests/bwd_fused_index_check.cpp with g++) that enumerates every thread of every
// access and checks that each address stays inside the structure it belongs to, that the stores of a K-step tile their images
// exactly once, and that each read finds the element the MFMA operand layout wants -- before any of it reaches a GPU
// (conv_wgrad_geom.h has the history of that rule).
#pragma once

#ifdef __HIPCC__
#define RN_HD __host__ __device__ __forceinline__
#else
#define RN_HD inline
#endif

// One K-step = 16 pixels.  Plane images of fp16 terms: dY [16 pixels][256 channels] (512-byte rows), X [16 pixels][64 channels]
// (128-byte rows); a buffer = dY hi, dY lo, X hi, X lo.  The 16-byte chunks (8 channels) of a row are XOR-permuted so that all three
// kinds of access are free of bank conflicts (MI355X: ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19,
// 28-31} and the same + 32; ds_read_b64_tr_b16 in two halves of 32 lanes; ds_write_b64 in four runs of 16 lanes):
//   dY: chunk c of row r sits at c ^ swd(r), swd(r) = (r & 3) << 2 | perm[r >> 2], perm = {0, 2, 3, 1}: the four rows a transposing
//       read touches land in four different 64-byte quarters of the 256-byte bank row, and the rows {0-3, 12-15} / {4-11} that share
//       a ds_read_b128 group take slot sets closed under ^1, so that the neighbouring chunk (lane group g ^ 1) never meets them;
//   X : two rows per bank row; chunk c of row r sits at c ^ swx(r), swx(r) = 4 * ((r >> 1) & 1).
struct Bwd1x1Geom {
    static constexpr int CO = 256, CI = 64, WK = 16;
    static constexpr int DY_ROWB = 2 * CO, X_ROWB = 2 * CI;
    static constexpr int DY_IMG = WK * DY_ROWB, X_IMG = WK * X_ROWB;
    static constexpr int BUF = 2 * DY_IMG + 2 * X_IMG;       // bytes of one buffer (20 KiB)
    static constexpr int ST_LD = CI + 4;                     // floats per row of the dx stage (padded: the four row groups of a store hit four bank quarters)
    static constexpr int STAGE = WK * ST_LD * 4;             // bytes of one dx stage
    static RN_HD int swd(int row) { return ((row & 3) << 2) | ((0x1320 >> (4 * (row >> 2))) & 3); }
    static RN_HD int swx(int row) { return 4 * ((row >> 1) & 1); }
    // global loads of a K-step: thread tid fetches channels 4 l .. 4 l + 3 (l = tid & 63) of dY pixels (tid >> 6) + 4 i, i = 0 .. 3 -- a wave
    // instruction is one pixel's 1 KiB -- and channels 4 (tid & 15) .. + 3 of X pixel tid >> 4
    static RN_HD int dy_pixel(int tid, int i) { return (tid >> 6) + 4 * i; }
    static RN_HD int x_pixel(int tid) { return tid >> 4; }
    // byte address (within a plane image) of the thread's 8-byte stores of those values
    static RN_HD int dy_wr(int tid, int i) {
        const int row = dy_pixel(tid, i), l = tid & 63;
        return DY_ROWB * row + 16 * ((l >> 1) ^ swd(row)) + 8 * (l & 1);
    }
    static RN_HD int x_wr(int tid) {
        const int row = x_pixel(tid), c4 = tid & 15;
        return X_ROWB * row + 16 * ((c4 >> 1) ^ swx(row)) + 8 * (c4 & 1);
    }
    // weight gradient: the address a lane supplies to ds_read_b64_tr_b16 for read rd (pixels 4 rd .. 4 rd + 3 of its half) of the
    // 32-column sub-tile t -- of wave `wave`'s 64 dY channels / of the 64 X channels.  The instruction hands lane j of a 16-lane group
    // column j of the 4 pixels x 16 columns its group addressed: v_mfma_f32_32x32x16_f16's operand [i = lane & 31][k = 8 (lane >> 5) ..]
    static RN_HD int dy_tr(int wave, int t, int rd, int lane) {
        const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
        const int row = 8 * (g >> 1) + 4 * rd + q;
        const int ch = (64 * wave + 32 * t + 16 * (g & 1)) / 8 + (pp >> 1);
        return DY_ROWB * row + 16 * (ch ^ swd(row)) + 8 * (pp & 1);
    }
    static RN_HD int x_tr(int t, int rd, int lane) {
        const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
        const int row = 8 * (g >> 1) + 4 * rd + q;
        const int ch = (32 * t + 16 * (g & 1)) / 8 + (pp >> 1);
        return X_ROWB * row + 16 * (ch ^ swx(row)) + 8 * (pp & 1);
    }
    // data gradient: v_mfma_f32_16x16x32_f16's A operand [i = lane & 15][k = 8 (lane >> 4) ..] of k-block kb (channels 32 kb .. + 31):
    // one ds_read_b128 of pixel row i, chunk 4 kb + (lane >> 4).  dy_a(lane, kb) == dy_a(lane, 0) ^ (kb << 6).
    static RN_HD int dy_a(int lane, int kb) {
        const int row = lane & 15;
        return DY_ROWB * row + 16 * ((4 * kb + (lane >> 4)) ^ swd(row));
    }
    // dx stage: the MFMA's result element r of lane `lane` in wave `wave` is (pixel 4 (lane >> 4) + r, channel 16 wave + (lane & 15));
    // thread tid then finishes channels 4 (tid & 15) .. + 3 of pixel tid >> 4: the K-step's 4 KiB of dx, contiguous over the workgroup
    static RN_HD int st_wr(int wave, int lane, int r) { return ((4 * (lane >> 4) + r) * ST_LD + 16 * wave + (lane & 15)) * 4; }
    static RN_HD int st_rd(int tid) { return ((tid >> 4) * ST_LD + 4 * (tid & 15)) * 4; }
};

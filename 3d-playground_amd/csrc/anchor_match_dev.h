// Which anchors an image's labels make positive: the one statement of the rule that the fused loss (focal_loss.hip), rn_assign and the
// need sets of the regression tower's forward (anchor_match.hip) have to agree on bit for bit.  A need set that misses one positive anchor
// of the loss hands it a tile nobody computed, and nothing raises.
//
// The rule: a label row is valid iff its class column != -1; its matching box is cols 0:4 (2D) or the min/max envelope of the 8 corners
// (directional, D/losses.py:93-107, NOT cols 16:20); IoU in fp32, one rounding per operation in calc_iou's order (D/losses.py:5-22; every
// file that includes this is compiled with -ffp-contract=off); the first maximum over the valid rows in row order (torch.max(dim=1));
// best < RN_IOU_NEG negative, best >= RN_IOU_POS positive, ignored between (D/losses.py:121-124).
#pragma once
#include "common.h"

#define RN_IOU_NEG 0.4f
#define RN_IOU_POS 0.5f

// Layout of a label row and of what the loss makes of it (D/losses.py, R/losses.py).
template <bool DIR>
struct LabelLayout {
    static constexpr int COLS = DIR ? 27 : 5;         // floats per label row
    static constexpr int CLS_COL = DIR ? 20 : 4;      // class; -1 marks an invalid (padding) row
    static constexpr int NREG = DIR ? 12 : 4;         // regression outputs per anchor
    static constexpr double NVALS = DIR ? 20.0 : 4.0; // smooth-L1 terms per positive anchor
};

static int check_args(int B, int64_t A, int C, int N) {
    if (B <= 0 || A <= 0 || C <= 0 || N < 0) return RN_EINVAL;
    if (N > RN_MAX_GT) return RN_ETOOMANY;
    if (B > 1024) return RN_EINVAL;
    if (A > 0x7fffffffLL) return RN_EINVAL;                                      // anchor / unit ids are ints; grid = B*G <= 1024*160
    return RN_OK;
}

// Row r of `rows` (global memory, or raw rows staged in LDS: the odd row stride is conflict-free across lanes) reduced to its matching
// box and validity; r >= n_rows gives an invalid row with a zero box.
template <bool DIR>
__device__ __forceinline__ void load_label_row(const float *__restrict__ rows, int n_rows, int r, float &bx1, float &by1,
                                               float &bx2, float &by2, bool &valid) {
    typedef LabelLayout<DIR> LL;
    valid = false;
    bx1 = by1 = bx2 = by2 = 0.f;
    if (r < n_rows) {
        const float *p = rows + (int64_t)r * LL::COLS;
        valid = p[LL::CLS_COL] != -1.0f;
        if (DIR) {
            bx1 = bx2 = p[0];
            by1 = by2 = p[1];
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                bx1 = fminf(bx1, p[2 * k]);
                bx2 = fmaxf(bx2, p[2 * k]);
                by1 = fminf(by1, p[2 * k + 1]);
                by2 = fmaxf(by2, p[2 * k + 1]);
            }
        } else {
            bx1 = p[0]; by1 = p[1]; bx2 = p[2]; by2 = p[3];
        }
    }
}

// calc_iou in two halves (D/losses.py:5-22): the clamped intersection of anchor a with a box, and the clamped union from the two areas.
// IoU = inter / union.  The matching callers divide only where inter > 0 -- otherwise the IoU is 0 / max(ua, 1e-8) == 0 exactly, which
// neither beats a best >= 0 nor reaches a band, and ~99 % of the pairs skip the divide -- and keep that test in their own `if`: behind
// one helper that returns the IoU with a flag, or 0, focal_kernel compiles to other code (profiles/focal_refactor_isa.txt).
__device__ __forceinline__ float box_inter(const float4 a, float gx1, float gy1, float gx2, float gy2) {
    float iw = fminf(a.z, gx2) - fmaxf(a.x, gx1);
    float ih = fminf(a.w, gy2) - fmaxf(a.y, gy1);
    iw = fmaxf(iw, 0.f);
    ih = fmaxf(ih, 0.f);
    return iw * ih;
}
__device__ __forceinline__ float box_union(float area_a, float garea, float inter) {
    return fmaxf((area_a + garea) - inter, 1e-8f);
}

// ----------------------------------------------------------------------------------------------------------
// The label set of one image, compacted to its valid rows in their original order (rn_assign, the need sets).
struct LabelLds {
    float x1[RN_MAX_GT], y1[RN_MAX_GT], x2[RN_MAX_GT], y2[RN_MAX_GT], area[RN_MAX_GT];
    int row[RN_MAX_GT];     // original row index in ann[j]
    int count;
};

// Wave 0 scans the rows in chunks of 64, ordered compaction by ballot.
template <bool DIR>
__device__ __forceinline__ void load_labels(const float *__restrict__ ann_j, int N, LabelLds &L) {
    if (threadIdx.x < 64) {
        int base = 0;
        for (int r0 = 0; r0 < N; r0 += 64) {
            const int r = r0 + threadIdx.x;
            bool valid;
            float bx1, by1, bx2, by2;
            load_label_row<DIR>(ann_j, N, r, bx1, by1, bx2, by2, valid);
            const unsigned long long m = __ballot(valid);
            if (valid) {
                const int pos = base + __popcll(m & ((1ull << threadIdx.x) - 1ull));
                L.x1[pos] = bx1; L.y1[pos] = by1; L.x2[pos] = bx2; L.y2[pos] = by2;
                L.area[pos] = (bx2 - bx1) * (by2 - by1);                       // D/losses.py:6
                L.row[pos] = r;
            }
            base += __popcll(m);
        }
        if (threadIdx.x == 0) L.count = base;
    }
    __syncthreads();
}

// IoU max / first argmax (index among the valid rows) of one anchor against the label set; a strict > keeps the first maximum.
__device__ __forceinline__ void match_anchor(const float4 a, const LabelLds &L, float &best, int &arg) {
    const float area_a = (a.z - a.x) * (a.w - a.y);
    best = -1.0f;
    arg = 0;
    for (int n = 0; n < L.count; ++n) {
        const float inter = box_inter(a, L.x1[n], L.y1[n], L.x2[n], L.y2[n]);
        float iou = 0.f;
        if (inter > 0.f) iou = inter / box_union(area_a, L.area[n], inter);
        if (iou > best) { best = iou; arg = n; }
    }
}

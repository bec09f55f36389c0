// The anchor <-> label matching rule (anchor_match_dev.h) as stand-alone operators: rn_assign (IoU max, argmax and state per anchor), the
// need sets of the regression tower's sparse forward (rn_reg_need_tiles) and calc_iou itself (rn_pairwise_iou).  The fused
// loss in focal_loss.hip takes its positives by the same rule from the same header.
#include "anchor_match_dev.h"

#define NTHR 256          // threads per workgroup, one anchor each

// ----------------------------------------------------------------------------------------------------------
template <bool DIR>
__global__ __launch_bounds__(NTHR) void assign_kernel(const float4 *__restrict__ anchors, const float *__restrict__ ann,
                                                      int64_t A, int N, float *__restrict__ iou_max,
                                                      int32_t *__restrict__ argmax, int32_t *__restrict__ state) {
    __shared__ LabelLds L;
    const int j = blockIdx.y;
    load_labels<DIR>(ann + (int64_t)j * N * LabelLayout<DIR>::COLS, N, L);
    const int64_t ai = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (ai >= A) return;
    float best = 0.f; int arg = -1; int st = 0;
    if (L.count > 0) {
        match_anchor(anchors[ai], L, best, arg);
        st = -1;
        if (best < RN_IOU_NEG) st = 0;
        if (best >= RN_IOU_POS) st = 1;
    }
    iou_max[(int64_t)j * A + ai] = best;
    argmax[(int64_t)j * A + ai] = arg;
    state[(int64_t)j * A + ai] = st;
}

extern "C" int rn_assign(const float *anchors, const float *ann, int B, int64_t A, int N, int directional,
                         float *iou_max, int32_t *argmax, int32_t *state, void *stream) {
    const int rc = check_args(B, A, 1, N);
    if (rc) return rc;
    const dim3 grid((unsigned)((A + NTHR - 1) / NTHR), B), block(NTHR);
    const float4 *anc = reinterpret_cast<const float4 *>(anchors);
    if (directional)
        hipLaunchKernelGGL(assign_kernel<true>, grid, block, 0, (hipStream_t)stream, anc, ann, A, N, iou_max, argmax, state);
    else
        hipLaunchKernelGGL(assign_kernel<false>, grid, block, 0, (hipStream_t)stream, anc, ann, A, N, iou_max, argmax, state);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ----------------------------------------------------------------------------------------------------------
// Need sets of the regression tower's forward.  The loss reads the regression output at the positive anchors only (the
// queue of focal_kernel: best IoU >= RN_IOU_POS against the image's valid labels -- the rule of anchor_match_dev.h), so the labels
// say BEFORE the forward which 4x4 output tiles of which pyramid level anybody will read: P0 = the tiles that hold a pixel with a positive
// anchor.  A 3x3 layer computed on a set S of tiles reads its input inside D(S), the 3x3 dilation of S on the tile grid of one image of
// one level, so the layers below need D^k(P0).  Flag arrays, RN_REG_NEED_ARRAYS of Tpad bytes each, in the tile order of the Winograd
// transforms (levels concatenated; image, tile row, tile column): [0] P0, [1] D^2(P0), [2] D^3, [3] D^4, [4] D^5, [5] D(P0).
struct NeedGeom {
    int n;
    int W[RN_MAX_GROUP], TH[RN_MAX_GROUP], TW[RN_MAX_GROUP];
    int64_t a_end[RN_MAX_GROUP];                 // inclusive prefix sums of the levels' anchors per image
    int64_t t_end[RN_MAX_GROUP];                 // ... and of their tiles over the whole batch
};

template <bool DIR>
__global__ __launch_bounds__(NTHR) void need_p0_kernel(const float4 *__restrict__ anchors, const float *__restrict__ ann, int64_t A, int N,
                                                       int per_pixel, const NeedGeom g, unsigned char *__restrict__ p0) {
    __shared__ LabelLds L;
    const int j = blockIdx.y;
    load_labels<DIR>(ann + (int64_t)j * N * LabelLayout<DIR>::COLS, N, L);
    const int64_t ai = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (ai >= A || L.count == 0) return;
    float best; int arg;
    match_anchor(anchors[ai], L, best, arg);
    if (!(best >= RN_IOU_POS)) return;
    int q = 0;
#pragma unroll
    for (int i = 0; i < RN_MAX_GROUP - 1; ++i) q += (i + 1 < g.n && ai >= g.a_end[i]) ? 1 : 0;
    const int64_t a_first = q ? g.a_end[q - 1] : 0, t_first = q ? g.t_end[q - 1] : 0;
    const int64_t pix = (ai - a_first) / per_pixel;
    const int h = (int)(pix / g.W[q]), w = (int)(pix - (int64_t)h * g.W[q]);
    p0[t_first + ((int64_t)j * g.TH[q] + (h >> 2)) * g.TW[q] + (w >> 2)] = 1;      // (plain byte stores of 1: no atomics)
}

// One thread per tile: its Chebyshev distance to the nearest tile of P0 on its own image's grid, up to 5, decides the five dilations.
__global__ __launch_bounds__(256) void need_dilate_kernel(const NeedGeom g, int64_t T, int64_t Tpad, unsigned char *__restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int q = 0;
#pragma unroll
    for (int i = 0; i < RN_MAX_GROUP - 1; ++i) q += (i + 1 < g.n && t >= g.t_end[i]) ? 1 : 0;
    const int64_t t_first = q ? g.t_end[q - 1] : 0;
    const int TH = g.TH[q], TW = g.TW[q];
    const int64_t local = t - t_first;
    const int64_t n = local / ((int64_t)TH * TW);
    const int r = (int)(local - n * TH * TW);
    const int th = r / TW, tw = r - th * TW;
    const unsigned char *img = flags + t_first + n * TH * TW;     // array 0: P0 of this tile's image
    int dmin = 6;
    for (int dh = -5; dh <= 5; ++dh) {
        const int th2 = th + dh;
        if ((unsigned)th2 >= (unsigned)TH) continue;
        for (int dw = -5; dw <= 5; ++dw) {
            const int tw2 = tw + dw;
            if ((unsigned)tw2 >= (unsigned)TW) continue;
            if (img[th2 * TW + tw2] != 0) {
                const int a = dh < 0 ? -dh : dh, b = dw < 0 ? -dw : dw, d = a > b ? a : b;
                dmin = d < dmin ? d : dmin;
            }
        }
    }
#pragma unroll
    for (int k = 1; k <= 4; ++k)
        if (dmin <= k + 1) flags[k * Tpad + t] = 1;
    if (dmin <= 1) flags[5 * Tpad + t] = 1;
}

__global__ __launch_bounds__(256) void need_zero_kernel(uint4 *__restrict__ p, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

extern "C" int rn_reg_need_tiles(const float *anchors, const float *ann, int B, int64_t A, int N, int directional, int n_levels,
                                 const int *H, const int *W, int per_pixel, void *flags, int64_t Tpad, void *stream) {
    const int rc = check_args(B, A, 1, N);
    if (rc) return rc;
    if (!anchors || (N > 0 && !ann) || !H || !W || !flags || n_levels < 1 || n_levels > RN_MAX_GROUP || per_pixel < 1) return RN_EINVAL;
    if (Tpad <= 0 || (Tpad & 15) || ((uintptr_t)flags & 15)) return RN_EINVAL;
    NeedGeom g = {};
    g.n = n_levels;
    int64_t a = 0, t = 0;
    for (int i = 0; i < RN_MAX_GROUP; ++i) {
        const int k = i < n_levels ? i : n_levels - 1;           // unused slots repeat the last level (never selected)
        if (H[k] <= 0 || W[k] <= 0) return RN_EINVAL;
        g.W[i] = W[k]; g.TH[i] = (H[k] + 3) / 4; g.TW[i] = (W[k] + 3) / 4;
        if (i < n_levels) { a += (int64_t)H[k] * W[k] * per_pixel; t += (int64_t)B * g.TH[i] * g.TW[i]; }
        g.a_end[i] = a; g.t_end[i] = t;
    }
    if (a != A || t > Tpad) return RN_EINVAL;                    // every anchor lies in a level, every tile in the arrays
    hipStream_t s = (hipStream_t)stream;
    const int64_t n16 = (int64_t)RN_REG_NEED_ARRAYS * Tpad / 16;       // (a kernel, not a memset node: part of a captured step like the rest)
    hipLaunchKernelGGL(need_zero_kernel, dim3(rn_blocks(n16, 256)), dim3(256), 0, s, reinterpret_cast<uint4 *>(flags), n16);
    RN_LAUNCH_CHECK();
    const dim3 grid((unsigned)((A + NTHR - 1) / NTHR), B), block(NTHR);
    const float4 *anc = reinterpret_cast<const float4 *>(anchors);
    unsigned char *f = reinterpret_cast<unsigned char *>(flags);
    if (directional) hipLaunchKernelGGL(need_p0_kernel<true>, grid, block, 0, s, anc, ann, A, N, per_pixel, g, f);
    else hipLaunchKernelGGL(need_p0_kernel<false>, grid, block, 0, s, anc, ann, A, N, per_pixel, g, f);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(need_dilate_kernel, dim3(rn_blocks(t, 256)), dim3(256), 0, s, g, t, Tpad, f);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// calc_iou as a standalone op (D/losses.py:5-22): one lane per (anchor, label) pair, label index fastest.
__global__ void pairwise_iou_kernel(const float4 *__restrict__ a, const float4 *__restrict__ b, float *__restrict__ out,
                                    int64_t A, int N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A * N) return;
    const int64_t ai = i / N;
    const int n = (int)(i - ai * N);
    const float4 p = a[ai], q = b[n];
    const float area_b = (q.z - q.x) * (q.w - q.y);
    const float inter = box_inter(p, q.x, q.y, q.z, q.w);
    // divides whatever inter is, as calc_iou does, without the matching rule's `inter > 0 ? .. : 0`: the two differ where the union is
    // NaN (non-finite boxes), and this operator returns what the reference returns for every input
    out[i] = inter / box_union((p.z - p.x) * (p.w - p.y), area_b, inter);
}

extern "C" int rn_pairwise_iou(const float *a, const float *b, float *iou, int64_t A, int N, void *stream) {
    if (A <= 0 || N <= 0) return RN_EINVAL;
    hipLaunchKernelGGL(pairwise_iou_kernel, dim3(rn_blocks(A * N, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(a), reinterpret_cast<const float4 *>(b), iou, A, N);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

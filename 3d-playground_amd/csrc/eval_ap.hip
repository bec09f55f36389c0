// Detector validation: per-class average precision of a whole dataset, device-resident.
//
// Replaces retinanet/csv_eval.py (R/ and D/ carry the same file): the selection of _get_detections (:102-123), the greedy
// matching loop of evaluate (:189-213) with compute_overlap (:21-35), and the per-class sort, cumulative sums and
// _compute_ap (:216-235, :38-62).  The reference copies every image's detections to the host and appends them one by
// one to numpy arrays; here they stay in one detection table on the device and the host reads C x (AP, count) at the end.
//   eval_select_kernel   one workgroup per image (one launch per image, stream-ordered): scores > threshold in fp32,
//                        the first max_detections of them by (score descending, index ascending) found by a radix
//                        select over the 56-bit key (f32_desc_key << 24 | index), ranked in LDS, appended as 32-byte
//                        rows at the device cursor.  The cursor is an ordinary word: launches on one stream cannot overlap.
//   eval_match_kernel    one wave per (image, class): the image's rows are walked in table order (= selected order), the
//                        lanes run over the group's annotations in chunks of 64; overlap in fp64 in the reference's
//                        operation order; first maximum by (value, lowest index); "taken" bytes per annotation in a
//                        workspace, touched only by the lane that owns the annotation
//   eval_count_kernel    num_annotations[c] = sum over the images of the group sizes (integers)
//   eval_keys_kernel / eval_hist_kernel / eval_scan_kernel / eval_scatter_kernel
//                        LSD radix sort of (class << 32 | f32_desc_key(score)) with the row position as payload: five
//                        8-bit passes, each stable (a wave places a tile of 64 rows by ballot ranks, tiles and blocks in
//                        order), so equal scores keep table order: image ascending, then selected rank
//   eval_ap_kernel       one workgroup per class: the class's range of the sorted table by binary search, integer prefix
//                        counts of TP, the reverse running maximum of the precision (exact in any order), the terms
//                        (t/N - (t-1)/N) * envelope at every true positive, summed in a fixed order
// All floating-point arithmetic is fp64, one rounding per operation (-ffp-contract=off); there are no floating-point
// atomics, so a repeated evaluation is bit-identical.  Integer LDS atomics build the histograms.
#include <math.h>

#include "common.h"
#include "wave_dev.h"

#define EV_TILE RN_EVAL_SORT_TILE
#define EV_SPAN RN_EVAL_SORT_SPAN

struct EvRow { float x1, y1, x2, y2, score; int32_t label, image, index; };     // 32 bytes, the table's row

__device__ __forceinline__ unsigned int ev_desc_key(float f) {                  // boxes.hip's f32_desc_key: larger float -> smaller key
    unsigned int u = __float_as_uint(f);
    if ((u << 1) == 0u) u = 0u;                                                 // -0.0 ranks with +0.0: the tie goes by position
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

__device__ __forceinline__ int ev_rows(const int32_t *state, int64_t cap) {     // rows in the table, clamped to its size
    const int c = state[0];
    return c < 0 ? 0 : ((int64_t)c > cap ? (int)cap : c);
}

// ------------------------------------------------------------------------------------------------ stage 1
__device__ __forceinline__ bool ev_key(const float *__restrict__ scores, int k, float thr, uint64_t *key) {
    const float s = scores[k];
    if (!(s > thr)) return false;                                               // :103, strict, fp32; NaN is dropped
    *key = ((uint64_t)ev_desc_key(s) << 24) | (uint64_t)k;
    return true;
}

__global__ __launch_bounds__(1024) void eval_select_kernel(const float *__restrict__ scores, const int64_t *__restrict__ labels,
                                                           const float *__restrict__ boxes, int64_t box_stride, int64_t box_col,
                                                           int K, int too_many, float thr, int max_det, int image, int C,
                                                           EvRow *__restrict__ table, int64_t cap, int32_t *__restrict__ state,
                                                           int32_t *__restrict__ img_rows) {
    __shared__ uint64_t sel[RN_EVAL_MAX_DET];
    __shared__ int hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ int s_remaining, s_fill;
    const int t = threadIdx.x;
    const int cur = ev_rows(state, cap);
    int status = too_many ? RN_EVAL_TOO_MANY : 0;
    int want = 0;
    if (!too_many) {
        // survivors of the threshold
        if (t < 256) hist[t] = 0;
        if (t == 0) s_fill = 0;
        __syncthreads();
        int mine = 0;
        for (int k = t; k < K; k += 1024) { uint64_t key; mine += ev_key(scores, k, thr, &key) ? 1 : 0; }
        mine = wave_sum(mine);
        if ((t & 63) == 0 && mine) atomicAdd(&hist[0], mine);
        __syncthreads();
        const int survivors = hist[0];
        want = survivors < max_det ? survivors : max_det;
        __syncthreads();
        uint64_t kth = ~(uint64_t)0;                                            // every survivor is taken
        if (want < survivors) {                                                 // the want-th smallest key, 8 bits per pass from the top
            if (t == 0) { s_prefix = 0; s_remaining = want; }
            for (int p = 6; p >= 0; --p) {
                if (t < 256) hist[t] = 0;
                __syncthreads();
                const uint64_t prefix = s_prefix;
                for (int k = t; k < K; k += 1024) {
                    uint64_t key;
                    if (ev_key(scores, k, thr, &key) && (p == 6 || (key >> (8 * (p + 1))) == prefix))
                        atomicAdd(&hist[(int)((key >> (8 * p)) & 255u)], 1);
                }
                __syncthreads();
                if (t == 0) {
                    int rem = s_remaining, b = 0;
                    while (b < 255 && hist[b] < rem) { rem -= hist[b]; ++b; }
                    s_remaining = rem;
                    s_prefix = (prefix << 8) | (uint64_t)b;
                }
                __syncthreads();
            }
            kth = s_prefix;
        }
        // the selected keys, in any order; their rank is the number of smaller keys (the keys are unique)
        if (want > 0) {
            for (int k = t; k < K; k += 1024) {
                uint64_t key;
                if (ev_key(scores, k, thr, &key) && key <= kth) {
                    const int slot = atomicAdd(&s_fill, 1);
                    if (slot < RN_EVAL_MAX_DET) sel[slot] = key;
                }
            }
        }
        __syncthreads();
        int bad = 0;
        for (int e = t; e < want; e += 1024) {
            const int64_t l = labels[(int)(sel[e] & 0xFFFFFFu)];
            bad |= (l < 0 || l >= (int64_t)C) ? 1 : 0;
        }
        bad = __syncthreads_or(bad);
        if (bad) status |= RN_EVAL_BAD_LABEL;
        if ((int64_t)cur + want > cap) status |= RN_EVAL_TABLE_FULL;
    }
    if (status) {                                                               // nothing is appended
        if (t == 0) {
            state[1] |= status;
            img_rows[2 * image] = cur;
            img_rows[2 * image + 1] = cur;
        }
        return;
    }
    for (int e = t; e < want; e += 1024) {
        const uint64_t key = sel[e];
        int rank = 0;
        for (int j = 0; j < want; ++j) rank += sel[j] < key ? 1 : 0;
        const int k = (int)(key & 0xFFFFFFu);
        const float *b = boxes + (int64_t)k * box_stride + box_col;
        EvRow r;
        r.x1 = b[0]; r.y1 = b[1]; r.x2 = b[2]; r.y2 = b[3];
        r.score = scores[k];
        r.label = (int32_t)labels[k];
        r.image = image;
        r.index = k;
        table[(int64_t)cur + rank] = r;                                         // cur + want <= cap was checked
    }
    if (t == 0) {
        state[0] = cur + want;
        img_rows[2 * image] = cur;
        img_rows[2 * image + 1] = cur + want;
    }
}

// ------------------------------------------------------------------------------------------------ stage 2
// numpy's minimum / maximum hand a NaN on (:23-31); fmin / fmax would drop it
__device__ __forceinline__ double ev_min(double a, double b) { return (a != a || b != b) ? (double)NAN : (a < b ? a : b); }
__device__ __forceinline__ double ev_max(double a, double b) { return (a != a || b != b) ? (double)NAN : (a > b ? a : b); }

// 4 waves per block, one (image, class) group per wave
__global__ __launch_bounds__(256) void eval_match_kernel(const EvRow *__restrict__ table, int64_t cap,
                                                         const int32_t *__restrict__ img_rows, int I, int C,
                                                         const double *__restrict__ ann, const int32_t *__restrict__ ann_off,
                                                         int64_t M, double iou_thr, uint8_t *__restrict__ taken,
                                                         uint8_t *__restrict__ tp) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);             // wave-uniform
    if (g >= (int64_t)I * C) return;
    const int image = (int)(g / C), cls = (int)(g % C);
    int64_t r0 = img_rows[2 * image], r1 = img_rows[2 * image + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > cap ? cap : r1;
    int64_t a0 = ann_off[g], a1 = ann_off[g + 1];
    a0 = a0 < 0 ? 0 : (a0 > M ? M : a0);
    a1 = a1 < a0 ? a0 : (a1 > M ? M : a1);
    const int n = (int)(a1 - a0);
    const double eps = 2.220446049250313e-16;                                   // np.finfo(float).eps
    for (int64_t r = r0; r < r1; ++r) {
        const EvRow d = table[r];                                               // the same row in every lane
        if (d.label != cls) continue;
        if (n == 0) {                                                           // :198-201
            if (lane == 0) tp[r] = 0;
            continue;
        }
        const double dx1 = d.x1, dy1 = d.y1, dx2 = d.x2, dy2 = d.y2;            // fp32 -> fp64 (:115)
        const double area_d = (dx2 - dx1) * (dy2 - dy1);
        double best = -INFINITY;
        int best_j = RN_NO_INDEX;
        bool nan = false;
        for (int j = lane; j < n; j += 64) {
            const double *b = ann + (a0 + j) * 4;
            const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
            const double area = (b2 - b0) * (b3 - b1);                          // :21
            double iw = ev_min(dx2, b2) - ev_max(dx1, b0);                      // :23
            double ih = ev_min(dy2, b3) - ev_max(dy1, b1);                      // :24
            iw = ev_max(iw, 0.0);                                               // :26-27
            ih = ev_max(ih, 0.0);
            double ua = (area_d + area) - iw * ih;                              // :29
            ua = ev_max(ua, eps);                                               // :31
            const double ov = (iw * ih) / ua;                                   // :33-35
            if (ov != ov) nan = true;
            else if (ov > best) { best = ov; best_j = j; }                      // j ascending: the first maximum of this lane
        }
        wave_arg_first(best, best_j, rn_gt_first<double>());                    // np.argmax: the first maximum (:204)
        int hit = 0;
        if (!__any(nan) && best >= iou_thr && best_j < n) {                     // a NaN overlap is argmax's pick and fails >= (:207)
            const int owner = best_j & 63;
            int was = 0;
            if (lane == owner) {
                was = taken[a0 + best_j];
                if (!was) taken[a0 + best_j] = 1;                               // :210
            }
            was = __shfl(was, owner, 64);
            hit = !was;
        }
        if (lane == 0) tp[r] = (uint8_t)hit;
    }
}

__global__ __launch_bounds__(256) void eval_count_kernel(const int32_t *__restrict__ ann_off, int I, int C, int64_t M,
                                                         int32_t *__restrict__ num_ann) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int64_t s = 0;
    for (int i = 0; i < I; ++i) {                                               // :192, every image, detections or not
        int64_t a0 = ann_off[(int64_t)i * C + c], a1 = ann_off[(int64_t)i * C + c + 1];
        a0 = a0 < 0 ? 0 : (a0 > M ? M : a0);
        a1 = a1 < a0 ? a0 : (a1 > M ? M : a1);
        s += a1 - a0;
    }
    num_ann[c] = (int32_t)s;
}

// ------------------------------------------------------------------------------------------------ stage 3: the sort
__global__ __launch_bounds__(256) void eval_keys_kernel(const EvRow *__restrict__ table, int64_t cap,
                                                        const int32_t *__restrict__ state, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ idx) {
    const int D = ev_rows(state, cap);
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= D) return;
    keys[r] = ((uint64_t)(uint32_t)table[r].label << 32) | (uint64_t)ev_desc_key(table[r].score);
    idx[r] = (uint32_t)r;
}

// one wave per block, block b owns rows [b * EV_SPAN, (b + 1) * EV_SPAN); hist[digit * nb + b]
__global__ __launch_bounds__(64) void eval_hist_kernel(const uint64_t *__restrict__ keys, int64_t cap,
                                                       const int32_t *__restrict__ state, int shift, int nb,
                                                       int32_t *__restrict__ hist) {
    __shared__ int cnt[256];
    const int D = ev_rows(state, cap);
    const int lane = threadIdx.x, b = blockIdx.x;
    for (int q = lane; q < 256; q += 64) cnt[q] = 0;
    __syncthreads();
    const int64_t base = (int64_t)b * EV_SPAN;
    for (int o = lane; o < EV_SPAN; o += EV_TILE) {
        const int64_t r = base + o;
        if (r < D) atomicAdd(&cnt[(int)((keys[r] >> shift) & 255u)], 1);
    }
    __syncthreads();
    for (int q = lane; q < 256; q += 64) hist[(int64_t)q * nb + b] = cnt[q];
}

// one workgroup: exclusive scan of hist[0 .. n) in place, thread t owns a contiguous piece
__global__ __launch_bounds__(1024) void eval_scan_kernel(int32_t *__restrict__ hist, int64_t n) {
    __shared__ int wave_tot[16];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t lo = (int64_t)t * per, hi = lo + per < n ? lo + per : n;
    int sum = 0;
    for (int64_t q = lo; q < hi; ++q) sum += hist[q];
    int total;
    int run = block_scan_incl<16>(sum, wave_tot, total) - sum;
    for (int64_t q = lo; q < hi; ++q) { const int v = hist[q]; hist[q] = run; run += v; }
}

__global__ __launch_bounds__(64) void eval_scatter_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                          int64_t cap, const int32_t *__restrict__ state, int shift, int nb,
                                                          const int32_t *__restrict__ hist, uint64_t *__restrict__ keys_out,
                                                          uint32_t *__restrict__ idx_out) {
    __shared__ int pos[256];
    const int D = ev_rows(state, cap);
    const int lane = threadIdx.x, b = blockIdx.x;
    const int64_t base = (int64_t)b * EV_SPAN;
    if (base >= D) return;                                                      // block-uniform
    for (int q = lane; q < 256; q += 64) pos[q] = hist[(int64_t)q * nb + b];
    __syncthreads();
    for (int o = 0; o < EV_SPAN; o += EV_TILE) {                                // tiles in order, lanes in order inside a tile
        if (base + o >= D) break;                                               // block-uniform
        const int64_t r = base + o + lane;
        const bool valid = r < D;
        uint64_t key = 0;
        uint32_t payload = 0;
        if (valid) { key = keys[r]; payload = idx[r]; }
        const int digit = (int)((key >> shift) & 255u);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (digit >> bit) & 1;
            const unsigned long long m = __ballot(valid && one);
            same &= one ? m : ~m;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull)), count = __popcll(same);
        int dst = -1;
        if (valid) dst = pos[digit] + rank;
        __syncthreads();                                                        // every lane has read pos
        if (valid && rank == count - 1) pos[digit] += count;
        __syncthreads();
        if (valid && dst >= 0 && dst < D) { keys_out[dst] = key; idx_out[dst] = payload; }
    }
}

// ------------------------------------------------------------------------------------------------ stage 3: the AP
__device__ __forceinline__ int ev_lower_bound(const uint64_t *__restrict__ keys, int D, uint64_t v) {
    int lo = 0, hi = D;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void eval_ap_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ order,
                                                      int64_t cap, const int32_t *__restrict__ state,
                                                      const uint8_t *__restrict__ tp, const int32_t *__restrict__ num_ann,
                                                      double *__restrict__ ap) {
    __shared__ int s_lo, s_hi;
    __shared__ int cnt[256];
    __shared__ double red[256];
    const int D = ev_rows(state, cap);
    const int t = threadIdx.x, c = blockIdx.x;
    const int N = num_ann[c];
    if (N <= 0) {                                                               // :216-218
        if (t == 0) ap[c] = 0.0;
        return;
    }
    if (t == 0) {
        s_lo = ev_lower_bound(keys, D, (uint64_t)c << 32);
        s_hi = ev_lower_bound(keys, D, (uint64_t)(c + 1) << 32);
    }
    __syncthreads();
    const int lo = s_lo, n = s_hi - s_lo;
    const int per = (n + 255) / 256;
    const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    const double Nd = (double)N;
    // true positives in this piece, and the largest precision inside it (:226-231)
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += tp[order[lo + i]] ? 1 : 0;
    cnt[t] = mine;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < t; ++k) before += cnt[k];
    double pmax = 0.0;
    int run = before;
    for (int i = i0; i < i1; ++i) {
        run += tp[order[lo + i]] ? 1 : 0;
        const double prec = (double)run / (double)(i + 1);                      // tp + fp = i + 1 >= 1 > eps
        pmax = prec > pmax ? prec : pmax;
    }
    red[t] = pmax;
    __syncthreads();
    double env = 0.0;                                                           // the sentinel mpre[-1] = 0 (:50)
    for (int k = t + 1; k < 256; ++k) env = red[k] > env ? red[k] : env;        // a maximum: exact in any order
    __syncthreads();
    // backwards over the piece: the envelope (:53-54), a term wherever the recall changes (:58-61) -- at every true
    // positive; the step to the sentinel mrec[-1] = 1 meets mpre = 0 and adds nothing
    double sum = 0.0;
    for (int i = i1 - 1; i >= i0; --i) {
        const double prec = (double)run / (double)(i + 1);
        env = prec > env ? prec : env;
        if (tp[order[lo + i]]) {
            sum += ((double)run / Nd - (double)(run - 1) / Nd) * env;
            --run;
        }
    }
    red[t] = sum;
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int k = 0; k < 256; ++k) total += red[k];                          // fixed order
        ap[c] = total;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rn_eval_select(const float *scores, const int64_t *labels, const float *boxes, int64_t box_stride,
                              int64_t box_col, int64_t K, float score_threshold, int max_detections, int image,
                              int64_t num_images, int num_classes, void *table, int64_t table_rows, int32_t *state,
                              int32_t *img_rows, void *stream) {
    if (K < 0 || max_detections < 0 || max_detections > RN_EVAL_MAX_DET || image < 0 || image >= num_images ||
        num_classes <= 0 || num_classes > RN_EVAL_MAX_CLASSES || table_rows < 0 || table_rows > RN_EVAL_MAX_ROWS ||
        box_col < 0 || box_stride < box_col + 4 || !state || !img_rows || (table_rows > 0 && !table) ||
        ((uintptr_t)table & 15) || (K > 0 && (!scores || !labels || !boxes)))
        return RN_EINVAL;
    const int too_many = K > RN_EVAL_MAX_K;
    hipLaunchKernelGGL(eval_select_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, scores, labels, boxes, box_stride,
                       box_col, too_many ? 0 : (int)K, too_many, score_threshold, max_detections, image, num_classes,
                       reinterpret_cast<EvRow *>(table), table_rows, state, img_rows);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_eval_match(const void *table, int64_t table_rows, const int32_t *img_rows, int64_t num_images,
                             int num_classes, const double *ann_box, const int32_t *ann_offsets, int64_t M,
                             double iou_threshold, void *taken, uint8_t *tp, int32_t *num_annotations, void *stream) {
    if (num_images < 0 || num_classes <= 0 || num_classes > RN_EVAL_MAX_CLASSES || table_rows < 0 ||
        table_rows > RN_EVAL_MAX_ROWS || M < 0 || M > 0x7fffffff || num_images * num_classes > 0x7ffffffe ||
        !ann_offsets || !num_annotations || ((uintptr_t)table & 15) || (M > 0 && (!ann_box || !taken)) ||
        (table_rows > 0 && (!table || !tp)) || (num_images > 0 && !img_rows))
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_count_kernel, dim3(rn_blocks(num_classes, 256)), dim3(256), 0, s, ann_offsets, (int)num_images,
                       num_classes, M, num_annotations);
    RN_LAUNCH_CHECK();
    if (num_images == 0) return RN_OK;
    if (M > 0) {
        hipError_t e = hipMemsetAsync(taken, 0, (size_t)M, s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(eval_match_kernel, dim3(rn_blocks(num_images * num_classes, 4)), dim3(256), 0, s,
                       reinterpret_cast<const EvRow *>(table), table_rows, img_rows, (int)num_images, num_classes, ann_box,
                       ann_offsets, M, iou_threshold, reinterpret_cast<uint8_t *>(taken), tp);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

struct EvWs { uint64_t *keys_a, *keys_b; uint32_t *idx_a; int32_t *hist; };

static int64_t ev_ws_layout(char *base, int64_t rows, EvWs *w) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *r = base ? base + o : nullptr; o += (bytes + 15) & ~(int64_t)15; return r; };
    const int64_t nb = (rows + EV_SPAN - 1) / EV_SPAN;
    EvWs t;
    t.keys_a = reinterpret_cast<uint64_t *>(take(rows * 8));
    t.keys_b = reinterpret_cast<uint64_t *>(take(rows * 8));
    t.idx_a = reinterpret_cast<uint32_t *>(take(rows * 4));
    t.hist = reinterpret_cast<int32_t *>(take(256 * nb * 4));
    if (w) *w = t;
    return o;
}

extern "C" int64_t rn_eval_ap_workspace_bytes(int64_t table_rows) {
    if (table_rows < 0 || table_rows > RN_EVAL_MAX_ROWS) return 0;
    return ev_ws_layout(nullptr, table_rows, nullptr) + 16;
}

extern "C" int rn_eval_ap(const void *table, int64_t table_rows, const int32_t *state, const uint8_t *tp,
                          const int32_t *num_annotations, int num_classes, void *workspace, double *ap, int32_t *order,
                          void *stream) {
    if (num_classes <= 0 || num_classes > RN_EVAL_MAX_CLASSES || table_rows < 0 || table_rows > RN_EVAL_MAX_ROWS ||
        !state || !num_annotations || !ap || ((uintptr_t)table & 15) || ((uintptr_t)workspace & 15) ||
        (table_rows > 0 && (!table || !tp || !workspace || !order)))
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    EvWs w = {nullptr, nullptr, nullptr, nullptr};
    if (table_rows > 0) {
        ev_ws_layout(reinterpret_cast<char *>(workspace), table_rows, &w);
        const int nb = (int)((table_rows + EV_SPAN - 1) / EV_SPAN);
        uint32_t *order_u = reinterpret_cast<uint32_t *>(order);
        hipLaunchKernelGGL(eval_keys_kernel, dim3(rn_blocks(table_rows, 256)), dim3(256), 0, s,
                           reinterpret_cast<const EvRow *>(table), table_rows, state, w.keys_a, w.idx_a);
        RN_LAUNCH_CHECK();
        // five passes: a -> b -> a -> b -> a -> b, the payload's "b" side is the caller's order
        for (int p = 0; p < 5; ++p) {
            const uint64_t *kin = (p & 1) ? w.keys_b : w.keys_a;
            uint64_t *kout = (p & 1) ? w.keys_a : w.keys_b;
            const uint32_t *iin = (p & 1) ? order_u : w.idx_a;
            uint32_t *iout = (p & 1) ? w.idx_a : order_u;
            hipLaunchKernelGGL(eval_hist_kernel, dim3(nb), dim3(64), 0, s, kin, table_rows, state, 8 * p, nb, w.hist);
            RN_LAUNCH_CHECK();
            hipLaunchKernelGGL(eval_scan_kernel, dim3(1), dim3(1024), 0, s, w.hist, (int64_t)256 * nb);
            RN_LAUNCH_CHECK();
            hipLaunchKernelGGL(eval_scatter_kernel, dim3(nb), dim3(64), 0, s, kin, iin, table_rows, state, 8 * p, nb,
                               (const int32_t *)w.hist, kout, iout);
            RN_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(eval_ap_kernel, dim3(num_classes), dim3(256), 0, s, (const uint64_t *)w.keys_b,
                       (const int32_t *)order, table_rows, state, tp, num_annotations, ap);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

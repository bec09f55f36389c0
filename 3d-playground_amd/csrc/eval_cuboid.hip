// 3D validation of the directional detector: average precision on the overlap of projected cuboids, and the corner errors of
// the matched boxes.  There is no counterpart in the reference (its csv_eval.py would read two corner points as a box); the
// matching rule is the reference's (csv_eval.py:189-213), on a new overlap.  Upstream of this file are rn_eval_select's row
// table and rn_eval_ap's sort and AP (eval_ap.hip), which are used as they are.
//   cuboid_corners_kernel   the 16 corner coordinates of the rows one image appended, copied beside the table
//   cuboid_overlap_kernel   one wave per (image, class): the group's rows, 64 table rows at a time, times the group's
//                           annotations are PAIRS, and the pairs are dealt over the lanes.  A lane computes one pair: the convex
//                           hull of the detection's corners and of the annotation's (monotone chain on the points sorted by
//                           (x, y), exact duplicates dropped, a cross product <= 0 pops), Sutherland-Hodgman clipping of the
//                           first hull by the edges of the second, shoelace areas.  The first maximum per row over all of the
//                           group's annotations by wave_arg_first / rn_gt_first
//   cuboid_assign_kernel    one thread per (group, threshold): the rows in table order; a true positive iff best_iou >= t and
//                           the candidate has not been taken at t
//   cuboid_terms_kernel     one thread per row: corner errors of the true positives at thresholds[0]
//   cuboid_sums_kernel      one wave per class: the per-class sums, added in table order by one lane from values the wave
//                           loaded together -- no floating-point atomics, the same bits every run
// All arithmetic is fp64 with one rounding per operation (-ffp-contract=off), detection corners widened from fp32.
// The vertex buffers of a lane (two of RN_EVAL_CUBOID_MAX_VERTS vertices, indexed at run time) live in LDS as [vertex][lane]
// -- as private arrays they would go to scratch --: 64 lanes x 2 x 16 x 16 B = 32 KB per wave, one wave per workgroup.
#include <math.h>

#include "common.h"
#include "wave_dev.h"

#define CB_MAXV RN_EVAL_CUBOID_MAX_VERTS
#define CB_EPS 2.220446049250313e-16                                            // np.finfo(float).eps, as compute_overlap clamps the union

struct CbRow { float x1, y1, x2, y2, score; int32_t label, image, index; };     // eval_ap.hip's EvRow: the table's 32-byte row

typedef double2 (*CbBuf)[RN_WAVE];                                              // a lane's vertex k is buf[k][lane]

__device__ __forceinline__ int cb_rows(const int32_t *state, int64_t cap) {
    const int c = state[0];
    return c < 0 ? 0 : ((int64_t)c > cap ? (int)cap : c);
}

__device__ __forceinline__ void cb_group(const int32_t *__restrict__ img_rows, const int32_t *__restrict__ ann_off, int64_t g,
                                         int image, int64_t cap, int64_t M, int64_t &r0, int64_t &r1, int64_t &a0, int &n) {
    r0 = img_rows[2 * image];
    r1 = img_rows[2 * image + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > cap ? cap : r1;
    int64_t b0 = ann_off[g], b1 = ann_off[g + 1];
    b0 = b0 < 0 ? 0 : (b0 > M ? M : b0);
    b1 = b1 < b0 ? b0 : (b1 > M ? M : b1);
    a0 = b0;
    n = (int)(b1 - b0);
}

// (a - o) x (b - o): two differences per factor, two products, one difference
__device__ __forceinline__ double cb_cross(double2 o, double2 a, double2 b) {
    return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x);
}

// `count` points from src (x, y pairs) into P, sorted by (x, y) by a stable insertion, then exact duplicates dropped (the first
// of equals stays).  Returns the number of points left; `finite` is cleared by a NaN or an infinity.
template <typename T>
__device__ __forceinline__ int cb_load(CbBuf P, int lane, const T *__restrict__ src, int count, bool &finite) {
    for (int i = 0; i < count; ++i) {
        double2 p;
        p.x = (double)src[2 * i];
        p.y = (double)src[2 * i + 1];
        if (!(fabs(p.x) <= 1.7976931348623157e308) || !(fabs(p.y) <= 1.7976931348623157e308)) finite = false;
        int j = i;
        while (j > 0) {
            const double2 q = P[j - 1][lane];
            if (p.x < q.x || (p.x == q.x && p.y < q.y)) { P[j][lane] = q; --j; } else break;
        }
        P[j][lane] = p;
    }
    int m = 0;
    for (int i = 0; i < count; ++i) {
        const double2 p = P[i][lane];
        bool dup = false;
        if (m > 0) { const double2 q = P[m - 1][lane]; dup = p.x == q.x && p.y == q.y; }
        if (!dup) { P[m][lane] = p; ++m; }
    }
    return m;
}

// Monotone chain over the n sorted points of P into H (at most n + 1 <= 9 entries while it runs).  Returns the number of hull
// vertices, counter-clockwise in (x right, y up); n < 3 is returned as it is, all points collinear gives 2.
__device__ __forceinline__ int cb_hull(CbBuf P, CbBuf H, int lane, int n) {
    if (n < 3) return n;
    int k = 0;
    for (int i = 0; i < n; ++i) {
        const double2 p = P[i][lane];
        while (k >= 2 && cb_cross(H[k - 2][lane], H[k - 1][lane], p) <= 0.0) --k;
        H[k][lane] = p;
        ++k;
    }
    const int t = k + 1;
    for (int i = n - 2; i >= 0; --i) {
        const double2 p = P[i][lane];
        while (k >= t && cb_cross(H[k - 2][lane], H[k - 1][lane], p) <= 0.0) --k;
        H[k][lane] = p;
        ++k;
    }
    return k - 1;
}

// Shoelace as the fan of triangles from vertex 0, in vertex order: the products are of differences, not of frame coordinates
__device__ __forceinline__ double cb_area(CbBuf H, int lane, int m) {
    double s = 0.0;
    const double2 o = H[0][lane];
    double2 a = H[1][lane];
    for (int i = 1; i + 1 < m; ++i) {
        const double2 b = H[i + 1][lane];
        s += cb_cross(o, a, b);
        a = b;
    }
    return 0.5 * s;
}

__device__ __forceinline__ void cb_emit(CbBuf out, int lane, int &o, double2 p) {
    if (o < CB_MAXV) { out[o][lane] = p; ++o; }                                 // a 17th vertex is dropped: never for convex input
}

// One Sutherland-Hodgman step: the polygon in[0 .. cnt) cut by the half-plane left of c1 -> c2 (on the line is inside)
__device__ __forceinline__ int cb_clip(CbBuf in, CbBuf out, int lane, int cnt, double2 c1, double2 c2) {
    int o = 0;
    double2 s = in[cnt - 1][lane];
    double ds = cb_cross(c1, c2, s);
    for (int i = 0; i < cnt; ++i) {
        const double2 e = in[i][lane];
        const double de = cb_cross(c1, c2, e);
        const bool cut = de >= 0.0 ? ds < 0.0 : ds >= 0.0;
        if (cut) {
            const double t = ds / (ds - de);
            double2 x;
            x.x = s.x + t * (e.x - s.x);
            x.y = s.y + t * (e.y - s.y);
            cb_emit(out, lane, o, x);
        }
        if (de >= 0.0) cb_emit(out, lane, o, e);
        s = e;
        ds = de;
    }
    return o;
}

// The overlap of one detection (fp32 corners) and one annotation (fp64 corners): `count` points each
__device__ __forceinline__ double cb_pair_iou(CbBuf A, CbBuf B, int lane, const float *__restrict__ det,
                                              const double *__restrict__ ann, int count) {
    bool finite = true;
    const int nb = cb_load(A, lane, ann, count, finite);
    const int mb = cb_hull(A, B, lane, nb);
    double2 c[8];                                                               // the clip polygon, indexed statically below
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = B[k][lane];
    const double area_b = mb >= 3 ? cb_area(B, lane, mb) : 0.0;
    const int na = cb_load(A, lane, det, count, finite);
    const int ma = cb_hull(A, B, lane, na);
    if (!finite || mb < 3 || ma < 3) return 0.0;
    const double area_a = cb_area(B, lane, ma);
    int cnt = ma;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (e < mb && cnt > 0) {
            const double2 c2 = (e + 1 < mb) ? c[e + 1 < 8 ? e + 1 : 0] : c[0];
            cnt = (e & 1) ? cb_clip(A, B, lane, cnt, c[e], c2) : cb_clip(B, A, lane, cnt, c[e], c2);
        }
    }
    double inter = cnt >= 3 ? cb_area((mb & 1) ? A : B, lane, cnt) : 0.0;
    const double lim = area_a < area_b ? area_a : area_b;
    if (!(inter >= 0.0)) inter = 0.0;                                           // also a NaN from an overflow
    if (inter > lim) inter = lim;
    double ua = (area_a + area_b) - inter;
    ua = ua > CB_EPS ? ua : CB_EPS;
    const double iou = inter / ua;
    return iou == iou ? iou : 0.0;
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void cuboid_corners_kernel(const float *__restrict__ boxes, int64_t box_stride, int64_t K,
                                                             int image, const int32_t *__restrict__ img_rows,
                                                             const CbRow *__restrict__ table, int64_t cap,
                                                             float *__restrict__ corners) {
    int64_t r0 = img_rows[2 * image], r1 = img_rows[2 * image + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > cap ? cap : r1;
    const int64_t total = (r1 - r0) * 16;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = r0 + (e >> 4);
        const int col = (int)(e & 15);
        const int64_t k = table[r].index;
        if (k >= 0 && k < K) corners[r * 16 + col] = boxes[k * box_stride + col];
    }
}

__global__ __launch_bounds__(64) void cuboid_overlap_kernel(const CbRow *__restrict__ table, int64_t cap,
                                                            const int32_t *__restrict__ img_rows, int I, int C,
                                                            const float *__restrict__ corners, const double *__restrict__ ann,
                                                            const int32_t *__restrict__ ann_off, int64_t M, int first, int count,
                                                            double *__restrict__ best_iou, int32_t *__restrict__ best_ann) {
    __shared__ double2 s_v[2][CB_MAXV][RN_WAVE];
    __shared__ double s_bv[RN_WAVE];
    __shared__ int s_bj[RN_WAVE], s_row[RN_WAVE];
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    if (g >= (int64_t)I * C) return;
    const int image = (int)(g / C), cls = (int)(g % C);
    int64_t r0, r1, a0;
    int n;
    cb_group(img_rows, ann_off, g, image, cap, M, r0, r1, a0, n);
    const rn_gt_first<double> before;
    for (int64_t base = r0; base < r1; base += RN_WAVE) {
        const int64_t r = base + lane;
        const bool mine = r < r1 && table[r].label == cls;
        const unsigned long long mask = __ballot(mine);
        const int m = __popcll(mask);
        if (m == 0) continue;                                                   // wave-uniform
        if (mine) s_row[__popcll(mask & ((1ull << lane) - 1ull))] = (int)r;     // r < RN_EVAL_MAX_ROWS
        if (lane < m) { s_bv[lane] = n ? -INFINITY : 0.0; s_bj[lane] = n ? RN_NO_INDEX : -1; }
        __syncthreads();
        const int64_t pairs = (int64_t)m * n;
        for (int64_t pb = 0; pb < pairs; pb += RN_WAVE) {
            const int64_t p = pb + lane;
            int q = -1, j = RN_NO_INDEX;
            double v = -INFINITY;
            if (p < pairs) {
                q = (int)(p / n);
                j = (int)(p - (int64_t)q * n);
                v = cb_pair_iou(s_v[0], s_v[1], lane, corners + (int64_t)s_row[q] * 16 + 2 * first,
                                ann + (a0 + j) * 16 + 2 * first, count);
            }
            const int64_t last = pb + RN_WAVE - 1 < pairs - 1 ? pb + RN_WAVE - 1 : pairs - 1;
            const int q_lo = (int)(pb / n), q_hi = (int)(last / n);
            for (int qq = q_lo; qq <= q_hi; ++qq) {                             // the rows this pass touches, wave-uniform
                double rv = q == qq ? v : -INFINITY;
                int ri = q == qq ? j : RN_NO_INDEX;
                wave_arg_first(rv, ri, before);
                if (lane == 0 && before(rv, ri, s_bv[qq], s_bj[qq])) { s_bv[qq] = rv; s_bj[qq] = ri; }
            }
        }
        __syncthreads();
        if (lane < m) { best_iou[s_row[lane]] = s_bv[lane]; best_ann[s_row[lane]] = s_bj[lane]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cuboid_count_kernel(const int32_t *__restrict__ ann_off, int I, int C, int64_t M,
                                                           int32_t *__restrict__ num_ann) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int64_t s = 0;
    for (int i = 0; i < I; ++i) {
        int64_t a0 = ann_off[(int64_t)i * C + c], a1 = ann_off[(int64_t)i * C + c + 1];
        a0 = a0 < 0 ? 0 : (a0 > M ? M : a0);
        a1 = a1 < a0 ? a0 : (a1 > M ? M : a1);
        s += a1 - a0;
    }
    num_ann[c] = (int32_t)s;
}

__global__ __launch_bounds__(256) void cuboid_assign_kernel(const CbRow *__restrict__ table, int64_t cap,
                                                            const int32_t *__restrict__ img_rows, int I, int C,
                                                            const int32_t *__restrict__ ann_off, int64_t M,
                                                            const double *__restrict__ best_iou,
                                                            const int32_t *__restrict__ best_ann,
                                                            const double *__restrict__ thresholds, int T,
                                                            uint8_t *__restrict__ taken, uint8_t *__restrict__ tp,
                                                            int32_t *__restrict__ matched) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)I * C * T) return;
    const int t = (int)(id % T);
    const int64_t g = id / T;
    const int image = (int)(g / C), cls = (int)(g % C);
    int64_t r0, r1, a0;
    int n;
    cb_group(img_rows, ann_off, g, image, cap, M, r0, r1, a0, n);
    const double thr = thresholds[t];
    uint8_t *mine = taken + (int64_t)t * M + a0;                                // this thread's n bytes
    for (int64_t r = r0; r < r1; ++r) {
        if (table[r].label != cls) continue;
        const int a = best_ann[r];
        int hit = 0;
        if (a >= 0 && a < n && best_iou[r] >= thr && !mine[a]) { mine[a] = 1; hit = 1; }
        tp[(int64_t)t * cap + r] = (uint8_t)hit;
        if (t == 0) matched[r] = hit ? a : -1;
    }
}

// terms [rows, 4]: best_iou, corner_px, corner_px / diag, corner_px of the reversed detection -- of a true positive, else zeros
__global__ __launch_bounds__(256) void cuboid_terms_kernel(const CbRow *__restrict__ table, int64_t cap,
                                                           const int32_t *__restrict__ state, int I, int C,
                                                           const float *__restrict__ corners, const double *__restrict__ ann,
                                                           const int32_t *__restrict__ ann_off, int64_t M,
                                                           const uint8_t *__restrict__ tp, const int32_t *__restrict__ matched,
                                                           const double *__restrict__ best_iou, double *__restrict__ terms) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= cap) return;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    if (r < cb_rows(state, cap) && tp[r]) {
        const CbRow d = table[r];
        if (d.image >= 0 && d.image < I && d.label >= 0 && d.label < C) {
            int64_t a0 = ann_off[(int64_t)d.image * C + d.label];
            a0 = a0 < 0 ? 0 : a0;
            const int64_t a = a0 + matched[r];
            if (matched[r] >= 0 && a < M) {
                const double *b = ann + a * 16;
                const float *p = corners + r * 16;
                double fwd = 0.0, rev = 0.0, x0 = b[0], x1 = b[0], y0 = b[1], y1 = b[1];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int kr = (k & 4) | (3 - (k & 3));                     // 3 2 1 0 7 6 5 4: turned by 180 degrees
                    const double bx = b[2 * k], by = b[2 * k + 1];
                    const double dx = (double)p[2 * k] - bx, dy = (double)p[2 * k + 1] - by;
                    const double ex = (double)p[2 * kr] - bx, ey = (double)p[2 * kr + 1] - by;
                    fwd += sqrt(dx * dx + dy * dy);
                    rev += sqrt(ex * ex + ey * ey);
                    x0 = bx < x0 ? bx : x0;
                    x1 = bx > x1 ? bx : x1;
                    y0 = by < y0 ? by : y0;
                    y1 = by > y1 ? by : y1;
                }
                const double w = x1 - x0, h = y1 - y0;
                double diag = sqrt(w * w + h * h);
                diag = diag > CB_EPS ? diag : CB_EPS;
                t0 = best_iou[r];
                t1 = fwd / 8.0;
                t2 = t1 / diag;
                t3 = rev / 8.0;
            }
        }
    }
    terms[r * 4 + 0] = t0;
    terms[r * 4 + 1] = t1;
    terms[r * 4 + 2] = t2;
    terms[r * 4 + 3] = t3;
}

// sums [C, 5]: n_tp, sum best_iou, sum corner_px, sum corner_px / diag, n_reversed.  One wave per class; 64 rows are loaded
// together and lane 0's accumulators take them one by one, in table order.
__global__ __launch_bounds__(64) void cuboid_sums_kernel(const CbRow *__restrict__ table, int64_t cap,
                                                         const int32_t *__restrict__ state, const uint8_t *__restrict__ tp,
                                                         const double *__restrict__ terms, double *__restrict__ sums) {
    const int lane = threadIdx.x, c = blockIdx.x;
    const int D = cb_rows(state, cap);
    double n_tp = 0.0, s_iou = 0.0, s_px = 0.0, s_rel = 0.0, n_rev = 0.0;
    for (int64_t base = 0; base < D; base += RN_WAVE) {
        const int64_t r = base + lane;
        const bool on = r < D && tp[r] && table[r].label == c;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
        if (on) { v0 = terms[r * 4]; v1 = terms[r * 4 + 1]; v2 = terms[r * 4 + 2]; v3 = terms[r * 4 + 3]; }
        unsigned long long mask = __ballot(on);
        while (mask) {                                                          // wave-uniform
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const double w0 = __shfl(v0, k, RN_WAVE), w1 = __shfl(v1, k, RN_WAVE), w2 = __shfl(v2, k, RN_WAVE),
                         w3 = __shfl(v3, k, RN_WAVE);
            n_tp += 1.0;
            s_iou += w0;
            s_px += w1;
            s_rel += w2;
            n_rev += w3 < w1 ? 1.0 : 0.0;
        }
    }
    if (lane == 0) {
        sums[c * 5 + 0] = n_tp;
        sums[c * 5 + 1] = s_iou;
        sums[c * 5 + 2] = s_px;
        sums[c * 5 + 3] = s_rel;
        sums[c * 5 + 4] = n_rev;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static bool cb_bad_shape(int64_t table_rows, int64_t num_images, int num_classes, int64_t M) {
    return num_images < 0 || num_classes <= 0 || num_classes > RN_EVAL_MAX_CLASSES || table_rows < 0 ||
           table_rows > RN_EVAL_MAX_ROWS || M < 0 || M > 0x7fffffff || num_images * num_classes > 0x7ffffffe;
}

extern "C" int rn_eval_corners(const float *boxes, int64_t box_stride, int64_t K, int image, int64_t num_images,
                               const int32_t *img_rows, const void *table, int64_t table_rows, float *corners, void *stream) {
    if (K < 0 || K > RN_EVAL_MAX_K || box_stride < 16 || image < 0 || image >= num_images || !img_rows || table_rows < 0 ||
        table_rows > RN_EVAL_MAX_ROWS || ((uintptr_t)table & 15) || (table_rows > 0 && (!table || !corners)) || (K > 0 && !boxes))
        return RN_EINVAL;
    if (K == 0 || table_rows == 0) return RN_OK;
    hipLaunchKernelGGL(cuboid_corners_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, boxes, box_stride, K, image, img_rows,
                       reinterpret_cast<const CbRow *>(table), table_rows, corners);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_eval_cuboid_overlap(const void *table, int64_t table_rows, const int32_t *img_rows, int64_t num_images,
                                      int num_classes, const float *corners, const double *ann_corners,
                                      const int32_t *ann_offsets, int64_t M, int overlap, double *best_iou, int32_t *best_ann,
                                      void *stream) {
    if (cb_bad_shape(table_rows, num_images, num_classes, M) || overlap < 0 || overlap > 2 || !ann_offsets ||
        ((uintptr_t)table & 15) || (M > 0 && !ann_corners) || (table_rows > 0 && (!table || !corners || !best_iou || !best_ann)) ||
        (num_images > 0 && !img_rows))
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (table_rows == 0) return RN_OK;
    hipError_t e = hipMemsetAsync(best_iou, 0, (size_t)table_rows * 8, s);      // rows behind the cursor: 0.0 and -1
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(best_ann, 0xFF, (size_t)table_rows * 4, s);
    if (e != hipSuccess) return (int)e;
    if (num_images == 0) return RN_OK;
    const int first = overlap == RN_EVAL_CUBOID_TOP ? 4 : 0, count = overlap == RN_EVAL_CUBOID_SILHOUETTE ? 8 : 4;
    hipLaunchKernelGGL(cuboid_overlap_kernel, dim3((unsigned)(num_images * num_classes)), dim3(64), 0, s,
                       reinterpret_cast<const CbRow *>(table), table_rows, img_rows, (int)num_images, num_classes, corners,
                       ann_corners, ann_offsets, M, first, count, best_iou, best_ann);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_eval_cuboid_assign(const void *table, int64_t table_rows, const int32_t *img_rows, int64_t num_images,
                                     int num_classes, const int32_t *ann_offsets, int64_t M, const double *best_iou,
                                     const int32_t *best_ann, const double *thresholds, int num_thresholds, void *taken,
                                     uint8_t *tp, int32_t *num_annotations, int32_t *matched, void *stream) {
    if (cb_bad_shape(table_rows, num_images, num_classes, M) || num_thresholds < 1 ||
        num_thresholds > RN_EVAL_CUBOID_MAX_THRESHOLDS || !thresholds || !ann_offsets || !num_annotations ||
        ((uintptr_t)table & 15) || (M > 0 && !taken) || (table_rows > 0 && (!table || !best_iou || !best_ann || !tp || !matched)) ||
        (num_images > 0 && !img_rows) || num_images * num_classes * num_thresholds > 0x7ffffffe)
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cuboid_count_kernel, dim3(rn_blocks(num_classes, 256)), dim3(256), 0, s, ann_offsets, (int)num_images,
                       num_classes, M, num_annotations);
    RN_LAUNCH_CHECK();
    hipError_t e;
    if (table_rows > 0) {
        e = hipMemsetAsync(tp, 0, (size_t)table_rows * num_thresholds, s);
        if (e != hipSuccess) return (int)e;
        e = hipMemsetAsync(matched, 0xFF, (size_t)table_rows * 4, s);
        if (e != hipSuccess) return (int)e;
    }
    if (num_images == 0 || table_rows == 0) return RN_OK;
    if (M > 0) {
        e = hipMemsetAsync(taken, 0, (size_t)M * num_thresholds, s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(cuboid_assign_kernel, dim3(rn_blocks(num_images * num_classes * num_thresholds, 256)), dim3(256), 0, s,
                       reinterpret_cast<const CbRow *>(table), table_rows, img_rows, (int)num_images, num_classes, ann_offsets, M,
                       best_iou, best_ann, thresholds, num_thresholds, reinterpret_cast<uint8_t *>(taken), tp, matched);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

extern "C" int rn_eval_cuboid_errors(const void *table, int64_t table_rows, const int32_t *state, int64_t num_images,
                                     int num_classes, const float *corners, const double *ann_corners,
                                     const int32_t *ann_offsets, int64_t M, const uint8_t *tp, const int32_t *matched,
                                     const double *best_iou, double *terms, double *sums, void *stream) {
    if (cb_bad_shape(table_rows, num_images, num_classes, M) || !state || !ann_offsets || !sums || ((uintptr_t)table & 15) ||
        (M > 0 && !ann_corners) || (table_rows > 0 && (!table || !corners || !tp || !matched || !best_iou || !terms)))
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (table_rows > 0) {
        hipLaunchKernelGGL(cuboid_terms_kernel, dim3(rn_blocks(table_rows, 256)), dim3(256), 0, s,
                           reinterpret_cast<const CbRow *>(table), table_rows, state, (int)num_images, num_classes, corners,
                           ann_corners, ann_offsets, M, tp, matched, best_iou, terms);
        RN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cuboid_sums_kernel, dim3(num_classes), dim3(64), 0, s, reinterpret_cast<const CbRow *>(table), table_rows,
                       state, tp, (const double *)terms, sums);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

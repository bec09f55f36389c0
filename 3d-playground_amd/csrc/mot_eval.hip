// Scoring of tracking output against ground truth, device-resident: MOT_Evaluator.evaluate (mot_evaluator.py:120-412).
//
// The reference walks the frames in Python: six homography calls per frame, a double loop calling self.iou for every
// ground-truth x prediction pair, scipy's assignment, and list bookkeeping per match.  Here all frames of a sequence are
// packed into flat arrays with per-frame offsets (gt_off / pr_off [F+1]; a frame missing from one side has a count of 0
// there), uploaded once, and scored by five launches:
//   rn_mot_prepare        one lane per object.  Ground truth: guess -> im_to_state -> state_to_im -> height_from_template ->
//                         im_to_state (:169-176, hg_im_to_state_refined of homography_dev.h with fp64 boxes, the refined
//                         height stays fp64), velocity appended (:178-179), fp32 footprint of state_to_space (:201-207).
//                         Predictions: footprint (:209-215) and image corners (:194-195).
//   rn_mot_iou            every frame's n_gt x n_pred matrix, grid over frames x tiles of 256 cells (:219-222)
//   rn_mot_assign         one wave64 per frame: scipy's solver (lsap_dev.h) on the negated matrix (:225), the assigned pairs
//                         written in ascending ground-truth row into the frame's slots (slot_off: prefix sum of min(n_gt,n_pred))
//   rn_mot_frame_metrics  one wave64 per frame: threshold (:229-238), the outside-the-frame test of unassigned predictions
//                         (:283-290), per match the error vectors (:301-310), the confusion cell (:314-325) and the ids
//   rn_mot_reduce         ONE workgroup: counters (:135-152, 294-299), unique ids, fragmentations and ID switches (:328-341,
//                         364-376), confusion matrix, and the sums of every (mean, deviation) figure (:384-397)
// Arithmetic widths (each read from the reference's operand types, -ffp-contract=off):
//   IoU        every step fp32: `a` is a row of an fp32 tensor and `b` an fp32 numpy row; Python's max(x, y) is
//              `y if y > x else x` (a NaN second operand is dropped), 1e-06 rounds to fp32 in the sum; the fp32 quotient
//              (a division, or reciprocal times numerator where the numerator is a numpy scalar) widens exactly into the
//              fp64 matrix
//   state_err  fp32, clamp keeps NaN;  im_bot_err / im_top_err  fp64 (both operands are fp64 image points)
//   figures    the reference sums the fp32 stack in fp32 and the lists with numpy's pairwise order; here every sum is fp64
//              in ONE fixed order (slot k -> partial k % 256, partials added in increasing order; two passes), so two
//              evaluations agree bit for bit and tests/mot_cases.py can restate the order
// Bounds: a frame holds at most RN_MOT_MAX objects on either side, so the solver's vectors (42 bytes per object, 21.5 KiB)
// sit in the LDS of the frame's workgroup and a frame costs at most RN_MOT_MAX augmentations of RN_MOT_MAX steps.  A larger
// frame is refused before any launch (RN_EINVAL); the kernels also guard it (status 3).  A NaN or +inf IoU gives status 1
// (scipy raises ValueError), no finite assignment status 2.  No kernel waits on another workgroup or spins on memory.
#include "common.h"
#include "homography_dev.h"
#include "lsap_dev.h"

#define MOT_BLOCK 256

// ---------------------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void mot_prepare_kernel(const double *__restrict__ gt_im, const float *__restrict__ gt_h0,
                                                          const float *__restrict__ gt_vel, int64_t G,
                                                          const float *__restrict__ pred_state, int64_t M,
                                                          const double *__restrict__ H, const double *__restrict__ P,
                                                          float *__restrict__ gt_state, float *__restrict__ gt_box,
                                                          float *__restrict__ pred_box, double *__restrict__ pred_im) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < G) {
        const double2 *p = reinterpret_cast<const double2 *>(gt_im + i * 16);
        double2 pt[8];
        double bx[8], by[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { pt[k] = p[k]; bx[k] = pt[k].x; by[k] = pt[k].y; }
        float st[6];
        hg_im_to_state_refined<double>(pt, bx, by, gt_h0[i], true, H, nullptr, P, nullptr, 0, st);
        const float4 fp = hg_footprint(st);
        float *o = gt_state + i * 7;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = st[k];
        o[6] = gt_vel[i];
        reinterpret_cast<float4 *>(gt_box)[i] = fp;
    } else if (i < G + M) {
        const int64_t j = i - G;
        float st[6], x[8], y[8], z[8];
#pragma unroll
        for (int k = 0; k < 6; ++k) st[k] = pred_state[j * 7 + k];
        reinterpret_cast<float4 *>(pred_box)[j] = hg_footprint(st);
        state_corners(st, x, y, z);
        hg_project_to_im(x, y, z, P, nullptr, 0, reinterpret_cast<double2 *>(pred_im + j * 16));
    }
}

extern "C" int rn_mot_prepare(const double *gt_im, const float *gt_h0, const float *gt_vel, int64_t G,
                              const float *pred_state, int64_t M, const double *H, const double *P, float *gt_state,
                              float *gt_box, float *pred_box, double *pred_im, void *stream) {
    if (G < 0 || M < 0 || !H || !P) return RN_EINVAL;
    if (G + M == 0) return RN_OK;
    if ((G && (!gt_im || !gt_h0 || !gt_vel || !gt_state || !gt_box)) || (M && (!pred_state || !pred_box || !pred_im)))
        return RN_EINVAL;
    hipLaunchKernelGGL(mot_prepare_kernel, dim3(rn_blocks(G + M, 256)), dim3(256), 0, (hipStream_t)stream, gt_im, gt_h0, gt_vel,
                       G, pred_state, M, H, P, gt_state, gt_box, pred_box, pred_im);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- IoU
__global__ __launch_bounds__(256) void mot_iou_kernel(const float *__restrict__ gt_box, const float *__restrict__ pred_box,
                                                      const int32_t *__restrict__ gt_off, const int32_t *__restrict__ pr_off,
                                                      const int64_t *__restrict__ iou_off, double *__restrict__ iou) {
    const int f = blockIdx.x;
    const int ng = gt_off[f + 1] - gt_off[f], np = pr_off[f + 1] - pr_off[f];
    const int64_t k = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (k >= (int64_t)ng * np) return;
    const int i = (int)(k / np), j = (int)(k - (int64_t)i * np);
    const float4 a = reinterpret_cast<const float4 *>(gt_box)[gt_off[f] + i];
    const float4 b = reinterpret_cast<const float4 *>(pred_box)[pr_off[f] + j];
    const float area_a = (a.z - a.x) * (a.w - a.y);                           // mot_evaluator.py:106-107
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float minx = (b.x > a.x) ? b.x : a.x, maxx = (b.z < a.z) ? b.z : a.z;   // :109-112, Python's max / min
    const float miny = (b.y > a.y) ? b.y : a.y, maxy = (b.w < a.w) ? b.w : a.w;
    const float dx = maxx - minx, dy = maxy - miny;
    const float inter = (dx > 0.f ? dx : 0.f) * (dy > 0.f ? dy : 0.f);        // :114
    const float uni = ((area_a + area_b) - inter) + (float)1e-06;             // :115
    // :116.  `intersection / union`: union is a tensor; an intersection built from b's values alone (the prediction strictly
    // inside the ground truth on both axes) is a numpy scalar, and Tensor.__rtruediv__ is reciprocal() * numerator
    const bool inside = b.x > a.x && b.z < a.z && b.y > a.y && b.w < a.w;
    const float q = inside ? (1.0f / uni) * inter : inter / uni;
    iou[iou_off[f] + k] = (double)q;                                          // stored into the fp64 matrix (:222)
}

extern "C" int rn_mot_iou(const float *gt_box, const float *pred_box, const int32_t *gt_off, const int32_t *pr_off,
                          const int64_t *iou_off, int64_t F, int64_t max_cells, double *iou, void *stream) {
    if (F < 0 || max_cells < 0 || max_cells > (int64_t)RN_MOT_MAX * RN_MOT_MAX) return RN_EINVAL;
    if (F == 0 || max_cells == 0) return RN_OK;
    if (F > INT_MAX || !gt_box || !pred_box || !gt_off || !pr_off || !iou_off || !iou) return RN_EINVAL;
    hipLaunchKernelGGL(mot_iou_kernel, dim3((unsigned)F, rn_blocks(max_cells, 256)), dim3(256), 0, (hipStream_t)stream, gt_box,
                       pred_box, gt_off, pr_off, iou_off, iou);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- assignment
__global__ __launch_bounds__(64) void mot_assign_kernel(const double *__restrict__ iou, const int32_t *__restrict__ gt_off,
                                                        const int32_t *__restrict__ pr_off, const int64_t *__restrict__ iou_off,
                                                        const int32_t *__restrict__ slot_off, int32_t *__restrict__ slot_row,
                                                        int32_t *__restrict__ slot_col, uint8_t *__restrict__ pred_assigned,
                                                        int32_t *__restrict__ frame_status) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int ng = gt_off[f + 1] - gt_off[f], np = pr_off[f + 1] - pr_off[f];
    if (ng <= 0 || np <= 0) { if (lane == 0) frame_status[f] = 0; return; }
    if (ng > RN_MOT_MAX || np > RN_MOT_MAX) { if (lane == 0) frame_status[f] = 3; return; }
    const double *mat = iou + iou_off[f];
    int bad = 0;
    for (int k = lane; k < ng * np; k += 64) {
        const double c = mat[k];
        bad |= (c != c) || (c == INFINITY);                                  // -c: NaN or -inf, scipy's invalid entries
    }
    if (__ballot(bad) != 0ull) { if (lane == 0) frame_status[f] = 1; return; }
    const bool tr = ng > np;                                                 // scipy transposes tall problems
    const int nr = tr ? np : ng, nc = tr ? ng : np;
    const int64_t rs = tr ? 1 : np, cs = tr ? np : 1;
    LsapWs w;
    lsap_arrays_layout(lds, nr, nc, &w);
    if (lsap_solve_wave<true>(mat, rs, cs, nr, nc, w, lane) != 0) { if (lane == 0) frame_status[f] = 2; return; }
    int32_t *srow = slot_row + slot_off[f], *scol = slot_col + slot_off[f];
    uint8_t *pa = pred_assigned + pr_off[f];
    if (!tr) {                                                               // every ground-truth row is assigned
        for (int r = lane; r < ng; r += 64) {
            const int c = w.col4row[r];
            srow[r] = r;
            scol[r] = c;
            pa[c] = 1;
        }
    } else {                                                                 // ascending ground-truth row = solver column
        int base = 0;
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int c = c0 + lane;
            const int r = c < nc ? w.row4col[c] : -1;
            const unsigned long long m = __ballot(r >= 0);
            if (r >= 0) {
                const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
                srow[pos] = c;
                scol[pos] = r;
                pa[r] = 1;
            }
            base += __popcll(m);
        }
    }
    if (lane == 0) frame_status[f] = 0;
}

extern "C" int rn_mot_assign(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                             const int32_t *slot_off, int64_t F, int64_t max_n, int64_t S, int64_t M, int32_t *slot_row,
                             int32_t *slot_col, uint8_t *pred_assigned, int32_t *frame_status, void *stream) {
    if (F < 0 || S < 0 || M < 0 || max_n < 0 || max_n > RN_MOT_MAX) return RN_EINVAL;   // a larger frame: no launch
    if (F == 0) return RN_OK;
    if (F > INT_MAX || !gt_off || !pr_off || !iou_off || !slot_off || !frame_status || (S && (!iou || !slot_row || !slot_col)) ||
        (M && !pred_assigned))
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (S) e = hipMemsetAsync(slot_row, 0xFF, S * 4, s);
    if (e == hipSuccess && S) e = hipMemsetAsync(slot_col, 0xFF, S * 4, s);
    if (e == hipSuccess && M) e = hipMemsetAsync(pred_assigned, 0, M, s);
    if (e != hipSuccess) return (int)e;
    const int64_t n = max_n < 1 ? 1 : max_n;
    const size_t bytes = (size_t)lsap_arrays_layout(nullptr, n, n, nullptr);
    hipLaunchKernelGGL(mot_assign_kernel, dim3((unsigned)F), dim3(64), bytes, s, iou, gt_off, pr_off, iou_off, slot_off, slot_row,
                       slot_col, pred_assigned, frame_status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- per-frame metrics
template <typename T>
__device__ __forceinline__ T clamp500(T x) { return x < (T)0 ? (T)0 : (x > (T)500 ? (T)500 : x); }   // keeps NaN

// torch.clamp(torch.mean(torch.sqrt(torch.sum(torch.pow(p - g, 2), dim=1))), 0, 500) over 4 corners, fp64 (:307-308)
__device__ __forceinline__ double corner_err(const double *__restrict__ p, const double *__restrict__ g) {
    double e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double dx = p[2 * k] - g[2 * k], dy = p[2 * k + 1] - g[2 * k + 1];
        e[k] = sqrt(dx * dx + dy * dy);
    }
    return clamp500((((e[0] + e[1]) + e[2]) + e[3]) / 4.0);
}

__global__ __launch_bounds__(64) void mot_frame_kernel(
    const double *__restrict__ iou, const int32_t *__restrict__ gt_off, const int32_t *__restrict__ pr_off,
    const int64_t *__restrict__ iou_off, const int32_t *__restrict__ slot_off, const int32_t *__restrict__ slot_row,
    const int32_t *__restrict__ slot_col, const int32_t *__restrict__ frame_status, double match_iou,
    const float *__restrict__ gt_state, const float *__restrict__ pred_state, const double *__restrict__ gt_im,
    const double *__restrict__ pred_im, const int32_t *__restrict__ gt_cls, const int32_t *__restrict__ pred_cls,
    const int32_t *__restrict__ gt_id, const int32_t *__restrict__ pred_id, const uint8_t *__restrict__ pred_assigned,
    double *__restrict__ slot_iou, int32_t *__restrict__ slot_gid, int32_t *__restrict__ slot_pid,
    float *__restrict__ slot_state_err, double *__restrict__ slot_bot, double *__restrict__ slot_top,
    uint8_t *__restrict__ slot_cls, int32_t *__restrict__ frame_edge, int32_t *__restrict__ frame_match) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int g0 = gt_off[f], p0 = pr_off[f];
    const int ng = gt_off[f + 1] - g0, np = pr_off[f + 1] - p0;
    int edge = 0, nmatch = 0;
    if (ng > 0 && np > 0 && frame_status[f] == 0) {
        const double *mat = iou + iou_off[f];
        const int s0 = slot_off[f], ns = slot_off[f + 1] - s0;
        for (int i = lane; i < ns; i += 64) {
            const int r = slot_row[s0 + i], c = slot_col[s0 + i];
            if (r < 0 || r >= ng || c < 0 || c >= np) continue;              // never after status 0; keeps every index in range
            const double v = mat[(int64_t)r * np + c];
            const bool ok = v >= match_iou;                                  // :232
            const int64_t s = s0 + i;
            slot_iou[s] = v;
            slot_gid[s] = ok ? gt_id[g0 + r] : -1;
            slot_pid[s] = ok ? pred_id[p0 + c] : -1;
            float se[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            double bot = 0.0, top = 0.0;
            int cell = 0;
            if (ok) {
                const float *ps = pred_state + (int64_t)(p0 + c) * 7, *gs = gt_state + (int64_t)(g0 + r) * 7;
#pragma unroll
                for (int q = 0; q < 7; ++q) se[q] = clamp500(fabsf(ps[q] - gs[q]));              // :303
                const double *pi = pred_im + (int64_t)(p0 + c) * 16, *gi = gt_im + (int64_t)(g0 + r) * 16;
                bot = corner_err(pi, gi);
                top = corner_err(pi + 8, gi + 8);
                const int gc = gt_cls[g0 + r], pc = pred_cls[p0 + c];        // -1: not in class_dict
                cell = gc < 0 ? 55 : gc * 10 + (pc < 0 ? 5 : pc);            // :314-325, an unknown gt string is looked up twice
                ++nmatch;
            }
#pragma unroll
            for (int q = 0; q < 7; ++q) slot_state_err[s * 7 + q] = se[q];
            slot_bot[s] = bot;
            slot_top[s] = top;
            slot_cls[s] = (uint8_t)cell;
        }
        for (int j = lane; j < np; j += 64) {
            if (pred_assigned[p0 + j]) continue;                             // `i not in b` (:284)
            const double *o = pred_im + (int64_t)(p0 + j) * 16;
            const double x0 = o[0], y0 = o[1], x2 = o[4], y2 = o[5];
            edge += (x0 < 0 || x2 < 0 || x0 > 1920 || x2 > 1920 || y0 < 0 || y2 < 0 || y0 > 1080 || y2 > 1080);   // :286-290
        }
    }
    edge = wave_sum(edge);
    nmatch = wave_sum(nmatch);
    if (lane == 0) { frame_edge[f] = edge; frame_match[f] = nmatch; }
}

extern "C" int rn_mot_frame_metrics(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                                    const int32_t *slot_off, int64_t F, int64_t S, const int32_t *slot_row,
                                    const int32_t *slot_col, const int32_t *frame_status, double match_iou,
                                    const float *gt_state, const float *pred_state, const double *gt_im, const double *pred_im,
                                    const int32_t *gt_cls, const int32_t *pred_cls, const int32_t *gt_id, const int32_t *pred_id,
                                    const uint8_t *pred_assigned, double *slot_iou, int32_t *slot_gid, int32_t *slot_pid,
                                    float *slot_state_err, double *slot_bot, double *slot_top, uint8_t *slot_cls,
                                    int32_t *frame_edge, int32_t *frame_match, void *stream) {
    if (F < 0 || S < 0 || F > INT_MAX) return RN_EINVAL;
    if (F == 0) return RN_OK;
    if (!gt_off || !pr_off || !iou_off || !slot_off || !frame_status || !frame_edge || !frame_match) return RN_EINVAL;
    if (S && (!iou || !slot_row || !slot_col || !gt_state || !pred_state || !gt_im || !pred_im || !gt_cls || !pred_cls || !gt_id ||
              !pred_id || !pred_assigned || !slot_iou || !slot_gid || !slot_pid || !slot_state_err || !slot_bot || !slot_top ||
              !slot_cls))
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (S) {                                                                 // slots of a frame with a status stay "no pair"
        hipError_t e = hipMemsetAsync(slot_gid, 0xFF, S * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(slot_pid, 0xFF, S * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(slot_iou, 0, S * 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(slot_state_err, 0, S * 28, s);
        if (e == hipSuccess) e = hipMemsetAsync(slot_bot, 0, S * 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(slot_top, 0, S * 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(slot_cls, 0, S, s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(mot_frame_kernel, dim3((unsigned)F), dim3(64), 0, s, iou, gt_off, pr_off, iou_off, slot_off, slot_row,
                       slot_col, frame_status, match_iou, gt_state, pred_state, gt_im, pred_im, gt_cls, pred_cls, gt_id, pred_id,
                       pred_assigned, slot_iou, slot_gid, slot_pid, slot_state_err, slot_bot, slot_top, slot_cls, frame_edge,
                       frame_match);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- sequence reduction
struct MotWs {
    int32_t *last, *pidcnt;          // last matched prediction id per ground-truth id (-1: none yet); gt lists holding each pred id
    uint32_t *pairs;                 // bit (g * n_pid + p): prediction id p is in ground-truth id g's list
    uint8_t *gt_seen, *pred_seen;
};

__host__ __device__ static inline int64_t mot_ws_layout(char *base, int64_t n_gid, int64_t n_pid, MotWs *w) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *r = base ? base + o : nullptr; o += (bytes + 15) & ~(int64_t)15; return r; };
    MotWs t;
    t.last = reinterpret_cast<int32_t *>(take(n_gid * 4));                   // first: the entry fills it with 0xFF
    t.pidcnt = reinterpret_cast<int32_t *>(take(n_pid * 4));
    t.pairs = reinterpret_cast<uint32_t *>(take(((n_gid * n_pid + 31) / 32) * 4));
    t.gt_seen = reinterpret_cast<uint8_t *>(take(n_gid));
    t.pred_seen = reinterpret_cast<uint8_t *>(take(n_pid));
    if (w) *w = t;
    return o;
}

extern "C" int64_t rn_mot_workspace_bytes(int64_t n_gid, int64_t n_pid) {
    if (n_gid < 0 || n_pid < 0 || n_gid > RN_MOT_MAX_IDS || n_pid > RN_MOT_MAX_IDS) return 0;
    return 16 + mot_ws_layout(nullptr, n_gid, n_pid, nullptr);
}

// value q of slot k, or "skip": 0 every assigned pair's IoU; 1 the matches' IoU; 2..8 state_err columns; 9 / 10 bottom / top
__device__ __forceinline__ bool mot_value(int q, int64_t k, const double *__restrict__ slot_iou, const int32_t *__restrict__ slot_gid,
                                          const int32_t *__restrict__ slot_row, const float *__restrict__ se,
                                          const double *__restrict__ bot, const double *__restrict__ top, double &v) {
    if (q == 0) { v = slot_iou[k]; return slot_row[k] >= 0; }
    if (slot_gid[k] < 0) return false;
    v = q == 1 ? slot_iou[k] : (q <= 8 ? (double)se[k * 7 + (q - 2)] : (q == 9 ? bot[k] : top[k]));
    return true;
}

__global__ __launch_bounds__(MOT_BLOCK) void mot_reduce_kernel(
    int F, int64_t S, const int32_t *__restrict__ gt_off, const int32_t *__restrict__ pr_off,
    const int32_t *__restrict__ slot_off, const int32_t *__restrict__ frame_status, const int32_t *__restrict__ frame_edge,
    const int32_t *__restrict__ frame_match, const int32_t *__restrict__ slot_row, const double *__restrict__ slot_iou,
    const int32_t *__restrict__ slot_gid, const int32_t *__restrict__ slot_pid, const float *__restrict__ slot_state_err,
    const double *__restrict__ slot_bot, const double *__restrict__ slot_top, const uint8_t *__restrict__ slot_cls,
    const int32_t *__restrict__ gt_id, const int32_t *__restrict__ pred_id, int n_gid, int n_pid, char *__restrict__ ws,
    double *__restrict__ result) {
    __shared__ unsigned long long cnt[12];     // TP FP FN edge FP02 FN02 n_gt_ids n_pred_ids frag switches pairs matches
    __shared__ int conf[100];
    __shared__ int bad_frame;
    __shared__ double part[MOT_BLOCK];
    __shared__ double total;
    const int t = threadIdx.x;
    MotWs w;
    mot_ws_layout(ws, n_gid, n_pid, &w);
    if (t < 12) cnt[t] = 0ull;
    if (t < 100) conf[t] = 0;
    if (t == 0) bad_frame = INT_MAX;
    __syncthreads();
    for (int f = t; f < F; f += MOT_BLOCK)
        if (frame_status[f] != 0) atomicMin(&bad_frame, f);
    __syncthreads();
    if (bad_frame != INT_MAX) {                                              // the host raises; nothing else is reported
        if (t == 0) { result[11] = (double)frame_status[bad_frame]; result[12] = (double)bad_frame; }
        return;
    }
    // counters and the ids of frames that one side lacks (:132-152, 294-299)
    for (int f = t; f < F; f += MOT_BLOCK) {
        const int ng = gt_off[f + 1] - gt_off[f], np = pr_off[f + 1] - pr_off[f];
        if (ng == 0) {
            atomicAdd(&cnt[1], (unsigned long long)np);
            for (int j = pr_off[f]; j < pr_off[f + 1]; ++j) {
                const int p = pred_id[j];
                if (p >= 0 && p < n_pid) w.pred_seen[p] = 1;                 // an id outside the dense range is not counted
            }
        } else if (np == 0) {
            atomicAdd(&cnt[2], (unsigned long long)ng);
            for (int i = gt_off[f]; i < gt_off[f + 1]; ++i) {
                const int g = gt_id[i];
                if (g >= 0 && g < n_gid) w.gt_seen[g] = 1;
            }
        } else {
            const int k = ng < np ? ng : np, m = frame_match[f];
            atomicAdd(&cnt[0], (unsigned long long)m);
            atomicAdd(&cnt[1], (unsigned long long)(np - m));
            atomicAdd(&cnt[2], (unsigned long long)(ng - m));
            atomicAdd(&cnt[3], (unsigned long long)frame_edge[f]);
            atomicAdd(&cnt[4], (unsigned long long)(np - k));
            atomicAdd(&cnt[5], (unsigned long long)(ng - k));
            atomicAdd(&cnt[10], (unsigned long long)k);
        }
    }
    // matches: unique ids, the (gt, pred) pair table, the confusion matrix -- sets and integer counts, order-free
    for (int64_t k = t; k < S; k += MOT_BLOCK) {
        const int g = slot_gid[k], p = slot_pid[k];
        if (g < 0 || g >= n_gid || p < 0 || p >= n_pid) continue;
        w.gt_seen[g] = 1;
        w.pred_seen[p] = 1;
        const int64_t bit = (int64_t)g * n_pid + p;
        const uint32_t mask = 1u << (bit & 31);
        if (!(atomicOr(&w.pairs[bit >> 5], mask) & mask)) atomicAdd(&w.pidcnt[p], 1);
        const int c = slot_cls[k];
        if (c < 100) atomicAdd(&conf[c], 1);
        atomicAdd(&cnt[11], 1ull);
    }
    __syncthreads();
    {
        unsigned long long a = 0, b = 0, c = 0;
        for (int i = t; i < n_gid; i += MOT_BLOCK) a += w.gt_seen[i];
        for (int i = t; i < n_pid; i += MOT_BLOCK) { b += w.pred_seen[i]; const int n = w.pidcnt[i]; c += n > 1 ? n - 1 : 0; }
        atomicAdd(&cnt[6], a);
        atomicAdd(&cnt[7], b);
        atomicAdd(&cnt[9], c);                                               // :367-376
    }
    // fragmentations: every thread walks the matches in sequence order and keeps the ground-truth ids it owns (:332-336, 364)
    {
        unsigned long long fr = 0;
        for (int64_t k = 0; k < S; ++k) {
            const int g = slot_gid[k];
            if (g < 0 || g >= n_gid || (g % MOT_BLOCK) != t) continue;
            const int p = slot_pid[k], l = w.last[g];
            fr += (l != -1 && l != p);
            w.last[g] = p;
        }
        atomicAdd(&cnt[8], fr);
    }
    __syncthreads();
    if (t < 12 && t != 11) result[t] = (double)cnt[t];
    if (t < 100) result[52 + t] = (double)conf[t];
    // (count, sum, sum of squared deviations) of every figure, fp64, fixed order
    for (int q = 0; q < 11; ++q) {
        const double n = (double)(q == 0 ? cnt[10] : cnt[11]);
        double mean = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
            double acc = 0.0;
            for (int64_t k = t; k < S; k += MOT_BLOCK) {
                double v;
                if (!mot_value(q, k, slot_iou, slot_gid, slot_row, slot_state_err, slot_bot, slot_top, v)) continue;
                if (pass) { const double d = v - mean; acc = acc + d * d; }
                else acc = acc + v;
            }
            part[t] = acc;
            __syncthreads();
            if (t == 0) {
                double s = 0.0;
                for (int i = 0; i < MOT_BLOCK; ++i) s = s + part[i];
                total = s;
            }
            __syncthreads();
            if (pass == 0) mean = total / n;
            if (t == 0) result[16 + 3 * q + 1 + pass] = total;
            __syncthreads();
        }
        if (t == 0) result[16 + 3 * q] = n;
    }
}

extern "C" int rn_mot_reduce(int64_t F, int64_t S, const int32_t *gt_off, const int32_t *pr_off, const int32_t *slot_off,
                             const int32_t *frame_status, const int32_t *frame_edge, const int32_t *frame_match,
                             const int32_t *slot_row, const double *slot_iou, const int32_t *slot_gid, const int32_t *slot_pid,
                             const float *slot_state_err, const double *slot_bot, const double *slot_top, const uint8_t *slot_cls,
                             const int32_t *gt_id, const int32_t *pred_id, int64_t n_gid, int64_t n_pid, void *workspace,
                             double *result, void *stream) {
    if (F < 0 || F > INT_MAX || S < 0 || n_gid < 0 || n_pid < 0 || n_gid > RN_MOT_MAX_IDS || n_pid > RN_MOT_MAX_IDS || !workspace ||
        !result)
        return RN_EINVAL;
    if (F && (!gt_off || !pr_off || !slot_off || !frame_status || !frame_edge || !frame_match)) return RN_EINVAL;
    if (S && (!slot_row || !slot_iou || !slot_gid || !slot_pid || !slot_state_err || !slot_bot || !slot_top || !slot_cls))
        return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace) + 16;
    const int64_t bytes = mot_ws_layout(nullptr, n_gid, n_pid, nullptr);
    const int64_t last_bytes = (n_gid * 4 + 15) & ~(int64_t)15;
    hipError_t e = hipMemsetAsync(result, 0, RN_MOT_RESULT * 8, s);
    if (e == hipSuccess && bytes) e = hipMemsetAsync(ws, 0, bytes, s);
    if (e == hipSuccess && last_bytes) e = hipMemsetAsync(ws, 0xFF, last_bytes, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mot_reduce_kernel, dim3(1), dim3(MOT_BLOCK), 0, s, (int)F, S, gt_off, pr_off, slot_off, frame_status,
                       frame_edge, frame_match, slot_row, slot_iou, slot_gid, slot_pid, slot_state_err, slot_bot, slot_top, slot_cls,
                       gt_id, pred_id, (int)n_gid, (int)n_pid, ws, result);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

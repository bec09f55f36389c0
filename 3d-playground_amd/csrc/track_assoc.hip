// Detection -> track association of the multi-camera tracker, device-resident.
//
// Replaces the middle of MC_Crop_Tracker.match_hungarian (MC3D_crop_tracker.py:637-731): the fp64 `1 - md_iou` cost of
// the road-plane footprints of the priors against the detections, scipy.optimize.linear_sum_assignment on it, and the
// phi_match gate.  The reference copies both state arrays to the host for this on every detection frame.
//   rn_track_cost          one lane per (prior, detection) pair: hg_footprint of both states (fp32, as the reference's
//                          boxes_new), IoU in md_iou's operation order in fp64 (:1030-1049), 1 - iou
//   rn_linear_sum_assignment
//     lsap_check_kernel    NaN / -inf anywhere -> invalid (scipy raises ValueError before solving)
//     lsap_solve_kernel    one wave64 per problem: scipy's rectangular_lsap restated (Crouse 2016, shortest augmenting
//                          path), then the gate `cost > max_cost` drops pairs (:719-723), fused in the same launch
// Exact restatement: every fp64 expression keeps scipy's evaluation order (-ffp-contract=off), the columns are scanned in
// the order of scipy's `remaining` list (swap-with-last removal), and the next column is chosen by scipy's tie rule --
// the lowest reduced cost, among equal costs the LAST unassigned column in scan order if there is one, else the first.
// The scan is split over the lanes by position and merged by a cross-lane reduction of (cost, unassigned, position),
// which reproduces that rule because it only depends on the positions, not on the order they are visited in.
// Every loop is bounded: an augmenting path visits at most nc columns and is at most nr rows long; past either bound
// the kernel writes a status and returns.
#include "common.h"
#include "homography_dev.h"
#include "lsap_dev.h"

// ---------------------------------------------------------------------------------------------- cost matrix
__global__ __launch_bounds__(256) void track_cost_kernel(const float *__restrict__ pre, int64_t pre_stride,
                                                         const float *__restrict__ det, int64_t det_stride, int64_t n,
                                                         int64_t m, double *__restrict__ cost) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n * m) return;
    const int64_t i = k / m, j = k - i * m;
    float sa[6], sb[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { sa[q] = pre[i * pre_stride + q]; sb[q] = det[j * det_stride + q]; }
    const float4 fa = hg_footprint(sa), fb = hg_footprint(sb);               // boxes_new (fp32), then .double()
    const double a0 = fa.x, a1 = fa.y, a2 = fa.z, a3 = fa.w;
    const double b0 = fb.x, b1 = fb.y, b2 = fb.z, b3 = fb.w;
    const double area_a = (a2 - a0) * (a3 - a1);                              // MC3D_crop_tracker.py:1035-1036
    const double area_b = (b2 - b0) * (b3 - b1);
    const double minx = fmax(a0, b0), maxx = fmin(a2, b2);                   // :1038-1041
    const double miny = fmax(a1, b1), maxy = fmin(a3, b3);
    const double inter = fmax(0.0, maxx - minx) * fmax(0.0, maxy - miny);     // :1044
    const double iou = inter / ((area_a + area_b) - inter);                   // :1045-1046, 0/0 stays NaN
    cost[k] = 1.0 - iou;                                                      // dist = 1.0 - md_iou(...) (:701)
}

extern "C" int rn_track_cost(const float *pre, int64_t pre_stride, const float *det, int64_t det_stride, int64_t n,
                             int64_t m, double *cost, void *stream) {
    if (n <= 0 || m <= 0 || pre_stride < 6 || det_stride < 6 || !pre || !det || !cost) return RN_EINVAL;
    hipLaunchKernelGGL(track_cost_kernel, dim3(rn_blocks(n * m, 256)), dim3(256), 0, (hipStream_t)stream, pre, pre_stride,
                       det, det_stride, n, m, cost);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- assignment
// Problem after the transpose: nr <= nc.  Column arrays sized nc, row arrays sized nr (LsapWs, lsap_dev.h).  The workspace
// is a 16-byte flag word (1 = a NaN or -inf entry, written by lsap_check_kernel), then the arrays.

static const int64_t LSAP_LDS_MAX = 64 * 1024;     // the arrays move to LDS when they fit in this much

extern "C" int64_t rn_lsap_workspace_bytes(int64_t nr, int64_t nc) {
    if (nr <= 0 || nc <= 0) return 0;
    const int64_t a = nr < nc ? nr : nc, b = nr < nc ? nc : nr;
    return 16 + lsap_arrays_layout(nullptr, a, b, nullptr);
}

__global__ __launch_bounds__(256) void lsap_check_kernel(const double *__restrict__ cost, int64_t total,
                                                          int32_t *__restrict__ flag) {
    int bad = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
        const double c = cost[k];
        bad |= (c != c) || (c == -INFINITY);                                  // scipy: RECTANGULAR_LSAP_INVALID
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) flag[0] = 1;         // every writer writes the same value
}


__global__ __launch_bounds__(64) void lsap_solve_kernel(const double *__restrict__ cost, int64_t nr_orig, int64_t nc_orig,
                                                        double max_cost, char *__restrict__ ws_arrays,
                                                        const int32_t *__restrict__ flag, int use_lds,
                                                        int32_t *__restrict__ row_match, int32_t *__restrict__ n_matched,
                                                        int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x;
    const bool tr = nr_orig > nc_orig;                                       // scipy transposes tall problems
    const int nr = (int)(tr ? nc_orig : nr_orig), nc = (int)(tr ? nr_orig : nc_orig);
    const int64_t rs = tr ? 1 : nc_orig, cs = tr ? nc_orig : 1;              // C(i,j) = cost[i*rs + j*cs], no copy
    for (int64_t r = lane; r < nr_orig; r += 64) row_match[r] = -1;
    if (flag[0] != 0) {                                                      // invalid: no matches
        if (lane == 0) { n_matched[0] = 0; status[0] = 1; }
        return;
    }
    LsapWs w;
    lsap_arrays_layout(use_lds ? lds : ws_arrays, nr, nc, &w);
    if (lsap_solve_wave<false>(cost, rs, cs, nr, nc, w, lane) != 0) {
        for (int64_t r = lane; r < nr_orig; r += 64) row_match[r] = -1;
        if (lane == 0) { n_matched[0] = 0; status[0] = 2; }
        return;
    }

    // outputs in the caller's orientation, with the gate (dist[i, matchings[i]] > 1 - phi_match -> -1)
    int cnt = 0;
    if (!tr) {
        for (int r = lane; r < nr; r += 64) {
            const int c = w.col4row[r];
            const bool keep = c >= 0 && !(cost[(int64_t)r * nc_orig + c] > max_cost);
            row_match[r] = keep ? c : -1;
            cnt += keep;
        }
    } else {                                                                 // original rows are the columns here
        for (int c = lane; c < nc; c += 64) {
            const int r = w.row4col[c];                                      // original column matched to original row c
            const bool keep = r >= 0 && !(cost[(int64_t)c * nc_orig + r] > max_cost);
            row_match[c] = keep ? r : -1;
            cnt += keep;
        }
    }
    cnt = wave_sum(cnt);
    if (lane == 0) { n_matched[0] = cnt; status[0] = 0; }
}

extern "C" int rn_linear_sum_assignment(const double *cost, int64_t nr, int64_t nc, double max_cost, void *workspace,
                                        int32_t *row_match, int32_t *n_matched, int32_t *status, void *stream) {
    if (nr <= 0 || nc <= 0 || !cost || !workspace || !row_match || !n_matched || !status) return RN_EINVAL;
    const int64_t a = nr < nc ? nr : nc, b = nr < nc ? nc : nr;
    if (a > RN_LSAP_MAX_MIN || b > RN_PARSE_MAX) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int32_t *flag = reinterpret_cast<int32_t *>(workspace);
    char *arrays = reinterpret_cast<char *>(workspace) + 16;
    const int64_t bytes = lsap_arrays_layout(nullptr, a, b, nullptr);
    const int use_lds = bytes <= LSAP_LDS_MAX;
    hipError_t e = hipMemsetAsync(flag, 0, 4, s);
    if (e != hipSuccess) return (int)e;
    const int64_t total = nr * nc;
    int blocks = rn_blocks(total, 256 * 8);
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(lsap_check_kernel, dim3(blocks), dim3(256), 0, s, cost, total, flag);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(lsap_solve_kernel, dim3(1), dim3(64), use_lds ? (size_t)bytes : 0, s, cost, nr, nc, max_cost, arrays,
                       flag, use_lds, row_match, n_matched, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// Per-camera time stamp bias of the multi-camera tracker, device-resident.
//
// Replaces MC_Crop_Tracker.estimate_ts_bias (MC3D_crop_tracker.py:237-315): the mean speed per travel direction of the
// tracked objects, the d x d fp64 IoU of the road-plane footprints of a frame's detections, the list of cross-camera
// pairs above phi_nms_space, and the serial exponential update of ts_bias over that list.  The reference walks the IoU
// matrix in a double Python loop with one .item() per pair; here the frame stays on the device.
//   ts_prepare_kernel   one lane per detection: hg_footprint (fp32, as the reference's boxes_new); wave 0 of block 0
//                       also forms the two mean speeds (:258-265) with the mu_v fallback for an empty direction
//   ts_pairs_kernel     one wave per row i, the lanes run over j = i+1 .. d-1 in chunks of 64: different cameras and
//                       iou[i,j] > phi (:286-287), IoU in md_iou's operation order in fp64 (:1030-1049, the same
//                       statements as track_cost_kernel).  FILL = false counts the row by ballot + popcount; FILL = true
//                       runs the same test again and writes the row's pairs behind its offset, a lane's slot being the
//                       number of set ballot bits below it -- so inside a row the order is j ascending, and the rows are
//                       laid end to end: the order of the reference's x_offsets list (:284-289)
//   ts_scan_kernel      one workgroup: exclusive scan of the row counts, the total, the range check of the camera
//                       indices, the status word
//   ts_update_kernel    one wave: the lanes fetch 64 pair records at a time, lane 0 applies the two entries of every
//                       pair in list order (:311-315) to ts_bias held in LDS, then the wave writes ts_bias back
// Precision, as torch's promotion rules give it in the reference: dx, vel, dt_expected, time_error are
// fp32 (dt_expected is a Python double difference rounded to fp32 by torch.tensor), the division is the correctly
// rounded one; the update is float((1-alpha)*bias[cam1]) + float(alpha) * (-te + float(bias[cam2])) with every
// operation rounded to fp32 and the result stored as a double.  Compiled with -ffp-contract=off.
// The two means are accumulated in fp64 and rounded once: for one or two objects per direction that equals torch's
// fp32 mean bit for bit, for more it is within half an ulp of the exact mean (torch's own summation order is not pinned).
#include <math.h>

#include "common.h"
#include "homography_dev.h"
#include "wave_dev.h"

struct TsPair { int32_t cam_i, cam_j; float te_ij, te_ji; };      // one 16-byte record per pair: its two entries

struct TsWs {
    float4 *fp;             // [d] footprints
    int32_t *row_count;     // [d]
    int32_t *row_off;       // [d]
    float *vel;             // [4]: EB_vel, WB_vel
    TsPair *rec;            // [max_pairs]
};

__host__ __device__ static inline int64_t ts_ws_layout(char *base, int64_t d, int64_t max_pairs, TsWs *w) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *r = base ? base + o : nullptr; o += (bytes + 15) & ~(int64_t)15; return r; };
    TsWs t;
    t.fp = reinterpret_cast<float4 *>(take(d * 16));
    t.row_count = reinterpret_cast<int32_t *>(take(d * 4));
    t.row_off = reinterpret_cast<int32_t *>(take(d * 4));
    t.vel = reinterpret_cast<float *>(take(16));
    t.rec = reinterpret_cast<TsPair *>(take(max_pairs * 16));
    if (w) *w = t;
    return o;
}

extern "C" int64_t rn_ts_bias_workspace_bytes(int64_t d, int64_t max_pairs) {
    if (d <= 0 || max_pairs < 0) return 0;
    return ts_ws_layout(nullptr, d, max_pairs, nullptr);
}

// rows valid: the device count when one is given, clamped to the launch size
__device__ __forceinline__ int ts_rows(const int32_t *d_count, int d) {
    if (!d_count) return d;
    const int c = d_count[0];
    return c < 0 ? 0 : (c > d ? d : c);
}

__global__ __launch_bounds__(256) void ts_prepare_kernel(const float *__restrict__ boxes, int64_t box_stride, int d,
                                                         const int32_t *__restrict__ d_count,
                                                         const float *__restrict__ objs, int64_t obj_stride, int n,
                                                         float mu_v, float4 *__restrict__ fp, float *__restrict__ vel) {
    const int dd = ts_rows(d_count, d);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < dd) {
        float s[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) s[q] = boxes[(int64_t)i * box_stride + q];
        fp[i] = hg_footprint(s);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {                                  // MC3D_crop_tracker.py:258-265
        double se = 0.0, sw = 0.0;
        int ne = 0, nw = 0;
        for (int r = threadIdx.x; r < n; r += 64) {
            const float dir = objs[(int64_t)r * obj_stride + 5], v = objs[(int64_t)r * obj_stride + 6];
            if (dir == 1.0f) { se += (double)v; ++ne; }
            if (dir == -1.0f) { sw += (double)v; ++nw; }
        }
        se = wave_sum(se); sw = wave_sum(sw);
        ne = wave_sum(ne); nw = wave_sum(nw);
        if (threadIdx.x == 0) {
            float eb = ne > 0 ? (float)(se / (double)ne) : NAN;                 // torch.mean of an empty set is NaN
            float wb = nw > 0 ? (float)(sw / (double)nw) * -1.0f : NAN;
            if (eb != eb) eb = mu_v;                                            // :264-265
            if (wb != wb) wb = -mu_v;                                           // :262-263
            vel[0] = eb;
            vel[1] = wb;
        }
    }
}

// one wave per row; 4 rows per block
template <bool FILL>
__global__ __launch_bounds__(256) void ts_pairs_kernel(const float *__restrict__ boxes, int64_t box_stride,
                                                       const int64_t *__restrict__ cams, int d,
                                                       const int32_t *__restrict__ d_count, int n_cam, double phi,
                                                       const double *__restrict__ timestamps, TsWs w,
                                                       const int32_t *__restrict__ info, int max_pairs,
                                                       int32_t *__restrict__ pairs_out, float *__restrict__ te_out) {
    const int dd = ts_rows(d_count, d);
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);                          // wave-uniform
    if (i >= dd) return;
    if (FILL && info[1] != 0) return;                                           // overflow / bad camera: nothing is written
    const float4 fa = w.fp[i];
    const int64_t cam_i = cams[i];
    const double a0 = fa.x, a1 = fa.y, a2 = fa.z, a3 = fa.w;
    const double area_a = (a2 - a0) * (a3 - a1);                                // MC3D_crop_tracker.py:1035
    int base = FILL ? w.row_off[i] : 0;
    float x_i = 0.f, vel = 0.f;
    double t_i = 0.0;
    if (FILL) {
        x_i = boxes[(int64_t)i * box_stride];
        const float dir_i = boxes[(int64_t)i * box_stride + 5];
        vel = dir_i == -1.0f ? w.vel[1] : w.vel[0];                             // :296-299, the direction of detection i
        t_i = timestamps[cam_i];                                                // cam_i is in range: info[1] == 0
    }
    for (int c = 0; c < RN_PARSE_MAX / 64; ++c) {
        const int j0 = i + 1 + c * 64;
        if (j0 >= dd) break;
        const int j = j0 + lane;
        bool hit = false;
        int64_t cam_j = 0;
        if (j < dd) {
            cam_j = cams[j];
            const float4 fb = w.fp[j];
            const double b0 = fb.x, b1 = fb.y, b2 = fb.z, b3 = fb.w;
            const double area_b = (b2 - b0) * (b3 - b1);                        // :1036
            const double minx = fmax(a0, b0), maxx = fmin(a2, b2);              // :1038-1041
            const double miny = fmax(a1, b1), maxy = fmin(a3, b3);
            const double inter = fmax(0.0, maxx - minx) * fmax(0.0, maxy - miny);   // :1044
            const double iou = inter / ((area_a + area_b) - inter);             // :1045-1046
            hit = cam_i != cam_j && iou > phi;                                  // :286-287 (NaN compares false)
        }
        const unsigned long long m = __ballot(hit);
        if (FILL) {
            if (hit) {
                const int k = base + __popcll(m & ((1ull << lane) - 1ull));
                if (k < max_pairs) {                                            // holds when info[1] == 0
                    const float x_j = boxes[(int64_t)j * box_stride];
                    const double t_j = timestamps[cam_j];
                    const float dx_ij = x_j - x_i, dx_ji = x_i - x_j;           // :288-289
                    const float dt_ij = (float)(t_j - t_i), dt_ji = (float)(t_i - t_j);     // :293
                    TsPair r;
                    r.cam_i = (int32_t)cam_i;
                    r.cam_j = (int32_t)cam_j;
                    r.te_ij = __fdiv_rn(dx_ij, vel) - dt_ij;                    // :302-303
                    r.te_ji = __fdiv_rn(dx_ji, vel) - dt_ji;
                    w.rec[k] = r;
                    if (pairs_out) { pairs_out[2 * k] = i; pairs_out[2 * k + 1] = j; }
                    if (te_out) { te_out[2 * k] = r.te_ij; te_out[2 * k + 1] = r.te_ji; }
                }
            }
        }
        base += __popcll(m);
    }
    if (!FILL && lane == 0) w.row_count[i] = base;
}

// one workgroup of 1024: thread t owns rows [16 t, 16 t + 16)
__global__ __launch_bounds__(1024) void ts_scan_kernel(const int64_t *__restrict__ cams, int d,
                                                       const int32_t *__restrict__ d_count, int n_cam, int max_pairs,
                                                       TsWs w, int32_t *__restrict__ info) {
    __shared__ int wave_tot[16];
    const int dd = ts_rows(d_count, d);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int cnt[RN_PARSE_MAX / 1024];
    int sum = 0, bad = 0;
#pragma unroll
    for (int q = 0; q < RN_PARSE_MAX / 1024; ++q) {
        const int r = t * (RN_PARSE_MAX / 1024) + q;
        cnt[q] = r < dd ? w.row_count[r] : 0;
        sum += cnt[q];
        if (r < dd) { const int64_t c = cams[r]; bad |= (c < 0 || c >= n_cam); }
    }
    const int incl = wave_scan_incl(sum);
    if (lane == 63) wave_tot[wv] = incl;
    bad = __syncthreads_or(bad);
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int v = wave_tot[k]; before += k < wv ? v : 0; total += v; }
    int run = before + incl - sum;
#pragma unroll
    for (int q = 0; q < RN_PARSE_MAX / 1024; ++q) {
        const int r = t * (RN_PARSE_MAX / 1024) + q;
        if (r < dd) w.row_off[r] = run;
        run += cnt[q];
    }
    if (t == 0) {
        info[0] = total;
        info[1] = bad ? 2 : (total > max_pairs ? 1 : 0);
    }
}

__global__ __launch_bounds__(64) void ts_update_kernel(TsWs w, const int32_t *__restrict__ info, int max_pairs,
                                                       int n_cam, double alpha, double *__restrict__ ts_bias) {
    __shared__ double bias[RN_TS_MAX_CAMS];
    if (info[1] != 0) return;                                                   // ts_bias stays untouched
    const int lane = threadIdx.x;
    int np = info[0];
    np = np > max_pairs ? max_pairs : np;
    if (np <= 0) return;
    for (int c = lane; c < n_cam; c += 64) bias[c] = ts_bias[c];
    __syncthreads();
    const double keep = 1.0 - alpha;                                            // Python: (1 - self.ts_alpha), a double
    const float alpha_f = (float)alpha;                                         // alpha * tensor: the scalar joins as fp32
    for (int k0 = 0; k0 < np; k0 += 64) {
        TsPair mine = {0, 0, 0.f, 0.f};
        if (k0 + lane < np) mine = w.rec[k0 + lane];
        const int nk = np - k0 < 64 ? np - k0 : 64;
        for (int t = 0; t < nk; ++t) {
            const int ci = __shfl(mine.cam_i, t, 64), cj = __shfl(mine.cam_j, t, 64);
            const float te1 = __shfl(mine.te_ij, t, 64), te2 = __shfl(mine.te_ji, t, 64);
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {                                   // (cam_i, cam_j, te_ij), then (cam_j, cam_i, te_ji)
                    const int cam1 = e ? cj : ci, cam2 = e ? ci : cj;
                    const float te = e ? te2 : te1;
                    if (cam1 != 0) {                                            // camera 0 is the time origin (:314)
                        const float a = (float)(keep * bias[cam1]);
                        const float s = -te + (float)bias[cam2];
                        const float m = alpha_f * s;
                        bias[cam1] = (double)(a + m);                           // float(...) (:315)
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int c = lane; c < n_cam; c += 64) ts_bias[c] = bias[c];
}

extern "C" int rn_estimate_ts_bias(const float *boxes, int64_t box_stride, const int64_t *camera_idxs, int64_t d,
                                   const int32_t *d_count, const float *objs, int64_t obj_stride, int64_t n,
                                   const double *timestamps, double *ts_bias, int n_cam, double phi, double alpha,
                                   float mu_v, void *workspace, int64_t max_pairs, int32_t *pairs_out, float *te_out,
                                   int32_t *info, void *stream) {
    if (d < 0 || n < 0 || !info) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (d == 0 || n == 0) {                                                     // the reference returns at once (:251-257)
        hipError_t e = hipMemsetAsync(info, 0, 8, s);
        return e != hipSuccess ? (int)e : RN_OK;
    }
    if (d > RN_PARSE_MAX || n_cam <= 0 || n_cam > RN_TS_MAX_CAMS || box_stride < 6 || obj_stride < 7 || max_pairs <= 0 ||
        max_pairs > (int64_t)RN_PARSE_MAX * (RN_PARSE_MAX - 1) / 2 || !boxes || !camera_idxs || !objs || !timestamps ||
        !ts_bias || !workspace)
        return RN_EINVAL;
    TsWs w;
    ts_ws_layout(reinterpret_cast<char *>(workspace), d, max_pairs, &w);
    const int di = (int)d, mp = (int)max_pairs;
    hipLaunchKernelGGL(ts_prepare_kernel, dim3(rn_blocks(d, 256)), dim3(256), 0, s, boxes, box_stride, di, d_count, objs,
                       obj_stride, (int)n, mu_v, w.fp, w.vel);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_pairs_kernel<false>, dim3(rn_blocks(d, 4)), dim3(256), 0, s, boxes, box_stride, camera_idxs, di,
                       d_count, n_cam, phi, timestamps, w, (const int32_t *)info, mp, (int32_t *)nullptr, (float *)nullptr);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_scan_kernel, dim3(1), dim3(1024), 0, s, camera_idxs, di, d_count, n_cam, mp, w, info);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_pairs_kernel<true>, dim3(rn_blocks(d, 4)), dim3(256), 0, s, boxes, box_stride, camera_idxs, di,
                       d_count, n_cam, phi, timestamps, w, (const int32_t *)info, mp, pairs_out, te_out);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_update_kernel, dim3(1), dim3(64), 0, s, w, (const int32_t *)info, mp, n_cam, alpha, ts_bias);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// Identity and association scores of tracking output, device-resident: IDF1 / IDP / IDR (Ristani et al., ECCV-W 2016) and the
// HOTA family (Luiten et al., IJCV 2021).  The reference's MOT_Evaluator stops at the CLEAR-MOT figures (mot_eval.hip); these go
// beyond it and are pinned to the published definitions, restated in tests/mot_assoc_cases.py.  Input is what mot_eval.hip already
// leaves on the device: the frames packed with per-frame offsets (gt_off / pr_off / iou_off / slot_off), every scored frame's fp64
// IoU matrix S_t [n_gt x n_pred] (rn_mot_iou) and dense id indices g < G, p < P.
//
// Definitions.  gc[g] / pc[p]: frames in which the id appears (scored or one-sided frames alike).  eps = 2^-52.
//   identity   C[g,p]  = number of frames with S_t[g,p] >= id_iou (every pair above the threshold, no per-frame assignment)
//              IDTP    = max over one-to-one partial matchings of ids of sum C[g,p]: the rectangular problem on C itself, maximised
//                        (the padded (G+P)^2 form of the published evaluators has the same optimum)
//              IDFN = sum gc - IDTP, IDFP = sum pc - IDTP; IDR / IDP / IDF1 are formed on the host
//   HOTA       per scored frame  den = (colsum(S)[p] + rowsum(S)[g]) - S[g,p];  J = S / den where den > eps, else 0;  pot[g,p] += J
//              ga[g,p] = pot / ((gc[g] + pc[p]) - pot)
//              per scored frame ONE assignment maximising ga[g,p] * S_t[g,p] (scipy's solver on the negated matrix)
//              for alpha_k (k = 0..18, ascending, passed by the host): a matched pair counts when S >= alpha_k - eps;
//              TP_k += m, FN_k += n_gt - m, FP_k += n_pred - m, Loc_k += S of the counted pairs, M_k[g,p] += 1;
//              a one-sided frame adds its count to FP_k or FN_k for every k
//              AssA-sum_k = sum M (M / max(1, gc + pc - M)), AssRe-sum_k with max(1, gc), AssPr-sum_k with max(1, pc)
//              the ratios, HOTA_k = sqrt(DetA_k AssA_k), LocA_k and the means over k are formed on the host from the per-alpha block
// Stages (one C entry point each):
//   rn_mot_id_counts    one workgroup per frame: gc, pc, C with integer atomics (exact); a thread per object scans its frame for
//                       the same id (RN_MOT_DUPLICATE_ID: the accumulators below rely on ids being unique in a frame)
//   rn_mot_id_assign    ONE wave64: C widened to fp64 in the workspace, lsap_solve_wave<true> (transposed through the strides when
//                       G > P) with its vectors in global memory -> the matching and IDTP
//   rn_mot_hota_align   pre-pass, one workgroup per frame: rowsum[i] = S[i,0] + S[i,1] + ... and colsum[j] = S[0,j] + S[1,j] + ...,
//                       each ONE thread's sequential ascending sum.  Then NO fp64 atomics: row g of pot belongs to workgroup g,
//                       which walks g's appearances in ascending frame order (a CSR of (frame, row) per id from the host); threads
//                       cover the frame's predictions; ids are unique in a frame, so every cell gets one add per frame, in frame order
//   rn_mot_hota_assign  one wave64 per frame: ga * S into the frame's cells of a score buffer, the solver in LDS, per matched pair
//                       (row, col, S, number of alphas passed) in the frame's slots (slot_off, ascending ground-truth row).  alpha
//                       ascends, so "S >= alpha_k - eps" holds for a prefix of k: the prefix length is stored, not 19 flags
//   rn_mot_hota_reduce  three launches: (a) per frame, histogram over (prefix length, g, p) and over the prefix length, integer
//                       atomics; (b) per cell, suffix sum over the prefix length -> M_k; (c) one workgroup per alpha: TP / FN / FP
//                       exact integers, Loc_k over the slots and the three association sums over the G x P cells, each fp64 in ONE
//                       fixed order (entry e -> partial e % 256 in ascending e, the partials added in increasing order)
// Bounds: a frame holds at most RN_MOT_MAX objects per side; G * P <= RN_MOT_ASSOC_MAX_CELLS (dense C, pot and 19 layers of M:
// 100 bytes per cell with the fp64 copy of C).  Above either the entry returns RN_EINVAL before any launch.  Every index read from
// memory (offset, id, row, column, slot, CSR entry) is checked before use; a bad one is left out and flagged RN_MOT_BAD_INDEX.  No
// kernel waits on another workgroup or spins on memory; every loop is bounded.  A NaN or +inf score gives RN_MOT_INVALID, no finite
// assignment RN_MOT_INFEASIBLE, as rn_mot_assign.  -ffp-contract=off.
#include "common.h"
#include "lsap_dev.h"
#include "wave_dev.h"

#define MA_BLOCK 256
#define MA_EPS 2.220446049250313e-16                                        // 2^-52, np.finfo(float).eps

// The packed frames.  Offsets come from memory: assoc_frame checks them against the totals before anything is indexed with them.
struct AssocLay {
    const int32_t *gt_off, *pr_off;
    const int64_t *iou_off;
    const int32_t *slot_off;
    int64_t n_gt, n_pr, cells, S;
    int F, max_n;                    // max_n: the largest frame the launch was sized for (LDS of the per-frame solver)
};
struct AssocFrame {
    int g0, p0, ng, np, s0;
    int64_t c0;
};

__device__ __forceinline__ bool assoc_frame(const AssocLay &L, int f, AssocFrame &fr) {
    if (f < 0 || f >= L.F) return false;
    fr.g0 = L.gt_off[f]; fr.p0 = L.pr_off[f]; fr.c0 = L.iou_off[f]; fr.s0 = L.slot_off[f];
    fr.ng = L.gt_off[f + 1] - fr.g0; fr.np = L.pr_off[f + 1] - fr.p0;
    if (fr.ng < 0 || fr.np < 0 || fr.ng > L.max_n || fr.np > L.max_n || L.max_n > RN_MOT_MAX) return false;
    const int ns = fr.ng < fr.np ? fr.ng : fr.np;
    return fr.g0 >= 0 && fr.p0 >= 0 && fr.c0 >= 0 && fr.s0 >= 0 && (int64_t)fr.g0 + fr.ng <= L.n_gt &&
           (int64_t)fr.p0 + fr.np <= L.n_pr && fr.c0 + (int64_t)fr.ng * fr.np <= L.cells && (int64_t)fr.s0 + ns <= L.S;
}

// status int32 [2]: the highest code met and the first frame (or id, for the CSR) that met one (0xFFFFFFFF: none)
__device__ __forceinline__ void assoc_flag(int32_t *status, int code, int where) {
    atomicMax(&status[0], code);
    atomicMin(reinterpret_cast<unsigned *>(&status[1]), (unsigned)where);
}

static inline bool assoc_dims_ok(int64_t G, int64_t P) {
    return G >= 0 && P >= 0 && G <= RN_MOT_MAX_IDS && P <= RN_MOT_MAX_IDS && G * P <= RN_MOT_ASSOC_MAX_CELLS;
}
static inline bool assoc_lay_ok(int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells, int64_t S) {
    return F >= 0 && F <= INT_MAX && max_n >= 0 && max_n <= RN_MOT_MAX && n_gt >= 0 && n_pr >= 0 && n_gt <= INT_MAX && n_pr <= INT_MAX &&
           cells >= 0 && S >= 0 && S <= INT_MAX;
}

struct AssocWs {
    double *cd;                      // C widened to fp64 [G * P]
    char *lsap;                      // the identity problem's vectors (lsap_arrays_layout)
    int32_t *hist;                   // [RN_MOT_ALPHAS][G * P]: layer n - 1 counts the pairs with prefix length n; then M_k
    unsigned long long *tp_hist;     // [RN_MOT_ALPHAS + 1]: matched pairs by prefix length
};

__host__ __device__ static inline int64_t assoc_ws_layout(char *base, int64_t G, int64_t P, AssocWs *w) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *r = base ? base + o : nullptr; o += (bytes + 15) & ~(int64_t)15; return r; };
    AssocWs t;
    t.cd = reinterpret_cast<double *>(take(G * P * 8));
    t.lsap = take(lsap_arrays_layout(nullptr, G < P ? G : P, G < P ? P : G, nullptr));
    t.hist = reinterpret_cast<int32_t *>(take(G * P * 4 * RN_MOT_ALPHAS));
    t.tp_hist = reinterpret_cast<unsigned long long *>(take((RN_MOT_ALPHAS + 1) * 8));
    if (w) *w = t;
    return o;
}

extern "C" int64_t rn_mot_assoc_workspace_bytes(int64_t n_gid, int64_t n_pid) {
    if (!assoc_dims_ok(n_gid, n_pid)) return 0;
    return 16 + assoc_ws_layout(nullptr, n_gid, n_pid, nullptr);
}

// ---------------------------------------------------------------------------------------------- identity: counts
__global__ __launch_bounds__(MA_BLOCK) void assoc_counts_kernel(AssocLay L, const double *__restrict__ iou,
                                                                const int32_t *__restrict__ gt_id, const int32_t *__restrict__ pred_id,
                                                                int G, int P, double id_iou, int32_t *__restrict__ gc,
                                                                int32_t *__restrict__ pc, int32_t *__restrict__ C,
                                                                int32_t *__restrict__ status) {
    __shared__ int32_t sg[RN_MOT_MAX], sp[RN_MOT_MAX];
    const int f = blockIdx.x, t = threadIdx.x;
    AssocFrame fr;
    if (!assoc_frame(L, f, fr)) { if (t == 0) assoc_flag(status, RN_MOT_TOO_LARGE, f); return; }
    for (int i = t; i < fr.ng; i += MA_BLOCK) {
        const int g = gt_id[fr.g0 + i];
        const bool ok = g >= 0 && g < G;
        if (!ok) assoc_flag(status, RN_MOT_BAD_INDEX, f);
        sg[i] = ok ? g : -1;
    }
    for (int j = t; j < fr.np; j += MA_BLOCK) {
        const int p = pred_id[fr.p0 + j];
        const bool ok = p >= 0 && p < P;
        if (!ok) assoc_flag(status, RN_MOT_BAD_INDEX, f);
        sp[j] = ok ? p : -1;
    }
    __syncthreads();
    for (int i = t; i < fr.ng; i += MA_BLOCK) {
        const int g = sg[i];
        if (g < 0) continue;
        atomicAdd(&gc[g], 1);
        bool dup = false;
        for (int q = 0; q < i; ++q) dup |= sg[q] == g;
        if (dup) assoc_flag(status, RN_MOT_DUPLICATE_ID, f);
    }
    for (int j = t; j < fr.np; j += MA_BLOCK) {
        const int p = sp[j];
        if (p < 0) continue;
        atomicAdd(&pc[p], 1);
        bool dup = false;
        for (int q = 0; q < j; ++q) dup |= sp[q] == p;
        if (dup) assoc_flag(status, RN_MOT_DUPLICATE_ID, f);
    }
    if (fr.ng == 0 || fr.np == 0) return;
    const double *mat = iou + fr.c0;
    for (int k = t; k < fr.ng * fr.np; k += MA_BLOCK) {
        const int i = k / fr.np, j = k - i * fr.np;
        const int g = sg[i], p = sp[j];
        if (g >= 0 && p >= 0 && mat[k] >= id_iou) atomicAdd(&C[(int64_t)g * P + p], 1);
    }
}

extern "C" int rn_mot_id_counts(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                                const int32_t *slot_off, int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells,
                                int64_t S, const int32_t *gt_id, const int32_t *pred_id, int64_t n_gid, int64_t n_pid, double id_iou,
                                int32_t *gc, int32_t *pc, int32_t *C, int32_t *status, void *stream) {
    if (!assoc_lay_ok(F, max_n, n_gt, n_pr, cells, S) || !assoc_dims_ok(n_gid, n_pid) || !status) return RN_EINVAL;
    if ((n_gid && !gc) || (n_pid && !pc) || (n_gid * n_pid && !C)) return RN_EINVAL;
    if (F && (!gt_off || !pr_off || !iou_off || !slot_off || (n_gt && !gt_id) || (n_pr && !pred_id) || (cells && !iou))) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(status, 0, 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(status + 1, 0xFF, 4, s);
    if (e == hipSuccess && n_gid) e = hipMemsetAsync(gc, 0, n_gid * 4, s);
    if (e == hipSuccess && n_pid) e = hipMemsetAsync(pc, 0, n_pid * 4, s);
    if (e == hipSuccess && n_gid * n_pid) e = hipMemsetAsync(C, 0, n_gid * n_pid * 4, s);
    if (e != hipSuccess) return (int)e;
    if (F == 0) return RN_OK;
    const AssocLay L = {gt_off, pr_off, iou_off, slot_off, n_gt, n_pr, cells, S, (int)F, (int)max_n};
    hipLaunchKernelGGL(assoc_counts_kernel, dim3((unsigned)F), dim3(MA_BLOCK), 0, s, L, iou, gt_id, pred_id, (int)n_gid, (int)n_pid,
                       id_iou, gc, pc, C, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- identity: the id x id assignment
__global__ __launch_bounds__(64) void assoc_id_assign_kernel(const int32_t *__restrict__ C, int G, int P, char *__restrict__ ws,
                                                             int32_t *__restrict__ match, long long *__restrict__ info) {
    const int lane = threadIdx.x;
    AssocWs a;
    assoc_ws_layout(ws, G, P, &a);
    const int64_t GP = (int64_t)G * P;
    for (int64_t k = lane; k < GP; k += 64) a.cd[k] = (double)C[k];
    lsap_wave_sync();
    const bool tr = G > P;                                                   // scipy transposes tall problems
    const int nr = tr ? P : G, nc = tr ? G : P;
    const int64_t rs = tr ? 1 : P, cs = tr ? P : 1;
    LsapWs w;
    lsap_arrays_layout(a.lsap, nr, nc, &w);
    if (lsap_solve_wave<true>(a.cd, rs, cs, nr, nc, w, lane) != 0) { if (lane == 0) info[1] = RN_MOT_INFEASIBLE; return; }
    long long sum = 0;
    for (int g = lane; g < G; g += 64) {
        const int p = tr ? w.row4col[g] : w.col4row[g];                      // ground-truth id = solver column when transposed
        if (p < 0 || p >= P) continue;                                       // unmatched (G > P), never out of range after status 0
        match[g] = p;
        sum += C[(int64_t)g * P + p];
    }
    if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(&info[0]), (unsigned long long)sum);
}

extern "C" int rn_mot_id_assign(const int32_t *C, int64_t n_gid, int64_t n_pid, void *workspace, int32_t *match, int64_t *info,
                                void *stream) {
    if (!assoc_dims_ok(n_gid, n_pid) || !info || (n_gid && !match)) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(info, 0, 16, s);
    if (e == hipSuccess && n_gid) e = hipMemsetAsync(match, 0xFF, n_gid * 4, s);
    if (e != hipSuccess) return (int)e;
    if (n_gid == 0 || n_pid == 0) return RN_OK;                              // nothing to match: IDTP = 0
    if (!C || !workspace) return RN_EINVAL;
    hipLaunchKernelGGL(assoc_id_assign_kernel, dim3(1), dim3(64), 0, s, C, (int)n_gid, (int)n_pid,
                       reinterpret_cast<char *>(workspace) + 16, match, reinterpret_cast<long long *>(info));
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- HOTA: global alignment
// rowsum / colsum of every scored frame: one thread per row and per column, each a sequential ascending sum
__global__ __launch_bounds__(MA_BLOCK) void assoc_sums_kernel(AssocLay L, const double *__restrict__ iou, double *__restrict__ rowsum,
                                                              double *__restrict__ colsum, int32_t *__restrict__ status) {
    const int f = blockIdx.x, t = threadIdx.x;
    AssocFrame fr;
    if (!assoc_frame(L, f, fr)) { if (t == 0) assoc_flag(status, RN_MOT_TOO_LARGE, f); return; }
    if (fr.ng == 0 || fr.np == 0) return;
    const double *mat = iou + fr.c0;
    for (int i = t; i < fr.ng; i += MA_BLOCK) {
        double s = 0.0;
        for (int j = 0; j < fr.np; ++j) s = s + mat[(int64_t)i * fr.np + j];
        rowsum[fr.g0 + i] = s;
    }
    for (int j = t; j < fr.np; j += MA_BLOCK) {
        double s = 0.0;
        for (int i = 0; i < fr.ng; ++i) s = s + mat[(int64_t)i * fr.np + j];
        colsum[fr.p0 + j] = s;
    }
}

// workgroup g owns row g of pot.  Every test that skips an appearance depends on workgroup-uniform values only, so the barrier
// at the end of an appearance is reached by all threads or by none.
__global__ __launch_bounds__(MA_BLOCK) void assoc_align_kernel(AssocLay L, const double *__restrict__ iou,
                                                               const int32_t *__restrict__ gt_id, const int32_t *__restrict__ pred_id,
                                                               const int32_t *__restrict__ csr_off, const int32_t *__restrict__ csr_frame,
                                                               const int32_t *__restrict__ csr_row, int64_t n_csr, int P,
                                                               const double *__restrict__ rowsum, const double *__restrict__ colsum,
                                                               double *__restrict__ pot, int32_t *__restrict__ status) {
    const int g = blockIdx.x, t = threadIdx.x;
    const int e0 = csr_off[g], e1 = csr_off[g + 1];
    if (e0 < 0 || e1 < e0 || e1 > n_csr) { if (t == 0) assoc_flag(status, RN_MOT_BAD_INDEX, g); return; }
    double *row = pot + (int64_t)g * P;
    int last = -1;
    for (int e = e0; e < e1; ++e) {
        const int f = csr_frame[e], i = csr_row[e];
        AssocFrame fr;
        const bool ok = f > last && assoc_frame(L, f, fr) && fr.ng > 0 && fr.np > 0 && i >= 0 && i < fr.ng && gt_id[fr.g0 + i] == g;
        if (!ok) { if (t == 0) assoc_flag(status, RN_MOT_BAD_INDEX, g); continue; }
        last = f;
        const double *srow = iou + fr.c0 + (int64_t)i * fr.np;
        const double rsum = rowsum[fr.g0 + i];
        for (int j = t; j < fr.np; j += MA_BLOCK) {
            const int p = pred_id[fr.p0 + j];
            if (p < 0 || p >= P) { assoc_flag(status, RN_MOT_BAD_INDEX, g); continue; }
            const double s = srow[j];
            const double den = (colsum[fr.p0 + j] + rsum) - s;
            const double jac = den > MA_EPS ? s / den : 0.0;
            row[p] = row[p] + jac;                                           // the only add to this cell in this frame
        }
        __syncthreads();                                                     // the next frame's thread for this cell sees the sum
    }
}

extern "C" int rn_mot_hota_align(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                                 const int32_t *slot_off, int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells,
                                 int64_t S, const int32_t *gt_id, const int32_t *pred_id, const int32_t *csr_off,
                                 const int32_t *csr_frame, const int32_t *csr_row, int64_t n_csr, int64_t n_gid, int64_t n_pid,
                                 double *rowsum, double *colsum, double *pot, int32_t *status, void *stream) {
    if (!assoc_lay_ok(F, max_n, n_gt, n_pr, cells, S) || !assoc_dims_ok(n_gid, n_pid) || n_csr < 0 || n_csr > INT_MAX || !status)
        return RN_EINVAL;
    if (n_gid * n_pid && !pot) return RN_EINVAL;
    if (F && (!gt_off || !pr_off || !iou_off || !slot_off)) return RN_EINVAL;
    if (cells && (!iou || !gt_id || !pred_id || !rowsum || !colsum)) return RN_EINVAL;
    if (n_gid && (!csr_off || (n_csr && (!csr_frame || !csr_row)))) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(status, 0, 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(status + 1, 0xFF, 4, s);
    if (e == hipSuccess && n_gid * n_pid) e = hipMemsetAsync(pot, 0, n_gid * n_pid * 8, s);
    if (e != hipSuccess) return (int)e;
    if (F == 0 || cells == 0 || n_gid == 0 || n_pid == 0) return RN_OK;
    const AssocLay L = {gt_off, pr_off, iou_off, slot_off, n_gt, n_pr, cells, S, (int)F, (int)max_n};
    hipLaunchKernelGGL(assoc_sums_kernel, dim3((unsigned)F), dim3(MA_BLOCK), 0, s, L, iou, rowsum, colsum, status);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(assoc_align_kernel, dim3((unsigned)n_gid), dim3(MA_BLOCK), 0, s, L, iou, gt_id, pred_id, csr_off, csr_frame,
                       csr_row, n_csr, (int)n_pid, rowsum, colsum, pot, status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- HOTA: per-frame assignment
__global__ __launch_bounds__(64) void assoc_hota_assign_kernel(AssocLay L, const double *__restrict__ iou,
                                                               const int32_t *__restrict__ gt_id, const int32_t *__restrict__ pred_id,
                                                               int G, int P, const int32_t *__restrict__ gc, const int32_t *__restrict__ pc,
                                                               const double *__restrict__ pot, const double *__restrict__ alphas,
                                                               double *__restrict__ score, int32_t *__restrict__ slot_row,
                                                               int32_t *__restrict__ slot_col, double *__restrict__ slot_s,
                                                               int32_t *__restrict__ slot_n, int32_t *__restrict__ frame_status) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int f = blockIdx.x, lane = threadIdx.x;
    AssocFrame fr;
    if (!assoc_frame(L, f, fr)) { if (lane == 0) frame_status[f] = RN_MOT_TOO_LARGE; return; }
    const int ng = fr.ng, np = fr.np;
    if (ng == 0 || np == 0) { if (lane == 0) frame_status[f] = RN_MOT_OK; return; }
    const double *mat = iou + fr.c0;
    double *sc = score + fr.c0;
    int bad = 0, bad_index = 0;
    for (int k = lane; k < ng * np; k += 64) {
        const int i = k / np, j = k - i * np;
        const int g = gt_id[fr.g0 + i], p = pred_id[fr.p0 + j];
        double v = 0.0;
        if (g < 0 || g >= G || p < 0 || p >= P) bad_index = 1;
        else {
            const double po = pot[(int64_t)g * P + p];
            const double ga = po / ((double)(gc[g] + pc[p]) - po);
            v = ga * mat[k];
        }
        sc[k] = v;
        bad |= (v != v) || (v == INFINITY);                                  // -v: NaN or -inf, scipy's invalid entries
    }
    if (__ballot(bad_index) != 0ull) { if (lane == 0) frame_status[f] = RN_MOT_BAD_INDEX; return; }
    if (__ballot(bad) != 0ull) { if (lane == 0) frame_status[f] = RN_MOT_INVALID; return; }
    lsap_wave_sync();
    const bool tr = ng > np;
    const int nr = tr ? np : ng, nc = tr ? ng : np;
    const int64_t rs = tr ? 1 : np, cs = tr ? np : 1;
    LsapWs w;
    lsap_arrays_layout(lds, nr, nc, &w);
    if (lsap_solve_wave<true>(sc, rs, cs, nr, nc, w, lane) != 0) { if (lane == 0) frame_status[f] = RN_MOT_INFEASIBLE; return; }
    double al[RN_MOT_ALPHAS];
#pragma unroll
    for (int k = 0; k < RN_MOT_ALPHAS; ++k) al[k] = alphas[k] - MA_EPS;
    auto emit = [&](int pos, int r, int c) {                                 // pos < min(ng, np): inside the frame's slots
        const double s = mat[(int64_t)r * np + c];
        int n = 0;
#pragma unroll
        for (int k = 0; k < RN_MOT_ALPHAS; ++k) n += (n == k && s >= al[k]);  // the prefix of k that passes
        slot_row[fr.s0 + pos] = r;
        slot_col[fr.s0 + pos] = c;
        slot_s[fr.s0 + pos] = s;
        slot_n[fr.s0 + pos] = n;
    };
    if (!tr) {                                                               // every ground-truth row is assigned
        for (int r = lane; r < ng; r += 64) {
            const int c = w.col4row[r];
            if (c >= 0 && c < np) emit(r, r, c);
        }
    } else {                                                                 // ascending ground-truth row = solver column
        int base = 0;
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int c = c0 + lane;
            const int r = c < nc ? w.row4col[c] : -1;
            const bool has = r >= 0 && r < np;
            const unsigned long long m = __ballot(has);
            if (has) {
                const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < np) emit(pos, c, r);
            }
            base += __popcll(m);
        }
    }
    if (lane == 0) frame_status[f] = RN_MOT_OK;
}

extern "C" int rn_mot_hota_assign(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                                  const int32_t *slot_off, int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells,
                                  int64_t S, const int32_t *gt_id, const int32_t *pred_id, int64_t n_gid, int64_t n_pid,
                                  const int32_t *gc, const int32_t *pc, const double *pot, const double *alphas, double *score,
                                  int32_t *slot_row, int32_t *slot_col, double *slot_s, int32_t *slot_n, int32_t *frame_status,
                                  void *stream) {
    if (!assoc_lay_ok(F, max_n, n_gt, n_pr, cells, S) || !assoc_dims_ok(n_gid, n_pid)) return RN_EINVAL;   // a larger frame: no launch
    if (F == 0) return RN_OK;
    if (!gt_off || !pr_off || !iou_off || !slot_off || !frame_status || !alphas) return RN_EINVAL;
    if (cells && (!iou || !score || !gt_id || !pred_id || !gc || !pc || !pot)) return RN_EINVAL;
    if (S && (!slot_row || !slot_col || !slot_s || !slot_n)) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (S) e = hipMemsetAsync(slot_row, 0xFF, S * 4, s);                     // slots of a frame with a status stay "no pair"
    if (e == hipSuccess && S) e = hipMemsetAsync(slot_col, 0xFF, S * 4, s);
    if (e == hipSuccess && S) e = hipMemsetAsync(slot_s, 0, S * 8, s);
    if (e == hipSuccess && S) e = hipMemsetAsync(slot_n, 0, S * 4, s);
    if (e != hipSuccess) return (int)e;
    const int64_t n = max_n < 1 ? 1 : max_n;
    const size_t bytes = (size_t)lsap_arrays_layout(nullptr, n, n, nullptr);
    const AssocLay L = {gt_off, pr_off, iou_off, slot_off, n_gt, n_pr, cells, S, (int)F, (int)max_n};
    hipLaunchKernelGGL(assoc_hota_assign_kernel, dim3((unsigned)F), dim3(64), bytes, s, L, iou, gt_id, pred_id, (int)n_gid, (int)n_pid,
                       gc, pc, pot, alphas, score, slot_row, slot_col, slot_s, slot_n, frame_status);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

// ---------------------------------------------------------------------------------------------- HOTA: sequence reduction
__global__ __launch_bounds__(64) void assoc_hist_kernel(AssocLay L, const int32_t *__restrict__ frame_status,
                                                        const int32_t *__restrict__ slot_row, const int32_t *__restrict__ slot_col,
                                                        const int32_t *__restrict__ slot_n, const int32_t *__restrict__ gt_id,
                                                        const int32_t *__restrict__ pred_id, int G, int P, int32_t *__restrict__ hist,
                                                        unsigned long long *__restrict__ tp_hist) {
    const int f = blockIdx.x, lane = threadIdx.x;
    AssocFrame fr;
    if (!assoc_frame(L, f, fr) || fr.ng == 0 || fr.np == 0 || frame_status[f] != RN_MOT_OK) return;
    const int ns = fr.ng < fr.np ? fr.ng : fr.np;
    const int64_t GP = (int64_t)G * P;
    for (int i = lane; i < ns; i += 64) {
        const int r = slot_row[fr.s0 + i], c = slot_col[fr.s0 + i], n = slot_n[fr.s0 + i];
        if (r < 0 || r >= fr.ng || c < 0 || c >= fr.np || n < 0 || n > RN_MOT_ALPHAS) continue;
        const int g = gt_id[fr.g0 + r], p = pred_id[fr.p0 + c];
        if (g < 0 || g >= G || p < 0 || p >= P) continue;
        atomicAdd(&tp_hist[n], 1ull);
        if (n > 0) atomicAdd(&hist[(int64_t)(n - 1) * GP + (int64_t)g * P + p], 1);
    }
}

// M_k[cell] = pairs of the cell with prefix length > k: the suffix sum over the layers, in place
__global__ __launch_bounds__(MA_BLOCK) void assoc_suffix_kernel(int64_t GP, int32_t *__restrict__ hist) {
    const int64_t c = (int64_t)blockIdx.x * MA_BLOCK + threadIdx.x;
    if (c >= GP) return;
    int acc = 0;
    for (int k = RN_MOT_ALPHAS - 1; k >= 0; --k) {
        acc += hist[(int64_t)k * GP + c];
        hist[(int64_t)k * GP + c] = acc;
    }
}

__global__ __launch_bounds__(MA_BLOCK) void assoc_sum_kernel(int F, int64_t S, int64_t n_gt, int64_t n_pr,
                                                             const int32_t *__restrict__ frame_status, const double *__restrict__ slot_s,
                                                             const int32_t *__restrict__ slot_n, const int32_t *__restrict__ gc,
                                                             const int32_t *__restrict__ pc, int G, int P, const int32_t *__restrict__ hist,
                                                             const unsigned long long *__restrict__ tp_hist, double *__restrict__ result) {
    __shared__ int bad_frame;
    __shared__ double part[4][MA_BLOCK];
    const int k = blockIdx.x, t = threadIdx.x;
    if (t == 0) bad_frame = INT_MAX;
    __syncthreads();
    for (int f = t; f < F; f += MA_BLOCK)
        if (frame_status[f] != RN_MOT_OK) atomicMin(&bad_frame, f);
    __syncthreads();
    if (bad_frame != INT_MAX) {                                              // the host raises; nothing else is reported
        if (k == 0 && t == 0) {
            result[RN_MOT_ALPHAS * 7] = (double)frame_status[bad_frame];
            result[RN_MOT_ALPHAS * 7 + 1] = (double)bad_frame;
        }
        return;
    }
    double loc = 0.0, aa = 0.0, ar = 0.0, ap = 0.0;
    for (int64_t s = t; s < S; s += MA_BLOCK)
        if (slot_n[s] > k) loc = loc + slot_s[s];
    const int64_t GP = (int64_t)G * P;
    const int32_t *layer = hist + (int64_t)k * GP;
    for (int64_t c = t; c < GP; c += MA_BLOCK) {
        const int m = layer[c];
        if (m <= 0) continue;                                                // an empty cell adds +0.0
        const int g = (int)(c / P), p = (int)(c - (int64_t)g * P);
        const int u = gc[g] + pc[p] - m;
        const double md = (double)m;
        aa = aa + md * (md / (double)(u > 1 ? u : 1));
        ar = ar + md * (md / (double)(gc[g] > 1 ? gc[g] : 1));
        ap = ap + md * (md / (double)(pc[p] > 1 ? pc[p] : 1));
    }
    part[0][t] = loc; part[1][t] = aa; part[2][t] = ar; part[3][t] = ap;
    __syncthreads();
    if (t < 4) {
        double s = 0.0;
        for (int i = 0; i < MA_BLOCK; ++i) s = s + part[t][i];
        result[k * 7 + 3 + t] = s;
    }
    if (t == 0) {
        unsigned long long tp = 0;
        for (int n = k + 1; n <= RN_MOT_ALPHAS; ++n) tp += tp_hist[n];
        result[k * 7 + 0] = (double)tp;
        result[k * 7 + 1] = (double)((unsigned long long)n_gt - tp);
        result[k * 7 + 2] = (double)((unsigned long long)n_pr - tp);
    }
}

extern "C" int rn_mot_hota_reduce(const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off, const int32_t *slot_off,
                                  int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells, int64_t S,
                                  const int32_t *frame_status, const int32_t *slot_row, const int32_t *slot_col, const double *slot_s,
                                  const int32_t *slot_n, const int32_t *gt_id, const int32_t *pred_id, const int32_t *gc,
                                  const int32_t *pc, int64_t n_gid, int64_t n_pid, void *workspace, double *result, void *stream) {
    if (!assoc_lay_ok(F, max_n, n_gt, n_pr, cells, S) || !assoc_dims_ok(n_gid, n_pid) || !workspace || !result) return RN_EINVAL;
    if (F && (!gt_off || !pr_off || !iou_off || !slot_off || !frame_status)) return RN_EINVAL;
    if (S && (!slot_row || !slot_col || !slot_s || !slot_n || !gt_id || !pred_id)) return RN_EINVAL;
    if ((n_gid && !gc) || (n_pid && !pc)) return RN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    AssocWs a;
    assoc_ws_layout(reinterpret_cast<char *>(workspace) + 16, n_gid, n_pid, &a);
    const int64_t GP = n_gid * n_pid;
    hipError_t e = hipMemsetAsync(result, 0, RN_MOT_ASSOC_RESULT * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.tp_hist, 0, (RN_MOT_ALPHAS + 1) * 8, s);
    if (e == hipSuccess && GP) e = hipMemsetAsync(a.hist, 0, GP * 4 * RN_MOT_ALPHAS, s);
    if (e != hipSuccess) return (int)e;
    const AssocLay L = {gt_off, pr_off, iou_off, slot_off, n_gt, n_pr, cells, S, (int)F, (int)max_n};
    if (F && S && GP) {
        hipLaunchKernelGGL(assoc_hist_kernel, dim3((unsigned)F), dim3(64), 0, s, L, frame_status, slot_row, slot_col, slot_n, gt_id,
                           pred_id, (int)n_gid, (int)n_pid, a.hist, a.tp_hist);
        RN_LAUNCH_CHECK();
        hipLaunchKernelGGL(assoc_suffix_kernel, dim3(rn_blocks(GP, MA_BLOCK)), dim3(MA_BLOCK), 0, s, GP, a.hist);
        RN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(assoc_sum_kernel, dim3(RN_MOT_ALPHAS), dim3(MA_BLOCK), 0, s, (int)F, S, n_gt, n_pr, frame_status, slot_s, slot_n,
                       gc, pc, (int)n_gid, (int)n_pid, a.hist, a.tp_hist, result);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

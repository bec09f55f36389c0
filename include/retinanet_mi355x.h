/*
 * retinanet_mi355x.h -- C ABI of libretinanet_mi355x.so (gfx950 / MI355X).
 *
 * The reference (DerekGloudemans/3D-playground) has no native layer: its hot path is Python on top of
 * torch / torchvision / numpy.  This library is the hand-written HIP layer inserted under the same Python
 * surface.  Every entry point takes raw DEVICE pointers, sizes and a hipStream_t (as void*), launches on
 * that stream without synchronising, allocates nothing, and returns 0 (hipSuccess) or a hipError_t /
 * RN_E* code.  Tensors are dense row-major fp32 unless a comment says otherwise.  No torch types cross
 * this boundary; the ctypes binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Each function cites the reference code it replaces.  D/ = pytorch_retinanet_detector_directional/retinanet/,
 * R/ = retinanet/ of the reference checkout.
 */
#ifndef RETINANET_MI355X_H
#define RETINANET_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RN_OK 0
#define RN_EINVAL 10001      /* bad size / unsupported shape */
#define RN_ETOOMANY 10002    /* more ground-truth rows per image than RN_MAX_GT */
#define RN_MAX_GT 256
#define RN_LEVELS 5

const char *rn_version(void);
/* Device the calling thread is bound to must be gfx950; returns 0 when it is. */
int rn_check_device(void);

/* ---------------------------------------------------------------- anchors ---------------------------------
 * Replaces Anchors.forward + generate_anchors + shift (D/anchors.py:21-40, 42-73, 109-129): levels 3..7,
 * 9 boxes per cell (ratio-major, scale-minor), fp64 arithmetic with ONE rounding to fp32, order
 * level -> row -> col -> box.  out: [A,4] fp32 (x1,y1,x2,y2). */
int64_t rn_anchor_count(int height, int width);
void rn_anchor_base_boxes(double out[RN_LEVELS * 9 * 4]);           /* host helper, numpy-identical fp64 */
int rn_anchors_fwd(float *out, int height, int width, void *stream);

/* ---------------------------------------------------------------- IoU -------------------------------------
 * Replaces calc_iou (D/losses.py:5-22): a [A,4] x b [N,4] -> iou [A,N]; no +1, union clamped at 1e-8. */
int rn_pairwise_iou(const float *a, const float *b, float *iou, int64_t A, int N, void *stream);

/* ---------------------------------------------------------------- focal / smooth-L1 / VP loss -------------
 * Replaces FocalLoss.forward, directional (D/losses.py:27-362, label_cols = 27, n_reg = 12) and 2D
 * (R/losses.py:27-177, label_cols = 5, n_reg = 4) in ONE launch each way (forward incl. the batch reduction): corner-envelope /
 * box IoU against every valid label row, max + first-argmax, 0.4/0.5 bands, alpha=.25 gamma=2 focal BCE on
 * clamp(cls,1e-4,1-1e-4), and for positives the smooth-L1 (beta 1/9; 20 values with the 0.5 top-corner
 * weight, or 4 std-scaled deltas) and the vanishing-point cosine term.
 *
 *   cls [B,A,C] post-sigmoid, reg [B,A,n_reg], anchors [A,4], ann [B,N,label_cols] (padding rows: class -1)
 *   workspace: rn_focal_workspace_bytes(B, A) bytes, written by fwd, read by bwd (per-image statistics).  Its first
 *           rn_focal_workspace_zero_bytes(B) bytes hold the forward's completion counters (one per image + one for the
 *           batch) and must be ZERO when rn_focal_loss_fwd is called; the kernel leaves them zero, so a workspace can be
 *           reused call after call without clearing it again (re-zero it after an aborted launch).  One workspace
 *           serves one stream at a time.
 *   losses: 3 floats  (cls, reg, vp; vp = 0 for the 2D variant).  An all-empty batch yields vp = NaN
 *           (the reference raises there, D/losses.py:362; the Python binding raises before launching).
 *   bwd: grad_losses = 3 device floats (dL/dcls_loss, dL/dreg_loss, dL/dvp_loss); writes dense
 *        dcls [B,A,C] and dreg [B,A,n_reg] (zeros where no gradient flows).
 */
int64_t rn_focal_workspace_bytes(int B, int64_t A);
int64_t rn_focal_workspace_zero_bytes(int B);
int rn_focal_loss_fwd(const float *cls, const float *reg, const float *anchors, const float *ann,
                      int B, int64_t A, int C, int N, int directional,
                      void *workspace, float *losses, void *stream);
int rn_focal_loss_bwd(const float *cls, const float *reg, const float *anchors, const float *ann,
                      int B, int64_t A, int C, int N, int directional,
                      const void *workspace, const float *grad_losses,
                      float *dcls, float *dreg, void *stream);
/* Assignment only (test / debugging aid): iou_max [B,A] fp32, argmax [B,A] int32 (index among VALID rows,
 * -1 for an image without labels), state [B,A] int32 in {-1 ignore, 0 negative, 1 positive}. */
int rn_assign(const float *anchors, const float *ann, int B, int64_t A, int N, int directional,
              float *iou_max, int32_t *argmax, int32_t *state, void *stream);

/* NEED SETS of the regression tower's forward.  The loss reads the regression output at the positive anchors only (rn_assign's rule: best
 * IoU >= 0.5 against the image's valid labels), so the labels decide before the forward which 4x4 output tiles of which pyramid level
 * are ever read: P0 = the tiles that hold a pixel with a positive anchor; the 3x3 layers below need its dilations D^k on the tile grid of
 * one image of one level.  anchors [A,4] in level order, per_pixel anchors per pixel, pixels row-major; H / W: n_levels (<= RN_MAX_GROUP)
 * HOST ints, sum H*W*per_pixel == A.  flags: RN_REG_NEED_ARRAYS arrays of Tpad bytes each (Tpad a multiple of 16 that holds every tile;
 * 16-byte aligned), in the tile order of rn_wino_group (levels concatenated; image, tile row, tile column), zeroed and filled here on
 * the device, no host read: [0] P0, [1] D^2(P0), [2] D^3(P0), [3] D^4(P0), [4] D^5(P0), [5] D(P0).  rn_tile_lists makes their work lists. */
#define RN_REG_NEED_ARRAYS 6
int rn_reg_need_tiles(const float *anchors, const float *ann, int B, int64_t A, int N, int directional, int n_levels,
                      const int *H, const int *W, int per_pixel, void *flags, int64_t Tpad, void *stream);

/* ---------------------------------------------------------------- decode / clip ---------------------------
 * rn_decode_dir replaces BBoxTransform.forward (D/utils.py:102-149): reg [B,A,12] -> boxes [B,A,20].
 * rn_decode_2d  replaces BBoxTransform.forward (R/utils.py:102-126) with std (.1,.1,.2,.2) and, when
 * clip != 0, ClipBoxes.forward fused (R/utils.py:134-144): deltas [B,A,4] -> boxes [B,A,4].
 * rn_clip_boxes is the standalone in-place ClipBoxes. */
int rn_decode_dir(const float *anchors, const float *reg, float *boxes, int B, int64_t A, void *stream);
/* Decode of the score filter's survivors only (the eval branches decode all B*A anchors at D/model.py:347 and then keep
 * <= 10 000, :322-328 / :368-374): candidate k (k < min(*count, max_candidates)) is flat anchor sel_idx[k] of [B*A];
 * writes boxes [max_candidates,20] (same per-anchor arithmetic as rn_decode_dir: bit-identical rows), cand_scores[k] =
 * scores[sel_idx[k] * score_stride] and, when cand_image != NULL, the image index sel_idx[k] / A (D/model.py:314-316).
 * count stays on the device (no host sync). */
int rn_decode_dir_select(const float *anchors, const float *reg, int64_t A, const float *scores, int64_t score_stride,
                         const int32_t *sel_idx, const int32_t *count, int max_candidates, float *boxes,
                         float *cand_scores, int32_t *cand_image, void *stream);
int rn_decode_2d(const float *anchors, const float *deltas, float *boxes, int B, int64_t A,
                 int clip, float width, float height, void *stream);
int rn_clip_boxes(float *boxes, int64_t n, float width, float height, void *stream);

/* ---------------------------------------------------------------- score filter + NMS ----------------------
 * The eval branch of ResNet.forward (D/model.py:311-397, R/model.py:283-311).
 *
 * rn_rowmax: scores[n] = max_c cls[n,c], classes[n] = first argmax (int64)          (D/model.py:320)
 * rn_threshold_select: the adaptive loop "t = start; repeat { mask = s > t; cnt = sum(mask); t *= 10**0.2 }
 *   until cnt <= keep" (D/model.py:322-328, 368-374) evaluated as one histogram pass; fixed_threshold >= 0
 *   selects the plain "s > thr" of the 2D path instead (R/model.py:289).  scores has `stride` floats between
 *   consecutive elements (class column of a [A,C] matrix).  Outputs, all device: count[0] = number selected,
 *   sel_idx[0..count) = indices in increasing order (the order a boolean mask gives).
 * rn_nms: greedy NMS (torchvision.ops.nms contract: score-descending, suppress IoU > thr; ties by lower
 *   index) over `count[0]` candidates: boxes are rows box_idx[i] of `boxes` (row stride box_stride floats,
 *   4 coords at column box_col); category[i] (may be NULL) reproduces batched_nms' fp32 offset trick
 *   (D/model.py:47-57).  keep[0..keep_count[0]) = positions into the candidate list, score-descending.
 * Workspace sizes are returned by rn_post_workspace_bytes(max_candidates).
 */
int64_t rn_post_workspace_bytes(int64_t n_scores, int64_t max_candidates);
int rn_rowmax(const float *cls, int64_t n, int C, float *scores, int64_t *classes, void *stream);
int rn_threshold_select(const float *scores, int64_t n, int64_t stride, double start, int keep,
                        double fixed_threshold, void *workspace, int32_t *count, int32_t *sel_idx, void *stream);
int rn_nms(const float *boxes, int64_t box_stride, int box_col, const float *scores, int64_t score_stride,
           const int32_t *cand_idx, const int32_t *category, const int32_t *count, int max_candidates,
           float iou_thr, void *workspace, int32_t *keep, int32_t *keep_count, void *stream);

/* ---------------------------------------------------------------- homography ------------------------------
 * Replaces Homography.i24_state_to_space + space_to_im = state_to_im (homography.py:305-320, 438-488) and
 * im_to_space + i24_space_to_state = im_to_state (homography.py:388-435, 274-303, 491-500).
 *   state [d,6] fp32 (x_rear, y_ctr, l, w, h, dir); image points [d,8,2] fp64; heights [d] fp32.
 *   P: 3x4 fp64 row-major, H: 3x3 fp64 row-major.  mat_index (may be NULL) picks a matrix per object
 *   (the reference's name = list of cameras); NULL uses matrix 0 for all (name = str).
 *   P2/H2 non-NULL = Homography_Wrapper (homography.py:840-862): objects whose corner-0 space y > 60 use
 *   the second set. */
int rn_state_to_space(const float *state, float *space, int64_t d, void *stream);
int rn_space_to_state(const double *space, float *state, int64_t d, void *stream);
int rn_state_to_im(const float *state, const double *P, const double *P2, const int32_t *mat_index,
                   double *im, int64_t d, void *stream);
int rn_space_to_im(const float *space, const double *P, const double *P2, const int32_t *mat_index,
                   double *im, int64_t d, void *stream);
int rn_im_to_space(const double *im, const float *heights, const double *H, const double *H2,
                   const int32_t *mat_index, double *space, int64_t d, void *stream);
int rn_im_to_state(const double *im, const float *heights, const double *H, const double *H2,
                   const int32_t *mat_index, float *state, int64_t d, void *stream);

/* ---------------------------------------------------------------- tracker: detection parsing ---------------
 * Replaces MC_Crop_Tracker.parse_detections with im_nms / space_nms (MC3D_crop_tracker.py:319-383, 592-636), the
 * step right after the MULTI_FRAME detector, without leaving the device or synchronising:
 *   keep scores > sigma_d (input order) -> NMS(phi_nms_im) on the image envelopes of the 8 corners, every box
 *   shifted by the constant 10 000 exactly as the reference does (its per-camera offset is computed and dropped,
 *   :610-613) -> image -> state through the camera's H of both wrapper homographies (switch at y > 60); with
 *   refine_height, state -> image through P, height_from_template, image -> state again (:366-370)
 *   -> NMS(phi_nms_space) on the road-plane footprints -> survivors in NMS order.
 *   scores [d] f32, labels [d] i64, boxes20 [d,20] f32 (16 corner coords + 2D box), camera_idxs [d] i64;
 *   H1,H2 [n_cam,3,3] / P1,P2 [n_cam,3,4] fp64 row-major, index = camera index (H2/P2 may be NULL: one homography;
 *   P1 is only read with refine_height); heights [d] f32 per input detection or NULL = 5 ft, which is what
 *   guess_heights returns for the integer labels the tracker passes (homography.py:502-517).
 *   Outputs sized for d rows; out_count[0] = rows valid.  d <= RN_PARSE_MAX.  perform_nms: bit 0 = image NMS, bit 1 =
 *   space NMS (3 = the reference's perform_nms=True, 0 = filter + transforms only, 1 = stop before the space NMS, where
 *   the tracker's estimate_ts_bias (tracker state, :373-374; not part of this call) looks at the boxes).
 * rn_md_iou: MC_Crop_Tracker.md_iou (:1030-1049), element-wise fp64 IoU of a[n,4], b[n,4] (union not clamped). */
#define RN_PARSE_MAX 16384
int64_t rn_parse_workspace_bytes(int64_t d);
int rn_parse_detections(const float *scores, const int64_t *labels, const float *boxes20, const int64_t *camera_idxs,
                        int64_t d, const double *H1, const double *H2, const double *P1, const double *P2, int n_cam,
                        const float *heights, float sigma_d, float phi_nms_im, float phi_nms_space,
                        int perform_nms, int refine_height, void *workspace,
                        float *out_state, int64_t *out_labels, float *out_scores, int64_t *out_cams,
                        int32_t *out_count, void *stream);
int rn_md_iou(const double *a, const double *b, double *out, int64_t n, void *stream);

/* ---------------------------------------------------------------- tracker: crop refinement ----------------
 * The block of MC_Crop_Tracker.track around the LOCALIZE detector (MC3D_crop_tracker.py:1172-1226), device-resident.
 * rn_crop_boxes: get_crop_boxes (:920-944): im_objs [n,8,2] fp64 (state_to_im of the priors) -> crop_boxes [n,4] fp64
 *   (x1,y1,x2,y2), squares of side max(w,h)*b; rois (may be NULL) [n,5] fp32 = (camera index, box), the argument of
 *   roi_align (:1183-1185).
 * rn_roi_align: torchvision.ops.roi_align(frames [N,C,H,W] fp32, rois, (out_h,out_w)) with its defaults
 *   (spatial_scale 1, sampling_ratio -1, aligned False), fp32, torchvision's operation order (third-party: restated,
 *   "parity unpinned"); nhwc4 != 0 writes [n,out_h,out_w,4] (C <= 4, rest 0), the stem convolution's layout.
 * rn_crop_select: everything after the detector (:1192-1226) for n objects: reg_boxes [n,A,20] / cls [n,A,C] (the
 *   LOCALIZE outputs), crop_boxes, cam_idxs [n] i64, pre_loc [n,6] priors -> per object the best of the cd_max most
 *   confident detections by (1-W)*IoU(footprint, prior footprint) + W*conf, as state [n,6] with the height refinement,
 *   class [n] i64, confidence [n].  A <= 4096, cd_max <= 256.  Heights start at 5 ft ("other"): what guess_heights
 *   returns for the integer classes the tracker passes. */
int rn_crop_boxes(const double *im_objs, const int64_t *cam_idxs, int n, double b, double *crop_boxes, float *rois,
                  void *stream);
int rn_roi_align(const float *frames, int N, int C, int H, int W, const float *rois, int n, int out_h, int out_w,
                 float *out, int nhwc4, void *stream);
int rn_crop_select(const float *reg_boxes, const float *cls, const double *crop_boxes, const int64_t *cam_idxs,
                   const float *pre_loc, const double *H1, const double *H2, const double *P1, const double *P2,
                   int n_cam, int n, int A, int C, double cs, int cd_max, float W, float *out_state, int64_t *out_cls,
                   float *out_conf, void *stream);

/* ---------------------------------------------------------------- tracker: Kalman filter -------------------
 * The tensor algebra of Torch_KF (util_track/kf.py:264-403), one lane per object.  X [n,6] fp32 (x,y,l,w,h,v),
 * P [n,6,6] fp32, D [n] fp32 travel direction, T [n] fp64 time stamps, F [6,6], Q [6,6], H [5,6], R [5,5], mu_R [5]
 * fp32.  dt: one fp64 value (dt_is_tensor 0: the reference's Python-float path, all fp32) or [n] fp64 values
 * (dt_is_tensor 1: Q*dt/dt_default is formed in fp64, kf.py:321-326).  F[0][5] is replaced by D*dt per object.
 * rn_kf_view (dt may be NULL = no prediction): out [n,6], or [n,7] with the direction inserted before the speed.
 * rn_kf_predict updates X, P, T in place.  rn_kf_update applies measurements z [m,5] fp64 to the objects rows[m]
 * (distinct rows), innovation in fp64, S^-1 by fp32 Gauss-Jordan with partial pivoting. */
int rn_kf_view(const float *X, const float *D, const float *F, const double *dt, int dt_is_tensor, int with_direction,
               float *out, int n, void *stream);
int rn_kf_predict(float *X, float *P, const float *D, double *T, const float *F, const float *Q, const double *dt,
                  int dt_is_tensor, double dt_default, int n, void *stream);
int rn_kf_update(float *X, float *P, const int32_t *rows, const double *z, const float *H, const float *R,
                 const float *mu_R, int m, void *stream);

/* ---------------------------------------------------------------- tracker: association --------------------
 * The middle of MC_Crop_Tracker.match_hungarian (MC3D_crop_tracker.py:637-731) without leaving the device.
 * rn_track_cost: pre [n, pre_stride] / det [m, det_stride] fp32 states, direction at column 5 (Torch_KF.view with
 *   with_direction gives 7 columns, parse_detections 6) -> cost [n,m] fp64 = 1 - md_iou of the fp32 road-plane
 *   footprints (min / max of the four bottom corners of state_to_space), md_iou's operation order (:1030-1049), the
 *   union not clamped (0/0 -> NaN, which the assignment reports as invalid, as scipy raises).
 * rn_linear_sum_assignment: scipy.optimize.linear_sum_assignment (its rectangular_lsap: Crouse 2016, shortest
 *   augmenting path, scipy's column order and tie rule) on cost [nr,nc] fp64 row-major, transposed by strides when
 *   nr > nc; then the gate of match_hungarian (:719-723): a pair whose cost is > max_cost is dropped (+inf: no gate).
 *   row_match [nr] i32 = matched column or -1; n_matched[0] = pairs kept; status[0] = 0 ok, 1 invalid (a NaN or -inf
 *   entry), 2 infeasible (no finite complete assignment) -- both with no matches, what match_hungarian's
 *   `except ValueError: return []` gives.  No synchronisation.  min(nr,nc) <= RN_LSAP_MAX_MIN, max(nr,nc) <=
 *   RN_PARSE_MAX.  workspace: rn_lsap_workspace_bytes(nr, nc) bytes. */
#define RN_LSAP_MAX_MIN 4096
int rn_track_cost(const float *pre, int64_t pre_stride, const float *det, int64_t det_stride, int64_t n, int64_t m,
                  double *cost, void *stream);
int64_t rn_lsap_workspace_bytes(int64_t nr, int64_t nc);
int rn_linear_sum_assignment(const double *cost, int64_t nr, int64_t nc, double max_cost, void *workspace,
                             int32_t *row_match, int32_t *n_matched, int32_t *status, void *stream);

/* ---------------------------------------------------------------- tracker: time stamp bias ----------------
 * MC_Crop_Tracker.estimate_ts_bias (MC3D_crop_tracker.py:237-315), the step between the transforms and the space NMS
 * of parse_detections when est_ts is set (:373-374, the reference's default), without leaving the device.
 * rn_estimate_ts_bias: boxes [d, box_stride] fp32 states (x,y,l,w,h,direction) and camera_idxs [d] i64 as the parser
 *   leaves them before the space NMS; d_count (may be NULL) = a device word holding the rows valid (the parser's
 *   out_count), clamped to d, so the call needs no host copy of it.  objs [n, obj_stride] = Torch_KF.view with
 *   with_direction (direction at column 5, speed at column 6).  timestamps / ts_bias [n_cam] fp64 on the device; ts_bias
 *   is updated in place.  Steps: mean speed per direction (:258-265, an empty direction takes +-mu_v); fp32 road-plane
 *   footprints and md_iou in fp64 (:1030-1049) for every i < j; the pairs from different cameras with iou > phi in the
 *   order i ascending, j ascending (:284-289); per pair the two entries (cam_i, cam_j, x_j - x_i) and (cam_j, cam_i,
 *   x_i - x_j), both with the direction of detection i; time_error = dx / vel - fp32(ts[cam2] - ts[cam1]) in fp32
 *   (:292-303); then serially, in list order, for cam1 != 0 (:311-315):
 *     ts_bias[cam1] = fp32(fp32((1 - alpha) * ts_bias[cam1]) + fp32(alpha) * (-time_error + fp32(ts_bias[cam2])))
 *   which is what torch's promotion makes of the reference's mix of Python floats and a 0-d fp32 tensor.
 *   info[0] = number of pairs, info[1] = status: 0 ok; 1 more pairs than max_pairs; 2 a camera index outside
 *   [0, n_cam) -- with 1 and 2 ts_bias is left untouched.  pairs_out [max_pairs,2] i32 (i, j) and te_out [max_pairs,2]
 *   fp32 (the time_error of the pair's two entries) may be NULL.  d == 0 or n == 0: info = (0, 0), nothing else (the
 *   reference's early returns).  No synchronisation.  d <= RN_PARSE_MAX, n_cam <= RN_TS_MAX_CAMS.
 *   workspace: rn_ts_bias_workspace_bytes(d, max_pairs) bytes. */
#define RN_TS_MAX_CAMS 1024
int64_t rn_ts_bias_workspace_bytes(int64_t d, int64_t max_pairs);
int rn_estimate_ts_bias(const float *boxes, int64_t box_stride, const int64_t *camera_idxs, int64_t d,
                        const int32_t *d_count, const float *objs, int64_t obj_stride, int64_t n,
                        const double *timestamps, double *ts_bias, int n_cam, double phi, double alpha, float mu_v,
                        void *workspace, int64_t max_pairs, int32_t *pairs_out, float *te_out, int32_t *info,
                        void *stream);

/* ---------------------------------------------------------------- tracker: crop frame front end ----------
 * The start of a crop frame in MC_Crop_Tracker.track (MC3D_crop_tracker.py:1150-1171), one lane per track, without
 * leaving the device.  X [n,6], D [n] fp32, T [n] fp64, F [6,6] fp32: the filter's tensors (see rn_kf_view).  centers
 * [n_cam,2] fp32 camera centres of view in state space; stamps / bias [n_cam] fp64 = timestamps and ts_bias.
 *   pre_loc [n,7] fp32: exactly what rn_kf_view writes for the scalar dt = 1/30.0 with direction (:1150).
 *   cam [n] i32: per track dist_k = |(cx_k - x)(cx_k - x) + (cy_k - y)(cy_k - y)| of that view in fp32, one rounding per
 *     operation (:1156-1162); the first k attaining the minimum, a NaN distance counting as smaller than any number,
 *     so the first NaN wins -- torch.argmin's rule on the CPU (:1163).
 *   dt [n] fp64 = (stamps[cam] + bias[cam]) - T (:1169-1171), the per-object dt of the predict that follows.
 * n == 0: success, nothing launched.  n_cam < 1: hipErrorInvalidValue.  No synchronisation. */
int rn_track_crop_prior(const float *X, const float *D, const double *T, const float *F, const float *centers,
                        const double *stamps, const double *bias, int n_cam, float *pre_loc, int32_t *cam, double *dt,
                        int n, void *stream);

/* ---------------------------------------------------------------- fitting the filter ----------------------
 * The two pieces of fit_filter_3D.py that the transforms and the filter kernels above do not cover.
 * rn_fit_nearest (fit_filter_3D.py:356-375): B frames, each with one ground-truth state gt [B,6] fp32 and the
 *   detections det [offsets[b], offsets[b+1]) of det [D,6] fp32 states (offsets [B+1] i32, clamped into [0, D]).  Per
 *   frame: the fp32 road-plane footprints (min / max of corners 0..3 of i24_state_to_space, :331-336 and :357-361), the
 *   script's own iou (:30-61; no epsilon, max(0, .) per factor) in fp32, distance 1.0 - iou, and the first detection
 *   whose distance is strictly below the running minimum (:363-372): ties go to the lowest index, a NaN distance (0/0)
 *   never wins.  rows [B] i32 = the chosen row of det, or -1 for an empty frame (the script's `continue`, :343-344) and
 *   for a frame in which no distance compared below infinity (the script would fail on None - gt_state; the frame is
 *   skipped and counted).  resid [B,5] fp32: det[row,:5] - gt[b,:5] (:374-375) of the frames with a match, compacted in
 *   frame order; the rows behind the count are not written.  info[0] = frames with a match, info[1] = empty frames,
 *   info[2] = frames without a comparable distance.  No synchronisation.  B, D <= RN_FIT_MAX.
 * rn_residual_moments (:292-299, :377-384, :426-434, :471-478): E [N,k] fp32, k <= RN_MOMENTS_MAX_K; group (may be
 *   NULL: one group) [N] i32 in [0, G), G <= RN_MOMENTS_MAX_G, rows with another id are left out.  Per group: count,
 *   mean [G,k] fp32 and the population covariance [G,k,k] fp32 (divided by the count), centred on the fp32 mean with the
 *   differences rounded to fp32 (the script's `vec - mean`); the sums run in fp64 in a fixed order (no atomics: the
 *   same bits every run) and are rounded to fp32 once.  A group without rows gets count 0 and zeros. */
#define RN_FIT_MAX (1 << 24)
#define RN_MOMENTS_MAX_K 8
#define RN_MOMENTS_MAX_G 16
int rn_fit_nearest(const float *gt, const float *det, const int32_t *offsets, int64_t B, int64_t D, int32_t *rows,
                   float *resid, int32_t *info, void *stream);
int rn_residual_moments(const float *E, int64_t N, int k, const int32_t *group, int G, float *mean, float *cov,
                        int32_t *count, void *stream);

/* ---------------------------------------------------------------- detector validation: mAP ----------------
 * retinanet/csv_eval.py (the same file in R/ and D/): evaluate, called after every epoch by D/train.py:168.  The
 * detections of the whole dataset stay in one device table of 32-byte rows
 *   { f32 x1, y1, x2, y2, score; i32 label, image, index (the detection's position in its image's input) }
 * and the host reads num_classes x (AP, annotation count) at the end.  No entry synchronises; all take any stream.
 * state [2] i32 on the device: state[0] = rows in the table (the append cursor), state[1] = status, an OR of the
 * RN_EVAL_* bits below; the caller zeroes both before the first image.  Ties in score keep dataset order everywhere
 * (image ascending, then selected rank; inside an image the lower input index first; -0.0 ranks with +0.0) -- the
 * reference's two np.argsort calls leave that order open.
 * rn_eval_select (_get_detections, csv_eval.py:102-123), one call per image, in stream order: keeps scores [K] fp32
 *   with score > score_threshold (fp32, strict; NaN is dropped), orders them by score descending and appends the first
 *   max_detections as rows at the cursor.  The box is boxes[k * box_stride + box_col .. + 4) -- box_col 0 for [K,4]
 *   boxes, 16 for the directional model's [K,20] rows (its 2D envelope).  img_rows [num_images,2] i32 receives the
 *   image's row range [begin, end).  K > RN_EVAL_MAX_K, a selected label outside [0, num_classes), or fewer than the
 *   selected number of free rows set RN_EVAL_TOO_MANY / RN_EVAL_BAD_LABEL / RN_EVAL_TABLE_FULL in state[1]; the image
 *   then appends nothing (an empty range).  max_detections <= RN_EVAL_MAX_DET (RN_EINVAL above).
 * rn_eval_match (evaluate, :189-213, with compute_overlap :21-35): annotations packed as ann_box [M,4] fp64 with
 *   ann_offsets [num_images * num_classes + 1] i32 in (image, class) order.  Every row gets tp[row] = 1 (true positive)
 *   or 0: rows are taken in table order; no annotation in the row's (image, class) -> 0; else the fp64 overlap with each
 *   of them, the union (area_a + area_b) - iw*ih clamped at DBL_EPSILON, no +1; the first maximum; 1 when it is >=
 *   iou_threshold and that annotation has not been taken, else 0 -- also when another, free annotation clears the
 *   threshold; a NaN overlap gives 0 and takes nothing.  Any number of annotations per group.  num_annotations
 *   [num_classes] i32 counts every image's annotations (:192).  taken: M bytes of workspace.
 * rn_eval_ap (:216-235 and _compute_ap :38-62): order [table_rows] i32 = the rows sorted stably by (label ascending,
 *   score descending) -- an LSD radix sort, tiles of RN_EVAL_SORT_TILE rows, RN_EVAL_SORT_SPAN rows per workgroup --
 *   of which the first state[0] entries are written; ap [num_classes] fp64: cumulative TP / FP (integers), recall =
 *   tp / num_annotations, precision = tp / (tp + fp), the envelope by a reverse running maximum, the sum of
 *   (recall step) * envelope over the points where the recall changes, in a fixed order: the same bits every run.  A
 *   class without annotations gets 0, as does one without detections.  workspace: rn_eval_ap_workspace_bytes(table_rows)
 *   bytes, 16-byte aligned like the table.  table_rows <= RN_EVAL_MAX_ROWS, num_classes <= RN_EVAL_MAX_CLASSES. */
#define RN_EVAL_MAX_K (1 << 20)
#define RN_EVAL_MAX_DET 4096
#define RN_EVAL_MAX_ROWS (1 << 24)
#define RN_EVAL_MAX_CLASSES 256
#define RN_EVAL_SORT_TILE 64
#define RN_EVAL_SORT_SPAN 2048
#define RN_EVAL_OK 0
#define RN_EVAL_TOO_MANY 1
#define RN_EVAL_BAD_LABEL 2
#define RN_EVAL_TABLE_FULL 4
int rn_eval_select(const float *scores, const int64_t *labels, const float *boxes, int64_t box_stride, int64_t box_col,
                   int64_t K, float score_threshold, int max_detections, int image, int64_t num_images,
                   int num_classes, void *table, int64_t table_rows, int32_t *state, int32_t *img_rows, void *stream);
int rn_eval_match(const void *table, int64_t table_rows, const int32_t *img_rows, int64_t num_images, int num_classes,
                  const double *ann_box, const int32_t *ann_offsets, int64_t M, double iou_threshold, void *taken,
                  uint8_t *tp, int32_t *num_annotations, void *stream);
int64_t rn_eval_ap_workspace_bytes(int64_t table_rows);
int rn_eval_ap(const void *table, int64_t table_rows, const int32_t *state, const uint8_t *tp,
               const int32_t *num_annotations, int num_classes, void *workspace, double *ap, int32_t *order,
               void *stream);

/* ---------------------------------------------------------------- detector validation in 3D: cuboid AP, corner errors
 * Beyond the reference (its csv_eval.py scores four columns; on the directional model's rows it would read two corner
 * points as a box).  Detections are the directional model's [K,20] rows, columns 0:16 the corners fbl fbr bbl bbr ftl ftr
 * btl btr as (x, y); annotations are ann_corners [M,16] fp64 with ann_offsets [num_images * num_classes + 1] i32 in
 * (image, class) order, as rn_eval_match takes its boxes.  Table, img_rows and state are rn_eval_select's, unchanged.
 * No entry synchronises; all take any stream.  All arithmetic is fp64, one rounding per operation; no floating-point atomics.
 * rn_eval_corners, once per image right after its rn_eval_select on the same stream: corners [table_rows,16] fp32 gets
 *   columns 0:16 of boxes[row.index] for the rows img_rows[image] names (none after a status).  box_stride >= 16.
 * rn_eval_cuboid_overlap: per row the first maximum over ALL annotations of its (image, class) group of the IoU of two
 *   convex polygons -- the hull of the chosen corners of the detection and of the annotation: RN_EVAL_CUBOID_SILHOUETTE all 8,
 *   _BASE corners 0..3, _TOP corners 4..7.  Hull: points sorted by (x, y), exact duplicates dropped, monotone chain in which
 *   a cross product <= 0 pops (collinear points go); fewer than 3 vertices or a non-finite coordinate on either side gives 0.
 *   Intersection: the detection's hull cut by each edge of the annotation's (Sutherland-Hodgman, on the edge is inside, at
 *   most RN_EVAL_CUBOID_MAX_VERTS vertices), shoelace area clipped to [0, min(area_a, area_b)]; iou = inter /
 *   max(area_a + area_b - inter, DBL_EPSILON).  best_iou [table_rows] fp64, best_ann [table_rows] i32: the index inside the
 *   group, or -1 with 0.0 for a group without annotations and for rows behind the cursor.
 * rn_eval_cuboid_assign: thresholds [num_thresholds <= RN_EVAL_CUBOID_MAX_THRESHOLDS] fp64 ON THE DEVICE.  Per (group,
 *   threshold) the rows in table order: tp[t * table_rows + row] = 1 iff best_iou >= thresholds[t] and best_ann has not been
 *   taken at t (csv_eval.py:189-213: the candidate is the argmax over all annotations, taken or not), else 0.  matched
 *   [table_rows] i32: best_ann of the true positives at thresholds[0], else -1.  num_annotations [num_classes] i32 as
 *   rn_eval_match counts them.  taken: M * num_thresholds bytes of workspace.
 * rn_eval_cuboid_errors, for the true positives at thresholds[0] (tp: that threshold's table_rows flags): terms
 *   [table_rows,4] fp64 = best_iou, corner_px (the mean over the 8 corners of the distance in pixels, label order),
 *   corner_px / max(diag, DBL_EPSILON) with diag the diagonal of the min / max envelope of the annotation's 8 corners,
 *   corner_px with the detection's corners taken in the order 3 2 1 0 7 6 5 4 (turned by 180 degrees); zeros for every other
 *   row.  sums [num_classes,5] fp64 = n_tp, sum best_iou, sum corner_px, sum corner_px / diag, n_reversed (rows whose
 *   turned corner_px is strictly smaller), each added in table order. */
#define RN_EVAL_CUBOID_SILHOUETTE 0
#define RN_EVAL_CUBOID_BASE 1
#define RN_EVAL_CUBOID_TOP 2
#define RN_EVAL_CUBOID_MAX_VERTS 16
#define RN_EVAL_CUBOID_MAX_THRESHOLDS 8
int rn_eval_corners(const float *boxes, int64_t box_stride, int64_t K, int image, int64_t num_images,
                    const int32_t *img_rows, const void *table, int64_t table_rows, float *corners, void *stream);
int rn_eval_cuboid_overlap(const void *table, int64_t table_rows, const int32_t *img_rows, int64_t num_images,
                           int num_classes, const float *corners, const double *ann_corners, const int32_t *ann_offsets,
                           int64_t M, int overlap, double *best_iou, int32_t *best_ann, void *stream);
int rn_eval_cuboid_assign(const void *table, int64_t table_rows, const int32_t *img_rows, int64_t num_images,
                          int num_classes, const int32_t *ann_offsets, int64_t M, const double *best_iou,
                          const int32_t *best_ann, const double *thresholds, int num_thresholds, void *taken, uint8_t *tp,
                          int32_t *num_annotations, int32_t *matched, void *stream);
int rn_eval_cuboid_errors(const void *table, int64_t table_rows, const int32_t *state, int64_t num_images, int num_classes,
                          const float *corners, const double *ann_corners, const int32_t *ann_offsets, int64_t M,
                          const uint8_t *tp, const int32_t *matched, const double *best_iou, double *terms, double *sums,
                          void *stream);

/* ---------------------------------------------------------------- frame ingest ----------------------------
 * Replaces F.to_tensor + F.normalize of the reference's loaders (util_track/mp_loader.py:239-243,
 * perform_3D_detection_on_video_sequences.py:51-58) on device: frames uint8 [B,H,W,3] (as the decoder / cv2.resize
 * leaves them) -> fp32 (u8/255 - mean[c]) / std[c], three separate fp32 operations as torchvision performs them
 * (bit-identical to the CPU).  swap_rb != 0 applies the second caller's BGR->RGB swap.
 * layout 0: out = NCHW [B,3,H,W], the tensor the reference hands to the model;
 * layout 1: out = NHWC4 [B,H,W,4] (4th channel 0), the stem convolution's input layout. */
int rn_frame_ingest(const uint8_t *frames, int B, int H, int W, int swap_rb, float mean0, float mean1, float mean2,
                    float std0, float std1, float std2, int layout, float *out, void *stream);

/* ---------------------------------------------------------------- 4K frames: reduction + ingest ------------
 * The loader's cv2.resize(original_im, (1920, 1080)) of a 3840x2160 frame followed by to_tensor + normalize
 * (util_track/mp_loader.py:237-243) in one pass.  frames uint8 [B,H2,W2,3]; H2 and W2 even (the exact halving, the
 * loader's only case; anything else is RN_EINVAL).  Per channel the reduced byte is (a + b + c + d + 2) >> 2 of the 2x2
 * block -- what OpenCV's resize yields for an exact halving of 8-bit data (parity with cv2 itself unpinned: DESIGN.md,
 * "4K frames") -- then rn_frame_ingest's arithmetic unchanged: out equals rn_frame_ingest of the reduced bytes bit for
 * bit, layout 0 NCHW [B,3,H2/2,W2/2], layout 1 NHWC4 [B,H2/2,W2/2,4].  out_u8 (may be NULL): the reduced frame
 * uint8 [B,H2/2,W2/2,3], the reference's original_im. */
int rn_frame_ingest_half(const uint8_t *frames, int B, int H2, int W2, int swap_rb, float mean0, float mean1,
                         float mean2, float std0, float std1, float std2, int layout, float *out, uint8_t *out_u8,
                         void *stream);

/* ---------------------------------------------------------------- 4K frames: burnt-in time stamps ---------
 * timestamp_utilities.parse_frame_timestamp (timestamp_utilities.py:46-115) for B frames and up to RN_TS_MAX_SETS
 * (geometry, checksum table) sets tried in order (datareader.py:59-63), with the callers' fall-back.
 * frames: uint8 [H,W,3] each, frame b at frames + b * frame_stride, row y at + y * row_stride (bytes): a strip cut from
 *   a frame works as the frame.  Channel order B,G,R; swap_rb != 0 reads R,G,B.
 * sets: HOST array of G geometries.  The strip is rows [y0, y0+h), columns [x0, x0+n*w); a pixel outside the frame is
 *   dark.  White: gray > 127 with gray = (3735 B + 19235 G + 9798 R + 16384) >> 15.  Cell j = columns [j*w, (j+1)*w);
 *   cell 10 (the decimal point) is never looked at.  Six counts per cell: the white pixels of the row bands [0,h13),
 *   [h13,h23), [h23,h) crossed with the column halves [0,w12), [w12,w), in that order (band major).
 * tables: DEVICE int32 [G, RN_TS_MAX_KEYS, RN_TS_ROW]; row k of set g = the six counts of the table's k-th entry, then
 *   the decimal digit it stands for (0-9), then 0; rows at and beyond K are not read.  A cell reads as the FIRST row
 *   equal in all six counts; a cell without one fails the set, and the first such cell in j order is the one reported.
 * Per frame the first set that reads every cell is used.  Outputs, all on the device:
 *   times [B] fp64: the digits as one integer D over 10^max(n-11,0), one fp64 division (both exact, so the correctly
 *     rounded value of the decimal string); nobody reads the frame: prev[b] + 1/30.0 (one fp64 add) with prev fp64 [B],
 *     or NaN when prev is NULL
 *   status [B] i32: RN_TS_READ, RN_TS_FAILED (NaN) or RN_TS_FELL_BACK;  set_index [B] i32: the set used, or -1
 *   digits [B,RN_TS_MAX_CELLS] i8: the table row per cell of the set used (of the FIRST set when none reads), -1 for the
 *     point, beyond n, and a cell without an equal row
 *   fail_cell [B] i32: the first failing cell of the FIRST set, -1 if it read the frame
 *   mask (may be NULL) uint8 [B,h,n*w] of the FIRST set: its 0 / 255 threshold strip, the point's cell included.
 * RN_EINVAL before any launch: a null pointer (prev and mask excepted), B, H, W <= 0, n outside [1,RN_TS_MAX_CELLS], K
 * outside [1,RN_TS_MAX_KEYS], G outside [1,RN_TS_MAX_SETS], x0 or y0 negative, 0 <= h13 <= h23 <= h or 0 <= w12 <= w
 * violated, w or h < 1, w*h > RN_TS_MAX_CELL_PIXELS, a coordinate above RN_TS_MAX_COORD, row_stride < 3 W, frames that
 * overlap.  One launch (a workgroup per frame), no synchronisation. */
#define RN_TS_MAX_SETS 4
#define RN_TS_MAX_CELLS 16
#define RN_TS_MAX_KEYS 64
#define RN_TS_ROW 8
#define RN_TS_MAX_CELL_PIXELS 4096
#define RN_TS_MAX_COORD (1 << 24)
#define RN_TS_READ 0
#define RN_TS_FAILED 1
#define RN_TS_FELL_BACK 2
typedef struct rn_ts_geometry {
    int32_t x0, y0, w, h, n, h13, h23, w12, K;
} rn_ts_geometry;
int rn_parse_frame_timestamps(const uint8_t *frames, int B, int H, int W, int64_t frame_stride, int64_t row_stride,
                              int swap_rb, const rn_ts_geometry *sets, int G, const int32_t *tables, const double *prev,
                              double *times, int32_t *status, int32_t *set_index, int8_t *digits, int32_t *fail_cell,
                              uint8_t *mask, void *stream);

/* ---------------------------------------------------------------- training-batch augmentation -------------
 * The image chain of the reference's training loader (corrected_3D_dataset.py: Detection_Dataset.__getitem__, :330-478,
 * CROP == 0) on device, byte for byte what torchvision's PIL backend computes: frames uint8 [B,H,W,3] -> fp32 NCHW
 * [B,3,H,W].  The random draws and the label transforms stay on the host (retinanet_mi355x/augment.py); what travels per
 * image is one rn_augment_params record and two rows of resampling coefficients.
 *
 * rn_augment_params (104 bytes, 8-byte aligned):
 *   affine[6]  destination -> source matrix of Image.rotate (:369): cos / sin rounded to 15 decimals, centre (W/2, H/2),
 *              angle % 360, computed on the host exactly as Pillow does; source (sx, sy) = (a0 (x+.5) + a1 (y+.5) + a2,
 *              a3 (x+.5) + a4 (y+.5) + a5) in double, output 0 unless 0 <= sx < W and 0 <= sy < H, else the bilinear blend of the
 *              four taps around (sx-.5, sy-.5) with clamped indices, truncated to a byte
 *   rh, rw     size of the resized image (:334-335); only its top-left min(rh,H) x min(rw,W) is read (:339), the rest of
 *              the frame is noise bytes floor(fp32(k 2^-24) 255) (:338, 342)
 *   flip       != 0: F.hflip (:352), a mirrored column in the rotation's reads
 *   apply      != 0: the ColorJitter of self.im_tf (:177-180) runs, in the order order[4] (0 brightness, 1 contrast,
 *              2 saturation, 3 hue = nothing), each t = a + f (p - a) in fp32 with f = factors[op], 0 if t <= 0, 255 if
 *              t >= 255, else truncated; a = 0, the mean of L over the image as it stands (floor(sum / N + .5)), or the pixel's L;
 *              L = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *   dy, dx     the tile swap (:468-478) as a roll: out[:, y, x] = t[:, (y + dy) % H, (x + dx) % W], 0 <= dy < H, 0 <= dx < W
 * table_x int32 [B,W,1+RN_AUG_TAPS], table_y int32 [B,H,1+RN_AUG_TAPS]: per output index of Pillow's bilinear resize
 *   (horizontal pass first, uint8 between the passes) the first source index and the taps k = int(.5 + w 2^22); the output is
 *   clip((2^21 + sum k p) >> 22, 0, 255).  Rows at and beyond min(rw, W) / min(rh, H) are not read; a pass whose size does
 *   not change is skipped.
 * noise: uint8 [B,H,W,3] pad bytes, or null for the device generator (splitmix64 of seed * 0x9E3779B97F4A7C15 + the element's
 *   index in [B,H,W,3]; its top 24 bits are k).  workspace: rn_augment_workspace_bytes(B, H, W) bytes, 8-byte aligned: two uint8
 *   images per frame and one 64-bit sum per image.  Finish: (byte / 255 - mean[c]) / std[c] as rn_frame_ingest.
 * Five launches for the whole batch on the stream, no host synchronisation. */
#define RN_AUG_TAPS 7
typedef struct rn_augment_params {
    double affine[6];
    int32_t rh, rw, flip, apply;
    int32_t order[4];
    int32_t dy, dx;
    float factors[3];
    int32_t reserved;
} rn_augment_params;
int64_t rn_augment_workspace_bytes(int B, int H, int W);
int rn_augment_frames(const uint8_t *frames, int B, int H, int W, const rn_augment_params *params, const int32_t *table_x,
                      const int32_t *table_y, const uint8_t *noise, uint64_t seed, float mean0, float mean1, float mean2,
                      float std0, float std1, float std2, void *workspace, float *out, void *stream);

/* ---------------------------------------------------------------- crop-detector training batches ----------
 * The same loader with CROP > 0 (corrected_3D_dataset.py:330-390, 501-594), the crop detector's: the frame is resized, padded,
 * flipped and rotated as above, then a window (minx, miny, cw, ch) is cut out of it (F.crop, zero outside the frame), resized
 * to crop x crop, jittered, normalised and sometimes partly occluded.  Only the window is evaluated: device work is
 * proportional to the window areas and crop^2, no launch is sized by the frame.  frames uint8 [B,H,W,3] -> fp32 NCHW
 * [B,3,crop,crop].
 *
 * rn_augment_crop_params (128 bytes, 8-byte aligned):
 *   affine, rh, rw, flip, apply, order, factors   as in rn_augment_params
 *   win[4]      minx, miny, cw, ch: the window in the rotated frame's coordinates; minx / miny may be negative and the window
 *               may lie partly or wholly outside the frame; 1 <= cw, ch <= win_max
 *   occluded    != 0: inside occlude[4] = x0, y0, x1, y1 (0 <= x0 <= x1 <= crop, likewise y; the end is exclusive) the output
 *               is a raw value that replaces the normalised one (:588-592)
 * table_x, table_y: the first resize, as for rn_augment_frames.  table_cx, table_cy int32 [B,crop,1+K]: the second resize
 *   (cw -> crop horizontally, then ch -> crop vertically, uint8 between the passes), per output index the first source index
 *   and K taps, zero beyond a row's own; K >= the largest ceil(max(size / crop, 1)) * 2 + 1 of the batch.  A pass whose size
 *   does not change is skipped and its table is not read.
 * noise: uint8 [B,H,W,3] pad bytes or null (the generator of rn_augment_frames, read only where the window needs it).
 * occlusion: fp32 [B,3,crop,crop] read at the output coordinate inside occlude, or null: then the value is
 *   mean[c] + std[c] z, z = sqrt(-2 ln u1) cos(2 pi u2) in fp32 with u1 = (k1 + 1) 2^-24, u2 = k2 2^-24, k1 = bits 40..63 and
 *   k2 = bits 16..39 of splitmix64 of seed * 0x9E3779B97F4A7C15 + (the element's index in [B,3,crop,crop] | 2^63).
 * win_max: at least the largest cw and ch of the batch (a record beyond it is clamped: wrong pixels, no access outside).
 * workspace: rn_augment_crops_workspace_bytes(B, win_max, crop) bytes, 8-byte aligned.
 * Five launches for the whole batch on the stream (window, resize h, resize v, contrast sum, finish), no host synchronisation. */
typedef struct rn_augment_crop_params {
    double affine[6];
    int32_t rh, rw, flip, apply;
    int32_t order[4];
    int32_t win[4];
    float factors[3];
    int32_t occluded;
    int32_t occlude[4];
} rn_augment_crop_params;
int64_t rn_augment_crops_workspace_bytes(int B, int win_max, int crop);
int rn_augment_crops(const uint8_t *frames, int B, int H, int W, const rn_augment_crop_params *params, const int32_t *table_x,
                     const int32_t *table_y, const int32_t *table_cx, const int32_t *table_cy, int K, int win_max, int crop,
                     const uint8_t *noise, const float *occlusion, uint64_t seed, float mean0, float mean1, float mean2,
                     float std0, float std1, float std2, void *workspace, float *out, void *stream);

/* ---------------------------------------------------------------- convolution engine ----------------------
 * fp32 implicit-GEMM convolutions on the matrix cores (v_mfma_f32_32x32x2_f32).  Replaces nn.Conv2d +
 * BatchNorm2d(eval) + ReLU + residual add (D/utils.py:25-43, 60-80), PyramidFeatures (D/model.py:84-117) and
 * the head towers (D/model.py:139-157, 182-205), forward and backward (the reference gets the latter from
 * torch autograd / cuDNN).
 *
 * Activations are NHWC fp32.  Weights are re-packed once per optimizer step by rn_pack_weights into
 * [rows][Kpad] with K = kh*kw*Cin contiguous (Kpad = K rounded up to 32, zero filled).
 *
 * rn_conv_igemm computes, for every output pixel (n, oh, ow) and output channel c:
 *     acc = sum_{r<kh, s<kw, ci<Cin} x[n, ih, iw, ci] * w[c][r][s][ci]
 *     with  ih = (oh*a + p + r*b) >> div_shift  (contributes only if the numerator is >= 0, divisible by
 *     1 << div_shift and ih < Hi; iw likewise from ow, s and p_w),
 *     v = scale[c]*acc + shift[c];  mask_mode 1: v = mask[...] > 0 ? v : 0;  v += add[...];  v = act(v);
 *     mask_mode 2: v = mask[...] > 0 ? v : 0;  y = v.   (mask has the geometry of y: ReLU backward of the
 *     tensor the gradient flows into, applied before or after other gradient contributions are added.)
 *     in_relu != 0 applies max(x, 0) to the input as it is loaded (P7 = conv(ReLU(P6)), D/model.py:114-115).
 *   forward conv (stride st, padding pd):    a = st, b = +1, p = p_w = -pd, div_shift = 0
 *   data gradient of that conv:              a = 1,  b = -1, p = p_w = +pd, div_shift = log2(st), x = dY, and
 *                                            w packed as [Cin][kh][kw][Cout] (rn_pack_weights mode 1)
 * add_mode 1: add has the geometry of y (residual / gradient accumulation); 2: add is [N,Ha,Wa,Cout] read at
 * (oh>>1, ow>>1) -- the FPN nearest-upsample + add, cropped to the output (D/model.py:88-108).
 * batch strides are in floats; y_batch_stride lets a head write straight into its slice of the concatenated
 * [B, A, n] tensor (the reference's permute+view+cat, D/model.py:155-157, 302-304).
 *
 * Size limits (RN_EINVAL otherwise): the operands are read through 32-bit buffer offsets, so one input image
 * (Hi*Wi*Cin floats) plus the images a 256-pixel run of outputs can span ((255 / (Ho*Wo) + 1) * x_batch_stride) must
 * stay below 2 GiB, likewise the packed weights, and N*Ho*Wo below 2^31.  x, w_packed need 4-byte alignment only.
 */
typedef struct rn_conv_desc {
    int N, Hi, Wi, Cin;            /* input  [N,Hi,Wi,Cin]; Cin % 4 == 0 */
    int Ho, Wo, Cout;              /* output [N,Ho,Wo,Cout] */
    int kh, kw;
    int a, b, p, p_w, div_shift;   /* p applies to rows, p_w to columns */
    int act;                       /* 0 none, 1 ReLU, 2 sigmoid */
    int add_mode;                  /* 0 none, 1 same geometry, 2 nearest-upsample x2 */
    int Ha, Wa;
    int mask_mode;                 /* 0 none, 1 before the add, 2 after the activation; | RN_MASK_BITS (4): `mask` points to the
                                      masking tensor's SIGN BITS (see sign_out below) instead of the tensor */
    int in_relu;                   /* ReLU applied to x on load */
    int os, oo_h, oo_w, Hy, Wy;    /* output pixel (oh,ow) is stored at (oh*os+oo_h, ow*os+oo_w) of a [N,Hy,Wy,Cout]
                                      tensor (os = 1, offsets 0, Hy = Ho, Wy = Wo: dense).  add (mode 1) and mask
                                      are read at the same place.  Used by the stride-2 data gradient, which is
                                      computed per output-parity class. */
    int add2_mode;                 /* 0 none, 3: add2 is [N,Ha2,Wa2,Cout], added where the stored position has
                                      even row and column, read at (row/2, col/2): gradient of a 1x1 stride-2
                                      shortcut (D/model.py:265-270) without materialising its zeros */
    int Ha2, Wa2;
    int64_t add2_batch_stride;
    int64_t x_batch_stride, y_batch_stride, add_batch_stride;
    int64_t w_batch_stride;        /* 0: one weight tensor.  != 0 (floats): image n uses w_packed + n * w_batch_stride -- a batch of
                                      independent GEMMs in one launch (the 36 positions of the Winograd path); Ho*Wo must then
                                      be a multiple of 256 so that no tile spans two images */
    int w_format;                  /* 0: w_packed is the fp32 tensor of rn_pack_weights; 1: its pre-split form (rn_split_weights),
                                      accepted in RN_FP32_SPLIT mode only (RN_EINVAL otherwise; not by the split-K form);
                                      2 (round 4): the pre-split form, and the products are formed from the operands' FIRST bf16
                                      terms only (one MFMA instead of six) -- bf16 arithmetic on fp32 tensors, for the fp32 stem of
                                      the bf16 / fp8 engines; layers with at most 64 output channels, single launches */
    void *sign_out;                /* NULL, or uint32 words that receive the SIGN BITS of the result: bit (e & 31) of word (e >> 5)
                                      = (y[e] > 0) for every stored element at float offset e -- what the backward pass needs of a ReLU
                                      output (D/utils.py:60-80), at 1/32 of the bytes.  Needs Cout % 32 == 0 and y_batch_stride % 32
                                      == 0.  mask_mode | RN_MASK_BITS (4): `mask` points to such words (the consumer's side). */
    const void *x_amax;            /* RN_FP32_SPLIT3 (round 5): the AMAX TABLES of x: per image 256 bytes whose HIGHEST set byte is the fp32
                                      exponent field of the image's largest |value|; a lower byte e set means only that some lane's
                                      largest stored |value| had exponent e, and most exponents present leave no byte (what a
                                      producer's y_amax left, or rn_amax) -- the kernel takes the
                                      largest exponent present as the image's power-of-two scale for its fp16 split, row by row: GEMM
                                      row (image n, pixel r) uses table n * x_amax_img_stride when x_amax_row_stride == 0 (the usual
                                      form, img stride 1: an image's result then does not depend on what else is in the batch), or the
                                      plain uint32 WORD x_amax[r * x_amax_row_stride] (an fp32 bit pattern whose exponent field bounds
                                      the row) when it is not: the Winograd-stage GEMM, whose rows are tiles (rn_wino_input_group
                                      writes the words).  Required when w_format == 3. */
    void *y_amax;                  /* NULL, or the amax tables of the RESULT, one per image [N][256]: every kernel that finishes elements
                                      sets the byte of the largest exponent it stored in image n (plain stores, idempotent: several
                                      launches may fill one tensor); the caller zeroes the tables before the first.  Any product mode;
                                      not by the raw Winograd-stage GEMM (its result feeds a transform, not a convolution). */
    const float *w_unscale;        /* w_format == 3: per weight row the inverse 2^-s of the power-of-two scale its fp16 terms were
                                      written with (rn_split_weights_f16); [batch * Cout] when w_batch_stride != 0 */
    int x_amax_img_stride, x_amax_row_stride;
    const void *row_active;        /* NULL, or TILE ACTIVITY FLAGS for the Winograd-stage GEMM (w_batch_stride != 0) of a sparse gradient: one
                                      byte per row of an image (Ho*Wo of them, 16-byte aligned), 0 = the row of x is zero in every image and
                                      nobody reads that row of y.  A workgroup whose rows are all inactive computes nothing; rows of
                                      inactive tiles inside an active workgroup are computed from whatever x holds.  A kernel without the
                                      test ignores the flags (a dense result is always right). */
    const void *row_list;          /* NULL, or the same activity as a WORK LIST on the device (rn_tile_lists): int32 indices of the 128-row
                                      blocks of an image that hold an active row, ascending; row_list_n points to their int32 count.  The
                                      Winograd-stage GEMM then launches a grid fixed by the device's size -- row_list_grid workgroups, 0:
                                      a few per compute unit -- whose workgroups walk listed block x column tile x image with stride
                                      gridDim.x and visit nothing else.  Kernels without the list form fall back to row_active / dense. */
    const void *row_list_n;
    int row_list_grid;
} rn_conv_desc;
#define RN_MASK_BITS 4

/* How the fp32 convolution kernels (rn_conv_igemm*, rn_conv_wgrad*, and through them the Winograd GEMMs) form their
 * products.  Operands, accumulation, epilogue and results are fp32 either way.
 *   RN_FP32_NATIVE  v_mfma_f32_32x32x2_f32 (157 TF peak).
 *   RN_FP32_SPLIT   each fp32 operand is split in registers into three bf16 terms h + m + l (exactly equal to it) and a
 *                   product is the sum of the six largest of the nine term products on v_mfma_f32_32x32x16_bf16 with the
 *                   fp32 accumulator; the three dropped terms are at most 2^-23 of the product (2^-25 rms), the size of
 *                   one fp32 rounding (csrc/mfma_split.h; DESIGN.md 4.6 has the measured errors of both modes against fp64).
 *   RN_FP32_SPLIT3  (round 5) each operand, scaled by a power of two so that its tensor's largest magnitude lands in [2^14, 2^15), is
 *                   split into TWO fp16 terms hi + lo (22 significand bits + a sign: |error| <= 2^-22 |x| for elements down to 2^-18
 *                   of the tensor's maximum, an absolute 2^-40 of the maximum below that) and a product is hi*hi + hi*lo + lo*hi
 *                   on v_mfma_f32_16x16x32_f16 / 32x32x16_f16: THREE MFMAs instead of six (csrc/mfma_split.h, second half).  Weight
 *                   scales per output channel (rn_split_weights_f16), activation / gradient scales per tensor from amax words
 *                   (rn_conv_desc.x_amax).  (The split-K form stays on the fp32 MFMA in every mode.)
 * Process-wide; initial value from the environment variable RN_FP32_MFMA = native | split | split3, else RN_FP32_DEFAULT. */
#define RN_FP32_NATIVE 0
#define RN_FP32_SPLIT 1
#define RN_FP32_SPLIT3 2
#define RN_FP32_DEFAULT RN_FP32_SPLIT3
int rn_get_fp32_mfma(void);
int rn_set_fp32_mfma(int mode);
/* Process-wide run-time options; initial value from the environment variable named (read ONCE, at the option's first use --
 * never on a launch path), else the default.  rn_set_option returns RN_EINVAL for a value outside the option's range.
 *   RN_OPT_SPLITK         (RN_SPLITK, 0/1, default 1)  rn_conv_splitk_workspace_bytes may choose the split-K form.  Off, a
 *                         convolution's result does not depend on how many images share the launch: every output element
 *                         is one K loop in a fixed order (the batch-invariance the batch-8 parity test relies on).
 *   RN_OPT_DETERMINISTIC  (RN_DETERMINISTIC, 0/1, default 0)  weight gradients are reduced in a fixed order: every K slice of
 *                         rn_conv_wgrad* stores its partial tile in a slab of the workspace and an ordered pass adds the
 *                         slabs (and the column sums) -- two runs give bit-identical gradients, as the reference's CPU path
 *                         does; costs the slab traffic (rn_conv_wgrad_det_workspace_bytes).  Off: fp32 atomics, fastest,
 *                         last bits depend on arrival order.
 * Kernel selectors of the split-operand family (A/B switches; the defaults are the measured best):
 *   RN_OPT_MF16           (RN_MF16, 0/1, default 1)  wide layers with Cin % 32 == 0 take csrc/conv_igemm_mf16.hip (16x16x32 MFMA).
 *   RN_OPT_MF16_MIN       (RN_MF16_MIN, >= 0, default 1)  fewest tiles a launch needs to take it.
 *   RN_OPT_WGRAD_ONCE     (RN_WGRAD_ONCE, 0/1, default 1)  weight gradient's 128 x 128 tile splits its operands once per workgroup.
 *   RN_OPT_BF16_P8        (RN_BF16_P8, 0..2, default 1)  the bf16 engine's stride-1 same-size convolutions on the eight-wave 256 x 256 x 64
 *                         tile with the phased K loop (csrc/conv_bf16_p8.hip): 0 never, 1 where it measured faster, 2 wherever legal.
 *   RN_OPT_FP8_P8         (RN_FP8_P8, 0..2, default 1)  the same for the fp8 inference engine (csrc/conv_fp8_p8.hip, 256 x 256 x 128). */
#define RN_OPT_SPLITK 0
#define RN_OPT_DETERMINISTIC 1
#define RN_OPT_MF16 2
#define RN_OPT_MF16_MIN 3
#define RN_OPT_WGRAD_ONCE 4
#define RN_OPT_BF16_P8 5
#define RN_OPT_FP8_P8 6
#define RN_OPT_COUNT 7
int rn_get_option(int option);
int rn_set_option(int option, int value);
/* RN_FP32_SPLIT applies to rn_conv_igemm / _grouped launches with kh*kw*Cin >= this (64; environment RN_FP32_SPLIT_MIN_K);
 * shorter reductions keep the fp32 MFMA kernel.  (A pre-split weight operand, w_format 1, is always
 * taken by the split kernels: prepare it for the long reductions only.) */
int rn_fp32_split_min_k(void);
/* RN_FP32_SPLIT: the weights' three bf16 terms can be prepared once per optimizer step instead of in every workgroup:
 * w_split [rows][Kpad/16][3][16] bf16 (6 bytes per element of w_packed [rows][Kpad], Kpad % 16 == 0; for a batch of GEMMs
 * rows = batch * rows).  Pass it as w_packed with rn_conv_desc.w_format = 1.  (rn_prep_batched: job kind 4.) */
int rn_split_weights(const float *w_packed, void *w_split, int64_t rows, int Kpad, void *stream);
/* RN_FP32_SPLIT3's weight operand: [rows][Kpad/16] records of 64 bytes = the hi and lo fp16 terms (2 x 16) of the row's 16 values of
 * a K-step, written with the row's own power-of-two scale (largest |value| of the row -> [2^14, 2^15)); row_unscale[rows] receives
 * the inverse scales.  Pass as w_packed with rn_conv_desc.w_format = 3 and w_unscale = row_unscale.  (rn_prep_batched: job kind 5.) */
int rn_split_weights_f16(const float *w_packed, void *w_split, float *row_unscale, int64_t rows, int Kpad, void *stream);
/* The amax tables of a tensor (rn_conv_desc.x_amax) for tensors no producer left them for: x = n_images images of per_image floats,
 * amax = [n_images][256] bytes: every thread sets the byte of the exponent field of the largest |value| it read, so the highest set
 * byte of table i is the exponent field of image i's largest |value| (lower bytes: some thread's maximum); zero the tables first.
 * One pass over x. */
int rn_amax(const float *x, int64_t per_image, int n_images, void *amax, void *stream);
/* *id = the identity of the graph capture `stream` is in (hipStreamGetCaptureInfo), 0 when it is not capturing.  Host only. */
int rn_stream_capture_id(void *stream, unsigned long long *id);
/* 1 when rn_conv_igemm would run this problem on an fp16-split kernel (so: wants w_format 3, x_amax, w_unscale): in RN_FP32_SPLIT3 mode,
 * every problem (the 16x16x32 kernel for the wide layers with Cin % 32 == 0, the two-term form of the 128 x 128 / 256 x 64 tile for the
 * rest); 0 in the other modes. */
int rn_conv_igemm_wants_f16(const rn_conv_desc *d);

int rn_conv_igemm(const rn_conv_desc *d, const float *x, const float *w_packed, float *y,
                  const float *scale, const float *shift, const float *add, const float *mask, const float *add2,
                  void *stream);

/* Split-K form for problems with few output tiles and a long K loop (the P6 / P7 pyramid levels, the deep layers of
 * the 112x112 crop detector): rn_conv_splitk_workspace_bytes returns 0 when splitting is not worthwhile, otherwise the
 * scratch size; rn_conv_igemm_splitk then slices K over grid.y, each slice storing its raw partial tile in its own slab
 * (no atomics: results are reproducible), and a finish kernel adds the slabs in order and applies the same epilogue. */
int64_t rn_conv_splitk_workspace_bytes(const rn_conv_desc *d);
int rn_conv_igemm_splitk(const rn_conv_desc *d, const float *x, const float *w_packed, float *y, const float *scale,
                         const float *shift, const float *add, const float *mask, const float *add2, void *workspace,
                         void *stream);

/* Grouped launch: up to RN_MAX_GROUP problems that share the weights and every scalar of the descriptor except the
 * geometry (N, Hi, Wi, Ho, Wo, output map, batch strides) run as ONE grid -- the five pyramid levels of a head tower
 * (D/model.py:302-304 loops over them): the small levels no longer occupy a fraction of the GPU for a full
 * workgroup round each.  tile_end[i] = exclusive prefix sum of the problems' tile counts (tile = 128x128 outputs,
 * 256x64 when Cout <= 64); add2 and in_relu are not available in grouped launches (RN_EINVAL). */
#define RN_MAX_GROUP 5
typedef struct rn_conv_group {
    int n;
    int tile_end[RN_MAX_GROUP];
    rn_conv_desc d[RN_MAX_GROUP];
    const float *x[RN_MAX_GROUP];
    float *y[RN_MAX_GROUP];
    const float *add[RN_MAX_GROUP];
    const float *mask[RN_MAX_GROUP];
} rn_conv_group;
int rn_conv_igemm_grouped(const rn_conv_group *g, const float *w_packed, const float *scale, const float *shift,
                          void *stream);

/* Which kernel a launch takes, without launching it: the launchers' own decision code run up to the launch statement, in the current
 * product mode and options (tests name their cases by it; DESIGN.md 4.2 has the table of paths).  RN_EINVAL for every descriptor /
 * group the launcher refuses.  rn_conv_igemm_plan: d as the launch would pass it (w_format, x_amax, w_unscale, sign_out, y_amax and
 * row_list matter: only NULL or not is looked at, nothing is dereferenced); add, mask and add2 count as present exactly when add_mode,
 * mask_mode and add2_mode name them.  ON ENTRY out[0] holds the RN_PLAN_ASK_ bits: AFFINE = the launch passes a scale or a shift (only
 * the raw GEMM instance asks), SPLITK = report rn_conv_igemm_splitk's launch instead of rn_conv_igemm's (RN_EINVAL where
 * rn_conv_splitk_workspace_bytes is 0).  rn_conv_igemm_grouped_plan: g as rn_conv_igemm_grouped takes it (add / mask pointers NULL or not).
 * out[RN_IGEMM_PLAN_WORDS] =
 *    0 family: 0 csrc/conv_igemm.hip (fp32 MFMA), 1 conv_igemm_split.hip, 2 conv_igemm_mf16.hip, 3 conv_igemm_splitk.hip
 *    1 tile rows   2 tile columns   3 waves per workgroup
 *    4 GENERAL (the output map is honoured; split-K: of the finish kernel)   5 RELU (on load)   6 RAW (no epilogue)
 *    7 SPLIT (family 1: 1 both operands split in the loop, 2 weights pre-split, 3 activations split once per workgroup; else 0)
 *    8 TERMS (3 bf16 terms, 2 fp16 terms, 1 first bf16 term only; 0: fp32 MFMA)
 *    9 activations staged through the LDS (family 2)   10 workgroups (split-K: grid.x, the tiles)
 *   11 split-K: slices asked for   12 slices used = grid.y   13 K-steps per slice   14 finish kernel 0 dense / 1 general (-1: no split-K)
 *   15 form: 0 single launch, 1 grouped, 2 work list (rn_conv_desc.row_list) */
#define RN_IGEMM_PLAN_WORDS 16
#define RN_PLAN_ASK_AFFINE 1
#define RN_PLAN_ASK_SPLITK 2
int rn_conv_igemm_plan(const rn_conv_desc *d, int32_t *out);
int rn_conv_igemm_grouped_plan(const rn_conv_group *g, int32_t *out);

/* Weight gradient: dw[co][r][s][ci] += sum_{n,oh,ow} dy[n,oh,ow,co] * x[n, oh*st + r - pd, ow*st + s - pd, ci]
 * (fp32 atomics into a zeroed or previously accumulated [Cout][Kpad] buffer, same layout as the packed forward
 * weights; heads accumulate their five pyramid levels into one buffer).  dy: [N,Ho,Wo,Cout] with channel
 * stride ldy >= Cout (a padded copy is allowed), x: [N,Hi,Wi,Cin]; in_relu applies max(x,0) on load.
 * colsum (may be NULL): colsum[co] += sum over pixels of dy[.,co] -- the bias / batch-norm-beta gradient, fused
 * because this kernel streams dy anyway.
 * Size limit: the K range is cut into slices whose dy bytes and span of input images each stay below 2 GiB (the
 * slices are made finer if need be); RN_EINVAL only if a single input image exceeds that. */
int rn_conv_wgrad(const float *dy, int ldy, const float *x, float *dw, float *colsum, int N, int Hi, int Wi,
                  int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int in_relu, void *stream);
/* nbatch independent problems of identical shape in one launch: operands and result of entry b at dy + b*dy_bstride,
 * x + b*x_bstride, dw + b*dw_bstride (floats); colsum (if given) is taken from entry colsum_batch only. */
int rn_conv_wgrad_batched(const float *dy, int ldy, const float *x, float *dw, float *colsum, int nbatch,
                          int64_t dy_bstride, int64_t x_bstride, int64_t dw_bstride, int colsum_batch, int N, int Hi, int Wi,
                          int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int in_relu,
                          const void *dy_amax, int dy_amax_n, const void *x_amax, int x_amax_n, void *stream);
/* dy_amax / x_amax (round 5): the amax of the two operands: count > 0 = amax tables (rn_conv_desc.x_amax) of that many images;
 * count -1 = ONE plain uint32 word (an fp32 bit pattern whose exponent field bounds the tensor: a Winograd-domain tensor's, whatever the
 * batch) -- with both given, RN_FP32_SPLIT3 mode runs the fp16 two-term kernels, each operand scaled by the power of two of its LARGEST
 * exponent (the reduction runs over all images); NULL: the three-term kernels. */
/* The same reduction in a FIXED order (RN_OPT_DETERMINISTIC; the host logic selects it when the option is on): every K slice
 * stores its partial result into its own slab of `workspace` (plain stores) and one ordered pass adds slabs 0, 1, 2 ... and the
 * slices' column sums into dw / colsum: bit-identical from run to run, as the reference's CPU autograd is.  Costs one write and
 * one read of slices x the result size (measured per training step: DESIGN.md 4.2). */
int64_t rn_conv_wgrad_det_workspace_bytes(int ldy, int nbatch, int64_t dw_bstride, int N, int Hi, int Wi, int Cin, int Ho, int Wo,
                                          int Cout, int kh, int kw);
int rn_conv_wgrad_batched_det(const float *dy, int ldy, const float *x, float *dw, float *colsum, int nbatch,
                              int64_t dy_bstride, int64_t x_bstride, int64_t dw_bstride, int colsum_batch, int N, int Hi, int Wi,
                              int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int in_relu,
                              const void *dy_amax, int dy_amax_n, const void *x_amax, int x_amax_n, void *workspace, int64_t workspace_bytes,
                              void *stream);
/* The batched 1x1 reductions of a SPARSE gradient (the Winograd weight gradient of the regression tower): k_active holds one byte per
 * pixel row of dy (N = Hi = Ho = 1, Wi = Wo pixels, 1x1, stride 1, no padding; 16-byte aligned, readable up to the next multiple of
 * 16), 0 = that row of dy is zero in every batch entry.  A K slice runs only the 16-row K-steps that hold an active row, in their
 * order; a slice without one adds nothing (fixed-order form: its slab is zero).  Skipped rows of dy and x are never read.  The result
 * equals the dense call's (the fixed-order form bit for bit, up to the sign of a zero).  workspace NULL: fp32 atomics
 * (rn_conv_wgrad_batched); else the fixed-order form (rn_conv_wgrad_batched_det).  RN_EINVAL where the flags cannot be honoured: another
 * geometry, the native product mode, a tile shape other than 128 x 128, more than 2040 K-steps per slice. */
int rn_conv_wgrad_batched_flags(const float *dy, int ldy, const float *x, float *dw, float *colsum, int nbatch,
                                int64_t dy_bstride, int64_t x_bstride, int64_t dw_bstride, int colsum_batch, int N, int Hi, int Wi,
                                int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int in_relu,
                                const void *dy_amax, int dy_amax_n, const void *x_amax, int x_amax_n, const void *k_active,
                                void *workspace, int64_t workspace_bytes, void *stream);
/* Which path the calls above would take for a problem in the current product mode and options -- nothing is launched (host code).  The
 * geometry arguments of rn_conv_wgrad_batched; have_amax: both amax operands given; have_flags: the rn_conv_wgrad_batched_flags form;
 * det: a fixed-order form.  out[0] tile shape (0: 64 x 256, 1: 256 x 64, 2: 128 x 128), out[1] tiles, out[2] K slices, out[3] pixels
 * per slice, out[4] whole slices per XCD (0/1), out[5] workgroups of the grid, out[6] kernel (0: per-wave operands, 1: operands split
 * once per workgroup), out[7] arithmetic (0: fp32 MFMA, 1: three bf16 terms, 2: two fp16 terms).  RN_EINVAL where the call would be. */
int rn_conv_wgrad_plan(int ldy, int nbatch, int64_t dy_bstride, int64_t x_bstride, int64_t dw_bstride, int colsum_batch, int N, int Hi,
                       int Wi, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int in_relu, int have_amax,
                       int have_flags, int det, int32_t *out);
/* Data AND weight gradient of a 1x1 stride-1 pad-0 convolution in one pass over dy (csrc/conv_bwd_1x1.hip; RN_FP32_SPLIT3 only).  Built
 * for Cin = 64, Cout = 256: dy [N,H,W,256], x [N,H,W,64] and dx [N,H,W,64] dense fp32, 16-byte aligned.
 *   dx = mask * (dy . w)   with w_split / w_unscale the layer's pre-split data-gradient weights (rn_split_weights_f16 of the packed
 *        [64][256] tensor: rn_conv_desc.w_format 3); stored once.  mask_mode 0: none (mask NULL); 1: mask = fp32 [N,H,W,64], elements
 *        > 0 pass (rn_conv_igemm's mask of a ReLU output); 2: mask = the sign bits of such a tensor (RN_MASK_BITS layout).  sign_out,
 *        if not NULL, receives dx's sign bits; dx_amax, if not NULL, its amax tables (one per image).
 *   dw [256][64] += dy^T x,  colsum [256] += column sums of dy (NULL: not wanted): fp32 atomics into zeroed accumulators, as
 *        rn_conv_wgrad_batched -- same layout, so rn_unpack_batched reads them unchanged.
 * dy_amax / x_amax: the operands' amax tables (one per image, both required).  Both products split the operands with the scale of the
 * pixel's IMAGE (rn_conv_igemm's rule), so an image's dx does not depend on the rest of the batch.  RN_EINVAL for what is not built:
 * other channel counts, stride != 1, an addend (add != NULL), another product mode, RN_OPT_DETERMINISTIC (no fixed-order form). */
int rn_conv_bwd_1x1(const float *dy, const float *x, const void *w_split, const float *w_unscale, float *dx, float *dw, float *colsum,
                    const void *mask, int mask_mode, const float *add, void *sign_out, const void *dy_amax, const void *x_amax,
                    void *dx_amax, int N, int H, int W, int Cin, int Cout, int stride, void *stream);

/* ---------------------------------------------------------------- bf16 convolution engine -----------------
 * The reduced-precision form of rn_conv_igemm / rn_conv_wgrad for BASELINE configs[2] (bf16 MFMA,
 * v_mfma_f32_32x32x16_bf16): activations, addend, mask and packed weights are bf16 (IEEE bfloat16, 2 bytes; NHWC /
 * [Cout][kh][kw][Cin] rows padded to a multiple of 32 ELEMENTS -- rn_pack_weights' fp32 output cast by rn_f32_to_bf16),
 * accumulation and the epilogue (scale, shift, mask, addend, activation: as rn_conv_igemm) are fp32, the result is rounded
 * once: to bf16, or stored as fp32 when y_is_f32 != 0 (head outputs that feed the loss).  Same rn_conv_desc, with strides
 * counted in elements; Cin % 8 == 0, Cout % 8 == 0 for a bf16 result (% 4 for an fp32 one); in_relu, add2 and w_batch_stride
 * are not available (RN_EINVAL).  x, w_packed, y 16-byte aligned; add, mask 16-byte aligned (8 beside an fp32 result).  Replaces the same nn.Conv2d call sites as rn_conv_igemm
 * (D/model.py:59-205, D/utils.py:12-80) when the caller opts into bf16 storage; the reference itself is fp32. */
int rn_f32_to_bf16(const float *src, void *dst, int64_t n, void *stream);   /* round-to-nearest-even, NaN stays NaN */
int rn_bf16_to_f32(const void *src, float *dst, int64_t n, void *stream);
int rn_conv_igemm_bf16(const rn_conv_desc *d, const void *x, const void *w_packed, void *y, int y_is_f32,
                       const float *scale, const float *shift, const void *add, const void *mask, void *stream);
/* Grouped form (see rn_conv_igemm_grouped): the pointers of rn_conv_group are bf16 (x, add, mask) / bf16 or fp32 (y). */
int rn_conv_igemm_bf16_grouped(const rn_conv_group *g, const void *w_packed, int y_is_f32, const float *scale,
                               const float *shift, void *stream);
/* Tile shape the grouped bf16 launcher uses for this group, as rows * 1000 + cols (128128, 256128 or 256256) --
 * tile_end[i] = running sum of ceil(N*Ho*Wo / rows) * ceil(Cout / cols).  (tile_end is ignored on input by this query;
 * d[], the pointers and n must be filled.) */
int rn_conv_igemm_bf16_tile_rows(const rn_conv_group *g, int y_is_f32);
/* ---------------------------------------------------------------- fp8 forward (BASELINE configs[4], first cut) -----------
 * The convolutions of the detector's forward pass with e4m3fn (OCP) weights and activations on v_mfma_scale_f32_32x32x64_f8f6f4
 * (all block scales 2^0; fp32 accumulation): every nn.Conv2d behind the fp32 stem with its fused batch-norm / bias / residual /
 * ReLU / sigmoid / FPN upsample-add epilogue (D/model.py:59-205, D/utils.py:12-80).  Inference only: no data or weight gradient.
 *   rn_fp8_quantize / _dequantize   fp32 <-> e4m3 with one scale per tensor: q = fp8(x * inv_scale) (saturating at +-448), x = q * scale;
 *   rn_fp8_quantize_rows            packed fp32 weight rows [rows][Kpad] -> e4m3 rows [rows][round64(Kpad)] + row_scale[rows]
 *                                   (= max|row| / 448): the per-output-channel weight scale;
 *   rn_conv_igemm_fp8               rn_conv_desc geometry as rn_conv_igemm (no mask, no input ReLU, no add2, Cin % 16 == 0):
 *                                   y = act(acc * scale[c] + shift[c] + add_q * add_scale), the caller folding
 *                                   x_scale * row_scale[c] * bn_scale[c] into scale[c]; stored as e4m3(y * out_inv_scale)
 *                                   (Cout % 16 == 0) or as fp32 (y_is_f32: head outputs). */
int rn_fp8_quantize(const float *src, void *dst, int64_t n, float inv_scale, void *stream);
/* The 3x3 / stride 2 / pad 1 max-pool of an fp32 NHWC tensor written as e4m3 with one scale (y = fp8(max * inv_scale)): max-pool followed by
 * rn_fp8_quantize, bit for bit, in one pass (the fp8 engine's stem boundary). */
int rn_maxpool_fwd_fp8out(const float *x, void *y, int N, int H, int W, int C, int Ho, int Wo, float inv_scale, void *stream);
int rn_fp8_dequantize(const void *src, float *dst, int64_t n, float scale, void *stream);
/* e4m3 -> bf16: dst[i] = bf16(q[i] * scale), n a multiple of 16, both pointers 16-byte aligned.  The fp8-forward training step (round 5:
 * BASELINE configs[4] as a TRAINING configuration) saves its activations as e4m3 and runs its data / weight gradients on the bf16
 * kernels (rn_conv_igemm_bf16, rn_conv_wgrad_bf16): this is the hand-over. */
int rn_fp8_to_bf16(const void *src, void *dst, int64_t n, float scale, void *stream);
/* bf16 -> e4m3 with one scale: dst[i] = fp8(src[i] * inv_scale), saturating at +-448; n a multiple of 16, pointers 16-byte aligned.  The
 * fp8 engine's bf16 residual stream (the last convolution of every bottleneck, the shortcuts and the FPN run in bf16 by default since
 * round 5: profiles/r05_fp8_error_budget.txt) enters the next e4m3 convolution through this. */
int rn_bf16_to_fp8(const void *src, void *dst, int64_t n, float inv_scale, void *stream);
int rn_fp8_quantize_rows(const float *w_packed, void *w_q, float *row_scale, int64_t rows, int Kpad, void *stream);
int rn_conv_igemm_fp8(const rn_conv_desc *d, const void *x_q, const void *w_q, void *y, int y_is_f32, const float *scale,
                      const float *shift, const void *add_q, float add_scale, float out_inv_scale, void *stream);
/* The pyramid levels of a head layer as one launch (rn_conv_igemm_grouped's form; the group's x / y / add are e4m3 -- y: or fp32 --
 * behind the float-typed fields, one input scale for the whole group folded into scale[c]).  tile_end[i] = running sum of
 * ceil(N*Ho*Wo / rows) * ceil(Cout / cols) with the tile rn_conv_igemm_fp8_tile_rows reports for the group (rows * 1000 + cols:
 * 128128, or 256256 where RN_OPT_FP8_P8 selects csrc/conv_fp8_p8.hip). */
int rn_conv_igemm_fp8_tile_rows(const rn_conv_group *g, int y_is_f32);
/* The tile a SINGLE launch takes for this problem (profiling and tests): rows * 1000 + cols; rn_conv_igemm_bf16_tile adds 1 000 000 when
 * the eight-wave phased kernel (csrc/conv_bf16_p8.hip) runs; for fp8, 256256 is csrc/conv_fp8_p8.hip. */
int rn_conv_igemm_fp8_tile(const rn_conv_desc *d, int y_is_f32);
int rn_conv_igemm_bf16_tile(const rn_conv_desc *d, int y_is_f32);
int rn_conv_igemm_fp8_grouped(const rn_conv_group *g, const void *w_q, int y_is_f32, const float *scale, const float *shift,
                              float add_scale, float out_inv_scale, void *stream);

/* dw[co][r][s][ci] (fp32, packed [Cout][Kpad] like rn_conv_wgrad, atomically accumulated) from bf16 dy [N,Ho,Wo,ldy>=Cout]
 * and bf16 x [N,Hi,Wi,Cin]; colsum (may be NULL) += column sums of dy.  Cin % 8 == 0, ldy % 8 == 0. */
int rn_conv_wgrad_bf16(const void *dy, int ldy, const void *x, float *dw, float *colsum, int N, int Hi, int Wi, int Cin,
                       int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, void *stream);
/* The same for n <= RN_MAX_GROUP problems that share ONE weight tensor -- the pyramid levels of a head layer (D/model.py:110-205), whose
 * weight gradient is the sum over the levels -- as one launch: dy[i] [N, Ho_i, Wo_i, ldy], x[i] [N, Hi[i], Wi[i], Cin]; dw / colsum
 * accumulate the sum.  The small levels, launches of tens of microseconds on their own, ride along with the big ones. */
int rn_conv_wgrad_bf16_grouped(int n, const void *const *dy, int ldy, const void *const *x, float *dw, float *colsum, int N,
                               const int *Hi, const int *Wi, int Cin, int Cout, int kh, int kw, int stride, int pad, void *stream);

/* Non-convolution steps of the schedule with bf16 activations (elementwise_bf16.hip): the same operations as
 * rn_maxpool_fwd / rn_maxpool_bwd / rn_upsample_add_bwd / rn_sigmoid_bwd_pad with bf16 storage on the activation side.
 * The stem stays fp32, so pooling is the boundary: forward reads the fp32 stem output and writes bf16 (+ uint8 argmax),
 * backward reads the bf16 gradient and writes the fp32 gradient of the stem output (masked by the stem's ReLU). */
int rn_maxpool_fwd_bf16out(const float *x, void *y, uint8_t *argmax, int N, int H, int W, int C, int Ho, int Wo, void *stream);
int rn_maxpool_bwd_bf16in(const float *x, const void *dy, const uint8_t *argmax, float *dx, int N, int H, int W, int C, int Ho,
                          int Wo, int relu_mask, void *stream);
int rn_upsample_add_bwd_bf16(const void *src, void *dst, int N, int Hs, int Ws, int Hd, int Wd, int C, void *stream);
int rn_sigmoid_bwd_pad_bf16(const float *dy, const float *s, void *out, int B, int64_t rows_per_image, int C, int ld,
                            int64_t src_batch_stride, void *stream);
int rn_relu_bf16(const void *src, void *dst, int64_t n, void *stream);      /* n % 4 == 0 */

/* Winograd F(4x4,3x3) stages for 3x3 / stride 1 / padding 1 convolutions (the head towers, D/model.py:120-205), fp32:
 *   rn_wino_input   x [N,H,W,C] -> V [36][Tpad][C]: B^T d B of every 6x6 patch; the problem's tiles (N * ceil(H/4) *
 *                   ceil(W/4), image-major) are written from row tile_offset on, so several problems (pyramid levels)
 *                   share one V;
 *   (GEMM)          rn_conv_igemm as a 1x1 convolution over 36 images of Tpad pixels with w_batch_stride = rows * Kpad:
 *                   M [36][Tpad][Cout] = V_p x U_p^T;
 *   rn_wino_output  M -> y [N,H,W,Cout]: A^T m A, then v = scale*v + shift; mask_mode 1: v = mask > 0 ? v : 0;
 *                   v += add; act 1: ReLU, 2: sigmoid; mask_mode 2: v = mask > 0 ? v : 0  (mask / add: dense geometry of
 *                   y, may be NULL); y_batch_stride (floats, 0 = dense) lets a head write into its slice of [B, A, n];
 *   rn_wino_weights U [36][rows][Kpad] from the OIHW parameter: mode 0 forward (rows = Cout, K = Cin), mode 1 data
 *                   gradient (rows = Cin, K = Cout, filter rotated by 180 degrees, times scale[co]); Kpad = K rounded up to 32.
 * Accuracy: ~1e-5 of the output's max magnitude (the direct kernel: ~3e-7). */
/* Grouped forms: up to RN_MAX_GROUP problems (the pyramid levels of a head layer) in one launch; their tiles are
 * concatenated in V / M / Z in table order starting at row tile_offset.  src: x or dy per problem (input transforms,
 * dy_form = 1 for A dy A^T); dst / add / mask: per problem for the output transform (add, mask may be NULL). */
typedef struct rn_wino_group {
    int n;
    int N[RN_MAX_GROUP], H[RN_MAX_GROUP], W[RN_MAX_GROUP];
    const float *src[RN_MAX_GROUP];
    float *dst[RN_MAX_GROUP];
    const float *add[RN_MAX_GROUP];
    const float *mask[RN_MAX_GROUP];       /* rn_wino_output_group: fp32, or sign-bit words with mask_mode | RN_MASK_BITS */
    void *sign[RN_MAX_GROUP];              /* rn_wino_output_group: NULL or the words that receive the result's sign bits (rn_conv_desc.sign_out) */
    void *amax[RN_MAX_GROUP];              /* RN_FP32_SPLIT3: NULL, or amax words, one per image [N] -- of src for the input transforms (read:
                                              rn_conv_desc.x_amax of the untransformed tensor), of dst for rn_wino_output_group (raised:
                                              rn_conv_desc.y_amax) */
} rn_wino_group;
/* row_amax / tensor_amax (round 5, RN_FP32_SPLIT3; NULL otherwise): the amax words of the TRANSFORMED tensor, derived from the sources'
 * per-image words by the transform's gain bound (2^7 for B^T d B, 2^8 for A dy A^T; csrc/conv_wino.hip) without a reduction:
 * row_amax[tile_offset + t] = the word of tile row t (its image's) -- the Winograd-stage GEMM's rn_conv_desc.x_amax with strides (0, 1);
 * *tensor_amax = max(*tensor_amax, the largest of them) -- the weight gradient's single word (zero it before the first launch). */
int rn_wino_input_group(const rn_wino_group *g, float *V, int C, int64_t tile_offset, int64_t Tpad, int dy_form,
                        void *row_amax, void *tensor_amax, void *stream);
/* Both input-side transforms of an output gradient in one pass over it: V = B^T dy B (rn_wino_input_group, dy_form 0: what the
 * data gradient's GEMM reads) and Z = A dy A^T (dy_form 1: what the weight gradient's reads). */
int rn_wino_input_both_group(const rn_wino_group *g, float *V, float *Z, int C, int64_t tile_offset, int64_t Tpad,
                             void *v_row_amax, void *z_tensor_amax, void *stream);
int rn_wino_output_group(const rn_wino_group *g, const float *M, int Cout, int64_t tile_offset, int64_t Tpad,
                         const float *scale, const float *shift, int mask_mode, int act, int64_t y_batch_stride, void *stream);
/* The same two with TILE ACTIVITY FLAGS: one byte per tile row of V / Z / M ([Tpad], 16-byte aligned, zeroed by the
 * caller, set by the producers of the gradient), 1 = some pixel of the tile's 6x6 patch may be non-zero.
 *   rn_wino_input_both_group_flags: a tile with flag 0 loads nothing and writes no V; its rows of Z are zeroed where the 16-row unit
 *       they lie in holds an active tile (what a reduction that skips whole inactive units reads).  flags NULL: the dense form.
 *   rn_wino_output_group_flags: a tile with flags_in 0 reads no M and runs the epilogue on zeros (the result is dense); flags_out receives
 *       the flags of the STORED tensors, in the same tile order, for the next layer.  Either may be NULL. */
int rn_wino_input_both_group_flags(const rn_wino_group *g, float *V, float *Z, int C, int64_t tile_offset, int64_t Tpad,
                                   void *v_row_amax, void *z_tensor_amax, const void *flags, void *stream);
int rn_wino_output_group_flags(const rn_wino_group *g, const float *M, int Cout, int64_t tile_offset, int64_t Tpad,
                               const float *scale, const float *shift, int mask_mode, int act, int64_t y_batch_stride,
                               const void *flags_in, void *flags_out, void *stream);
/* WORK LISTS of one flag array (Tpad bytes, a multiple of 256 and at most 32 768, 16-byte aligned), built on the device by one workgroup and never read by
 * the host: tiles = the rows with a non-zero flag, units = the aligned 16-row units and blocks = the 128-row blocks that hold one, each
 * ascending int32 (room for Tpad, Tpad / 16 and Tpad / 128 entries; entries past the count keep what they held), counts[0..2] = their
 * lengths.  Stages that take a list visit nothing else, so an inactive tile costs nothing:
 *   rn_wino_input_both_group_lists: what rn_wino_input_both_group_flags stores, thread -> entry of `units` -> tile; row words of V are
 *       written for the listed units only, the caller zeroes the others.
 *   rn_conv_desc.row_list / row_list_n (= blocks, counts + 2): the Winograd-stage GEMM. */
int rn_tile_lists(const void *flags, int64_t Tpad, void *counts, void *tiles, void *units, void *blocks, void *stream);
int rn_wino_input_both_group_lists(const rn_wino_group *g, float *V, float *Z, int C, int64_t tile_offset, int64_t Tpad,
                                   void *v_row_amax, void *z_tensor_amax, const void *flags, const void *units, const void *n_units,
                                   void *stream);
/* The FORWARD of a layer whose output is needed on a known set of tiles only (rn_reg_need_tiles), over the work lists of that set's flags:
 *   rn_wino_input_group_list: thread -> entry of `units` -> tile.  A flagged tile gets what rn_wino_input_group stores (bit for bit) and its
 *       row word; the other tiles of a listed 16-row unit get ZERO rows (the weight gradient reads whole units of a kept V); nothing else
 *       is visited.  The caller zeroes the row words.  tensor_amax as rn_wino_input_group.
 *   rn_wino_output_group_list: thread -> entry of `tiles` (n_tiles = counts) -> tile.  A listed tile gets what rn_wino_output_group stores
 *       (result, sign bits, amax table); every other tile is neither read nor written. */
int rn_wino_input_group_list(const rn_wino_group *g, float *V, int C, int64_t tile_offset, int64_t Tpad, void *row_amax,
                             void *tensor_amax, const void *flags, const void *units, const void *n_units, void *stream);
int rn_wino_output_group_list(const rn_wino_group *g, const float *M, int Cout, int64_t tile_offset, int64_t Tpad,
                              const float *scale, const float *shift, int mask_mode, int act, int64_t y_batch_stride,
                              const void *tiles, const void *n_tiles, void *stream);
int rn_wino_input(const float *x, float *V, int N, int H, int W, int C, int64_t tile_offset, int64_t Tpad, void *stream);
int rn_wino_output(const float *M, float *y, int N, int H, int W, int Cout, int64_t tile_offset, int64_t Tpad,
                   const float *scale, const float *shift, const float *add, const float *mask, int mask_mode, int act,
                   int64_t y_batch_stride, void *stream);
int rn_wino_weights(const float *w, float *U, int Cout, int Cin, int mode, const float *scale, void *stream);
/* Weight gradient of the same convolutions:  dL/dg = G^T [ sum over tiles (A dy A^T) .* (B^T d B) ] G.
 *   rn_wino_dy   dy [N,H,W,C] -> Z [36][Tpad][C] (A dy A^T of every 4x4 tile; same tile order as rn_wino_input);
 *   (GEMM)       rn_conv_wgrad_batched over the 36 positions: dU[p] += Z_p^T V_p, a 1x1 problem with Tpad-strided
 *                operands and T "pixels"; colsum of batch entry 7 (position (1,1)) is the bias gradient;
 *   rn_wino_dw   dw[co][(r*3+s)*Cin + ci] += (G^T dU G)[r][s]  (the packed layout rn_conv_wgrad accumulates into,
 *                dU [36][Cout][Cin rounded up to 32]). */
int rn_wino_dy(const float *dy, float *Z, int N, int H, int W, int C, int64_t tile_offset, int64_t Tpad, void *stream);
int rn_wino_dw(const float *dU, float *dw, int Cout, int Cin, void *stream);

/* Batched per-step preparation: batch-norm folding (kind 0: bn_scale = gamma / sqrt(var + eps), bn_shift = beta - mean *
 * bn_scale, bn_rstd), weight packing (kind 1: the arguments of rn_pack_weights, rows / Kpad as it derives them) and
 * Winograd weight transforms (kind 2: the arguments of rn_wino_weights, dst [36][rows][Kpad]) and bf16 copies of packed
 * buffers (kind 3: rows * Kpad floats at src -> bf16 at dst; a launch AFTER the one that packs src), the pre-split forms of packed buffers
 * (kind 4: rn_split_weights, 8 values per thread; kind 5: rn_split_weights_f16, chunk = 4 rows, inverse row scales to bn_scale; both AFTER
 * the launch that packs src) for many layers in one launch.  jobs_dev: device array of rn_prep_job; chunks_dev: device array of nchunks (job index,
 * 256-element block inside the job) pairs.  Jobs of one launch must not depend on each other: the data-gradient packs
 * (which read bn_scale) go in a second launch. */
typedef struct rn_prep_job {
    int kind;
    int Cout, Cin, kh, kw, kw_pad, c_pad, mode, r0, nr, s0, ns, rows, Kpad;
    float eps;
    const float *src;
    float *dst;
    const float *scale;
    const float *gamma, *beta, *mean, *var;
    float *bn_scale, *bn_shift, *bn_rstd;
} rn_prep_job;
int rn_prep_batched(const rn_prep_job *jobs_dev, const int32_t *chunks_dev, int nchunks, void *stream);

/* Weight packing.  src is the reference's OIHW parameter [Cout][Cin][kh][kw] (state_dict layout).
 *   mode 0 (forward):  dst[co][r][s][ci]          = src[co][ci][r][s]
 *   mode 1 (dgrad):    dst[ci][r][s][co]          = src[co][ci][r][s] * scale[co]   (scale NULL = 1)
 *   mode 2 (dgrad, tap subset): as mode 1 but only taps r = r0 + 2*i (i < nr), s = s0 + 2*j (j < ns) are
 *                      packed, as an nr x ns filter: one output-parity class of a stride-2 data gradient
 * kw_pad >= kw and cin_pad >= Cin (forward) / cout_pad >= Cout (dgrad) give zero-filled padding of the tap and
 * channel dimensions (stem: 7x7x3 -> 7x8x4); rows are Kpad = roundup(kh*kw_pad*c_pad, 32) floats.
 * rn_unpack_wgrad converts an accumulated dw[Cout][Kpad] back to OIHW and applies the folded batch-norm:
 *   dweight[co][ci][r][s] = scale[co] * dw[co][r][s][ci]
 *   dgamma[co] = (sum_k w[co][k]*dw[co][k] - mean[co]*colsum[co]) * rstd[co],  dbeta[co] = colsum[co]
 * (any of dgamma/dbeta/scale may be NULL). */
int rn_pack_weights(const float *src, float *dst, int Cout, int Cin, int kh, int kw, int kw_pad, int c_pad,
                    int mode, const float *scale, int r0, int nr, int s0, int ns, void *stream);
int rn_unpack_wgrad(const float *dw, const float *w_packed, float *dweight, int Cout, int Cin, int kh, int kw,
                    int kw_pad, int c_pad, const float *scale, const float *mean, const float *rstd,
                    const float *colsum, float *dgamma, float *dbeta, void *stream);

/* rn_unpack_wgrad for many layers in one launch.  jobs_dev: device array of rn_unpack_job (the arguments of rn_unpack_wgrad; Kpad
 * = roundup(kh*kw_pad*c_pad, 32)); chunks_dev: device array of nchunks (job index, output channel) pairs -- every output
 * channel of every job exactly once.  The engine issues one per all-reduce bucket (or one per backward pass). */
typedef struct rn_unpack_job {
    const float *dw, *w_packed;
    float *dweight;
    int Cout, Cin, kh, kw, kw_pad, c_pad, Kpad;
    const float *scale, *mean, *rstd, *colsum;
    float *dgamma, *dbeta;
} rn_unpack_job;
int rn_unpack_batched(const rn_unpack_job *jobs_dev, const int32_t *chunks_dev, int nchunks, void *stream);

/* Frozen batch-norm folding (eval-mode BatchNorm2d, eps 1e-5, D/model.py:278-282):
 *   scale = gamma / sqrt(var + eps), shift = beta - mean*scale, rstd = 1/sqrt(var + eps). */
int rn_bn_fold(const float *gamma, const float *beta, const float *mean, const float *var, float eps, int C,
               float *scale, float *shift, float *rstd, void *stream);

/* Elementwise / data-movement kernels around the convolutions (all NHWC fp32):
 *   rn_nchw_to_nhwc4:   image [N,3,H,W] -> [N,H,W,4] (4th channel 0) for the stem's 16-byte loads
 *   rn_maxpool_fwd/bwd: MaxPool2d(3, stride 2, pad 1) (D/model.py:216); fwd also records (argmax may be NULL) the
 *                       window position 3*r+s of the FIRST maximum, bwd routes dy there (torch semantics) and
 *                       applies the stem ReLU mask (x > 0)
 *   rn_colsum:          out[c] (+)= sum over rows of g[rows, ld] (bias / beta gradients), deterministic two-pass;
 *                       accumulate != 0 adds to out (shared heads sum their five pyramid levels)
 *   rn_upsample_add_bwd: dst[n,h,w,c] += sum_{dy,dx<2} src[n,2h+dy,2w+dx,c] within src bounds (FPN top-down bwd)
 *   rn_relu_mask:       g = (z > 0) ? g : 0 in place
 *   rn_maxpool_bwd:     relu_mask 1: the gradient is also masked by x > 0 (x = the pooled tensor, a ReLU output); 2: the same with
 *                       x pointing to that tensor's SIGN BITS (rn_conv_desc.sign_out) instead of the tensor (C % 32 == 0)
 *   rn_sigmoid_bwd_pad: out[b][p][c<C] = dy[b][p][c] * s[b][p][c]*(1-s[b][p][c]) (s = sigmoid output, NULL =
 *                       identity), out[..][C..ld) = 0: a head-output gradient slice (rows_per_image rows per
 *                       image, images src_batch_stride floats apart in dy and s) copied to a dense, channel-
 *                       padded [B*rows_per_image, ld] matrix the GEMMs accept
 *   rn_add_inplace:     dst += src
 */
int rn_nchw_to_nhwc4(const float *src, float *dst, int N, int H, int W, void *amax, void *stream);
int rn_maxpool_fwd(const float *x, float *y, uint8_t *argmax, int N, int H, int W, int C, int Ho, int Wo, void *stream);
int rn_maxpool_bwd(const float *x, const float *dy, const uint8_t *argmax, float *dx, int N, int H, int W, int C,
                   int Ho, int Wo, int relu_mask, void *amax, void *stream);
int rn_colsum(const float *g, int64_t rows, int C, int ld, float *out, int accumulate, void *workspace, void *stream);
int64_t rn_colsum_workspace_bytes(int64_t rows, int C);
int rn_upsample_add_bwd(const float *src, float *dst, int N, int Hs, int Ws, int Hd, int Wd, int C, void *amax, void *stream);
int rn_relu_mask(float *g, const float *z, int64_t n, void *stream);
int rn_sigmoid_bwd_pad(const float *dy, const float *s, float *out, int B, int64_t rows_per_image, int C, int ld,
                       int64_t src_batch_stride, void *amax, void *stream);
/* rn_sigmoid_bwd_pad for images of H x W pixels that also sets the tile activity flags of its result (one byte per 4x4 tile of the
 * B images, zeroed by the caller): a non-zero value sets its tile and the neighbours whose 6x6 patch contains its pixel. */
int rn_sigmoid_bwd_pad_flags(const float *dy, const float *s, float *out, int B, int H, int W, int C, int ld,
                             int64_t src_batch_stride, void *amax, void *flags, void *stream);
int rn_add_inplace(float *dst, const float *src, int64_t n, int64_t per_image, void *amax, void *stream);
/* `amax` of rn_nchw_to_nhwc4 / rn_maxpool_bwd / rn_upsample_add_bwd / rn_sigmoid_bwd_pad / rn_add_inplace (round 5): NULL, or the amax
 * words of the tensor the call produces, one per image (rn_conv_desc.y_amax: raised by atomic max; the caller zeroes them first).
 * rn_add_inplace: image of element i = i / per_image. */

/* ---------------------------------------------------------------- optimizer step ---------------------------
 * clip_grad_norm_(params, max_norm) + Adam(lr, betas, eps).step() of the reference trainer
 * (train_detector_3D_angle.py:337, 385-387) over every parameter tensor in two launches, no host sync.
 *   tensor_table: device array of n_tensors entries {float *p, *g, *m, *v; int64_t n}
 *   chunk_table:  device array of n_chunks entries {int tensor; int chunk_in_tensor}, 4096 elements per chunk
 *   step: 1-based Adam step count (bias correction); max_norm <= 0 disables clipping
 *   total_norm: device float, receives the pre-clip global L2 norm; write_clipped != 0 stores g*coef back
 */
int64_t rn_opt_workspace_bytes(int n_chunks);
int rn_opt_clip_adam(const void *tensor_table, const void *chunk_table, int n_chunks, float max_norm, float lr,
                     float beta1, float beta2, float eps, int step, int write_clipped, void *workspace,
                     float *total_norm, void *stream);
/* The same step with the step number on the device: *step_dev (int32, start at 0) is incremented, then used for the bias
 * corrections.  No argument changes between steps: the launch sequence can be captured into a hipGraph and replayed. */
int rn_opt_clip_adam_dev(const void *tensor_table, const void *chunk_table, int n_chunks, float max_norm, float lr,
                         float beta1, float beta2, float eps, int *step_dev, int write_clipped, void *workspace,
                         float *total_norm, void *stream);
/* The same step with the hyper-parameters on the device as well: hp = six floats [lr, max_norm, beta1, beta2, eps, grad_scale].
 * A scheduler's new lr (ReduceLROnPlateau, train_detector_3D_angle.py:338, 412) reaches a replayed hipGraph because the caller
 * rewrites hp outside the graph.  grad_scale multiplies every gradient before the norm and the update (1/world for a
 * data-parallel gradient SUM, so no separate pass scales the gradient buffer); max_norm <= 0 disables the clip. */
int rn_opt_clip_adam_hp(const void *tensor_table, const void *chunk_table, int n_chunks, const float *hp, int *step_dev,
                        int write_clipped, void *workspace, float *total_norm, void *stream);

/* ---------------------------------------------------------------- tracking evaluation (MOT metrics) --------
 * MOT_Evaluator.evaluate (mot_evaluator.py:120-412) over all frames of a sequence at once.  The host packs the frames in
 * increasing order into flat arrays: gt_off / pr_off int32 [F+1] (objects of frame f; 0 objects = the frame is missing on
 * that side), iou_off int64 [F+1] (prefix sum of n_gt * n_pred), slot_off int32 [F+1] (prefix sum of min(n_gt, n_pred): one
 * slot per assigned pair).  Ids and classes are dense int32 indices (class -1 = not in class_dict).  No synchronisation.
 *   rn_mot_prepare        replaces :155-179 and :182-195 and the footprints of :201-215.  gt_im fp64 [G,8,2], gt_h0 fp32 [G]
 *                         (guess_heights), gt_vel fp32 [G], pred_state fp32 [M,7], H fp64 [9], P fp64 [12] ->
 *                         gt_state fp32 [G,7], gt_box / pred_box fp32 [G,4] / [M,4] (xmin ymin xmax ymax), pred_im fp64 [M,8,2]
 *   rn_mot_iou            replaces the double loop over self.iou (:87-118, 219-222): fp32 arithmetic, fp64 matrix.
 *                         max_cells = the largest n_gt * n_pred of a frame
 *   rn_mot_assign         replaces linear_sum_assignment(ious, maximize=True) (:225) for every frame: slot_row / slot_col
 *                         int32 [S] (ground-truth row ascending, -1 = no pair), pred_assigned uint8 [M], frame_status int32
 *                         [F]: RN_MOT_OK, RN_MOT_INVALID (a NaN or +inf IoU), RN_MOT_INFEASIBLE, RN_MOT_TOO_LARGE.
 *                         max_n = the largest n_gt or n_pred of a frame; above RN_MOT_MAX the call returns RN_EINVAL and
 *                         launches nothing
 *   rn_mot_frame_metrics  replaces :229-238, 283-290, 301-341 per frame: per slot the IoU, the matched ids (slot_gid /
 *                         slot_pid, -1 = below match_iou), state_err fp32 [S,7], im_bot_err / im_top_err fp64 [S], the
 *                         confusion cell uint8 [S] (10 * gt + pred); per frame the outside-the-frame count and the matches
 *   rn_mot_reduce         replaces :135-152, 294-299 and :348-397: result fp64 [RN_MOT_RESULT] =
 *                         [0..11] TP FP FN "FP edge-case" "FP @ 0.2" "FN @ 0.2" unique-gt unique-pred fragmentations
 *                         ID-switches assigned-pairs status, [12] the first frame with a status,
 *                         [16 + 3q ..] (count, sum, sum of squared deviations) of figure q = pre-threshold IoU, match IoU,
 *                         state_err columns 0..6, bottom, top -- fp64 in a fixed order (slot k to partial k % 256, the
 *                         partials in increasing order), [52..151] the confusion matrix [10,10].
 *                         n_gid / n_pid = the number of distinct ids (<= RN_MOT_MAX_IDS); workspace:
 *                         rn_mot_workspace_bytes(n_gid, n_pid) bytes. */
#define RN_MOT_MAX 512          /* objects of one frame on either side: the solver's vectors (42 B / object) stay in LDS */
#define RN_MOT_MAX_IDS 16384
#define RN_MOT_RESULT 152
#define RN_MOT_OK 0
#define RN_MOT_INVALID 1
#define RN_MOT_INFEASIBLE 2
#define RN_MOT_TOO_LARGE 3
int rn_mot_prepare(const double *gt_im, const float *gt_h0, const float *gt_vel, int64_t G, const float *pred_state,
                   int64_t M, const double *H, const double *P, float *gt_state, float *gt_box, float *pred_box,
                   double *pred_im, void *stream);
int rn_mot_iou(const float *gt_box, const float *pred_box, const int32_t *gt_off, const int32_t *pr_off,
               const int64_t *iou_off, int64_t F, int64_t max_cells, double *iou, void *stream);
int rn_mot_assign(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                  const int32_t *slot_off, int64_t F, int64_t max_n, int64_t S, int64_t M, int32_t *slot_row,
                  int32_t *slot_col, uint8_t *pred_assigned, int32_t *frame_status, void *stream);
int rn_mot_frame_metrics(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                         const int32_t *slot_off, int64_t F, int64_t S, const int32_t *slot_row, const int32_t *slot_col,
                         const int32_t *frame_status, double match_iou, const float *gt_state, const float *pred_state,
                         const double *gt_im, const double *pred_im, const int32_t *gt_cls, const int32_t *pred_cls,
                         const int32_t *gt_id, const int32_t *pred_id, const uint8_t *pred_assigned, double *slot_iou,
                         int32_t *slot_gid, int32_t *slot_pid, float *slot_state_err, double *slot_bot, double *slot_top,
                         uint8_t *slot_cls, int32_t *frame_edge, int32_t *frame_match, void *stream);
int64_t rn_mot_workspace_bytes(int64_t n_gid, int64_t n_pid);
int rn_mot_reduce(int64_t F, int64_t S, const int32_t *gt_off, const int32_t *pr_off, const int32_t *slot_off,
                  const int32_t *frame_status, const int32_t *frame_edge, const int32_t *frame_match,
                  const int32_t *slot_row, const double *slot_iou, const int32_t *slot_gid, const int32_t *slot_pid,
                  const float *slot_state_err, const double *slot_bot, const double *slot_top, const uint8_t *slot_cls,
                  const int32_t *gt_id, const int32_t *pred_id, int64_t n_gid, int64_t n_pid, void *workspace,
                  double *result, void *stream);

/* ---------------------------------------------------------------- identity and association scores (IDF1, HOTA) --------
 * Beyond the reference, whose evaluator stops at the CLEAR-MOT figures above: the identity scores of Ristani et al. (ECCV-W
 * 2016) and the HOTA family of Luiten et al. (IJCV 2021), from the same packed frames, fp64 IoU matrices (rn_mot_iou) and dense
 * ids (csrc/mot_assoc.hip states the definitions).  Every entry takes the frame layout: the four offset arrays, F, max_n (the
 * largest n_gt or n_pred of a frame; above RN_MOT_MAX -> RN_EINVAL, no launch) and the totals n_gt / n_pr (objects), cells, S
 * (slots) that the offsets are checked against on the device.  n_gid * n_pid <= RN_MOT_ASSOC_MAX_CELLS (dense id x id
 * storage), else RN_EINVAL before any launch.  No synchronisation.
 *   rn_mot_id_counts    gc int32 [n_gid] / pc int32 [n_pid]: frames holding each id; C int32 [n_gid, n_pid]: frames with
 *                       S_t[g,p] >= id_iou.  status int32 [2] = (highest code, first frame with one or -1): RN_MOT_TOO_LARGE
 *                       (a frame outside the layout), RN_MOT_DUPLICATE_ID (an id twice in one frame on one side),
 *                       RN_MOT_BAD_INDEX (an id outside the dense range; it is left out)
 *   rn_mot_id_assign    scipy's linear_sum_assignment(C, maximize=True) on one wave64: match int32 [n_gid] (the prediction id
 *                       or -1), info int64 [2] = (IDTP = sum of C over the matching, status)
 *   rn_mot_hota_align   pot fp64 [n_gid, n_pid] = sum over scored frames of S / ((colsum[p] + rowsum[g]) - S) (0 where the
 *                       denominator is <= 2^-52).  rowsum fp64 [n_gt] / colsum fp64 [n_pr] are scratch the call fills: each a
 *                       sequential ascending sum.  csr_off int32 [n_gid + 1], csr_frame / csr_row int32 [n_csr]: per
 *                       ground-truth id its (frame slot, row in the frame) over the scored frames, frames strictly ascending --
 *                       workgroup g walks them in that order and owns row g of pot, so there is no fp64 atomic and the
 *                       result is the same bits every time.  status int32 [2] as above (second word: the first id)
 *   rn_mot_hota_assign  per scored frame linear_sum_assignment(-(ga * S)) with ga = pot / ((gc + pc) - pot); score fp64 [cells]
 *                       is scratch.  Per slot (ground-truth row ascending): slot_row / slot_col (-1 = no pair), slot_s (the
 *                       pair's S), slot_n (how many of the ascending alphas fp64 [RN_MOT_ALPHAS] pass S >= alpha - 2^-52: a
 *                       prefix).  frame_status int32 [F] as rn_mot_assign, and RN_MOT_BAD_INDEX
 *   rn_mot_hota_reduce  result fp64 [RN_MOT_ASSOC_RESULT]: per alpha k seven values at [7 k]: TP FN FP (exact integers), Loc
 *                       (sum of S of the counted pairs), AssA-sum = sum M (M / max(1, gc + pc - M)), AssRe-sum (max(1, gc)),
 *                       AssPr-sum (max(1, pc)) over the cells of M_k -- each fp64 sum in one fixed order (entry e to partial
 *                       e % 256 in ascending e, the partials in increasing order); [133] status, [134] the first frame with
 *                       one (then nothing else is reported).  workspace: rn_mot_assoc_workspace_bytes(n_gid, n_pid) bytes
 *                       (0 = above a limit), shared with rn_mot_id_assign. */
#define RN_MOT_ALPHAS 19
#define RN_MOT_ASSOC_RESULT 135
#define RN_MOT_ASSOC_MAX_CELLS 1048576   /* n_gid * n_pid: 100 bytes of workspace per cell */
#define RN_MOT_DUPLICATE_ID 4
#define RN_MOT_BAD_INDEX 5
int64_t rn_mot_assoc_workspace_bytes(int64_t n_gid, int64_t n_pid);
int rn_mot_id_counts(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                     const int32_t *slot_off, int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells, int64_t S,
                     const int32_t *gt_id, const int32_t *pred_id, int64_t n_gid, int64_t n_pid, double id_iou, int32_t *gc,
                     int32_t *pc, int32_t *C, int32_t *status, void *stream);
int rn_mot_id_assign(const int32_t *C, int64_t n_gid, int64_t n_pid, void *workspace, int32_t *match, int64_t *info,
                     void *stream);
int rn_mot_hota_align(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                      const int32_t *slot_off, int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells, int64_t S,
                      const int32_t *gt_id, const int32_t *pred_id, const int32_t *csr_off, const int32_t *csr_frame,
                      const int32_t *csr_row, int64_t n_csr, int64_t n_gid, int64_t n_pid, double *rowsum, double *colsum,
                      double *pot, int32_t *status, void *stream);
int rn_mot_hota_assign(const double *iou, const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off,
                       const int32_t *slot_off, int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells, int64_t S,
                       const int32_t *gt_id, const int32_t *pred_id, int64_t n_gid, int64_t n_pid, const int32_t *gc,
                       const int32_t *pc, const double *pot, const double *alphas, double *score, int32_t *slot_row,
                       int32_t *slot_col, double *slot_s, int32_t *slot_n, int32_t *frame_status, void *stream);
int rn_mot_hota_reduce(const int32_t *gt_off, const int32_t *pr_off, const int64_t *iou_off, const int32_t *slot_off,
                       int64_t F, int64_t max_n, int64_t n_gt, int64_t n_pr, int64_t cells, int64_t S,
                       const int32_t *frame_status, const int32_t *slot_row, const int32_t *slot_col, const double *slot_s,
                       const int32_t *slot_n, const int32_t *gt_id, const int32_t *pred_id, const int32_t *gc,
                       const int32_t *pc, int64_t n_gid, int64_t n_pid, void *workspace, double *result, void *stream);

/* ---- camera calibration (csrc/calibrate.hip): the set-up half of homography.py, fp64 in the reference's order --------
 * rn_vanishing_points  replaces find_vanishing_point (homography.py:96-154) for `sets` line sets in one launch, one
 *                      workgroup per set: lines fp64 [N,4] (x0, y0, x1, y1), offsets int64 [sets+1] (CSR rows into
 *                      lines).  The start point is homography.py:113-122 as written (only lines 0 and 1 enter); 16
 *                      levels g = 1e16 .. 10; each axis is np.arange(p - 15 g, p + 15 g, g) by numpy's own rule (length
 *                      ceil((stop - start) / g), element i = start + i * ((start + g) - start)), up to RN_VP_MAX_AXIS
 *                      points; the squared line distances are added over the set's lines in order; of a level's grid
 *                      the smallest distance wins, the lowest scan index (x outer, y inner) among equals, and only if it
 *                      is below the best carried over from the levels before; NaN never wins.
 *                      out fp64 [sets,3] = (px, py, best); trace fp64 [sets,16,3] = (px, py, best) each level STARTED
 *                      with (zero-filled by the caller: levels not reached stay as they are); status int32 [sets], bits:
 *                      RN_VP_FEW_LINES (fewer than 2 lines: IndexError in the reference), RN_VP_BAD_START (start not
 *                      finite: np.arange raises there), RN_VP_LONG_AXIS (an axis longer than RN_VP_MAX_AXIS was cut),
 *                      RN_VP_BAD_OFFSETS (the set's row range is not inside the `rows` rows of lines: nothing was read).
 * rn_hg_reproj_error   replaces test_transformation's arithmetic (homography.py:581-587) for K scales of P's third column
 *                      in one launch: boxes fp64 [d,8,2], heights fp32 [d], H fp64 [3,3], P_orig fp64 [3,4], C fp64 [K];
 *                      out fp64 [K,2] = (top, bottom) mean corner distance with P[:,2] = P_orig[:,2] * C.  image ->
 *                      state is projected in fp64 and rounded to the fp32 state, state -> space is fp32, the projection
 *                      back fp64.  The means: per box ((e0 + e1) + e2) + e3, box b into partial b % 256 in ascending b,
 *                      the partials folded pairwise (t += t + s, s = 128 .. 1), divided by 4 d.
 * rn_hg_scale_z        replaces the search of scale_Z (homography.py:607-666) in one launch: np.linspace's rule (step =
 *                      (hi - lo) / 9, y[i] = i * step + lo, y[9] = hi), step_size = y[1] - y[0], while step_size >
 *                      granularity: the 10 errors (top + bottom as above), the first smallest wins, new bounds best_C -+
 *                      step_size.  trace fp64 [max_iters,10,2] = (C, error); out fp64 [3] = (the LAST C evaluated -- the
 *                      reference leaves P scaled by it, not by the best --, best C, best error of the last iteration);
 *                      info int32 [2] = (iterations, status bits: RN_SZ_BAD_FIRST_STEP the first step is not above the
 *                      granularity, RN_SZ_NO_WINNER every error of an iteration was NaN, RN_SZ_TOO_MANY max_iters reached).
 * rn_fit_homography    stands in for cv2.findHomography(src, dst) at its default method (homography.py:354-355; parity
 *                      with OpenCV is NOT pinned): src, dst fp64 [N,2], offsets int64 [problems+1], one workgroup per
 *                      problem.  Hartley-normalised DLT, the 9x9 normal matrix summed in point order, cyclic Jacobi with
 *                      12 sweeps, the eigenvector of the smallest eigenvalue; for n > 4 and refine != 0 ten damped
 *                      Gauss-Newton steps on the forward transfer error over the eight free entries (8x8 solve with
 *                      partial pivoting; a step is kept only if the error falls); denormalised, H[2,2] = 1.
 *                      H fp64 [problems,3,3] (NaN where status != 0); status int32 [problems]: RN_FIT_FEW_POINTS n < 4,
 *                      RN_FIT_DEGENERATE collinear / coincident points, RN_FIT_NOT_FINITE, RN_FIT_BAD_OFFSETS (the row
 *                      range is not inside the `rows` rows of src / dst). */
#define RN_VP_MAX_AXIS 32
#define RN_VP_FEW_LINES 1
#define RN_VP_BAD_START 2
#define RN_VP_LONG_AXIS 4
#define RN_VP_BAD_OFFSETS 8
#define RN_SZ_BAD_FIRST_STEP 1
#define RN_SZ_NO_WINNER 2
#define RN_SZ_TOO_MANY 4
#define RN_FIT_FEW_POINTS 1
#define RN_FIT_DEGENERATE 2
#define RN_FIT_NOT_FINITE 4
#define RN_FIT_BAD_OFFSETS 8
int rn_vanishing_points(const double *lines, int64_t rows, const int64_t *offsets, int64_t sets, double *out, double *trace,
                        int32_t *status, void *stream);
int rn_hg_reproj_error(const double *boxes, const float *heights, const double *H, const double *P_orig, const double *C,
                       int64_t d, int64_t K, double *out, void *stream);
int rn_hg_scale_z(const double *boxes, const float *heights, const double *H, const double *P_orig, int64_t d,
                  double granularity, double max_scale, int max_iters, double *trace, double *out, int32_t *info,
                  void *stream);
int rn_fit_homography(const double *src, const double *dst, int64_t rows, const int64_t *offsets, int64_t problems, int refine,
                      double *H, int32_t *status, void *stream);

/* ---- tracking CSV resampling and rewrite (csrc/datareader.hip): Data_Reader.reinterpolate / write_to_file --------
 * The host packs the frames of Data_Reader.data in order: offsets int64 [F+1] (rows of frame f), ids int64 [R], fields fp64
 * [R,6] (x, y, l, w, h, v), frame_ts fp64 [F]; and walks the output instants as the reference does (datareader.py:406-444):
 * inst_a int32 [T] (the instant falls in frame pair (a, a + 1)), inst_time fp64 [T].  fp64 with one rounding per operation.
 * All four share one status word (int32, zeroed by the caller, bits OR-ed in): a bad index is never used, its item is left out.
 *   rn_reinterp_mate     replaces `if id in next_ts_data.keys()` (:416-417) for every row: mate int32 [R] = the row of the next
 *                        frame with the same id, else -1.  One workgroup per frame pair; the next frame's ids go through LDS
 *                        in tiles of RN_REINTERP_TILE, so a frame of any size works.  The first match wins.
 *   rn_reinterp_offsets  count int32 [T] = mated rows of frame inst_a[t]; prefix int64 [T+1] = its exclusive prefix (prefix[T]
 *                        = all output rows).  frame_count int32 [F] is workspace.
 *   rn_reinterp_rows     replaces the loop body (:418-430): one workgroup per instant compacts the mated rows of frame a in the
 *                        frame's own order into rows prefix[t] .. prefix[t+1] - 1 of out_fields fp64 [U,6] / out_src int32 [U]
 *                        (the row of frame a) / out_inst int32 [U] (t).  r1 = (t - ts) / (next_ts - ts), r2 = 1 - r1, value =
 *                        field * r1 + next_field * r2: the reference's weights as written (the NEXT frame's value at t == ts).
 *   rn_track_rows        replaces write_to_file's per-row arithmetic (:530-550): state fp32 [N,7] = (x, y, l, w, h, direction,
 *                        v) rounded from fp64; keep uint8 [N] = state[0] != 0 on the fp32 value; space fp32 [N,4,2] (the first
 *                        four corners, x and y); im fp64 [N,8,2] through matrix mat_index[i] of P fp64 [n_mats,3,4] (nullptr:
 *                        matrix 0; P2 != nullptr: Homography_Wrapper's switch on corner-0 y > 60, as rn_state_to_im); box fp64
 *                        [N,4] = (min x, min y, max x, max y) of the eight image corners. */
#define RN_REINTERP_TILE 1024
#define RN_REINTERP_BAD_OFFSETS 1     /* frame offsets not monotone or outside the R rows */
#define RN_REINTERP_BAD_PAIR 2        /* inst_a < 0 or inst_a + 1 >= F */
#define RN_REINTERP_BAD_MATE 4        /* a non-negative mate outside the next frame */
#define RN_REINTERP_BAD_PREFIX 8      /* a destination outside its prefix slot or outside the U output rows */
#define RN_REINTERP_BAD_MAT_INDEX 16  /* mat_index outside the n_mats matrices */
int rn_reinterp_mate(const int64_t *offsets, const int64_t *ids, int64_t F, int64_t R, int32_t *mate, int32_t *status,
                     void *stream);
int rn_reinterp_offsets(const int64_t *offsets, const int32_t *mate, int64_t F, int64_t R, const int32_t *inst_a, int64_t T,
                        int32_t *frame_count, int32_t *count, int64_t *prefix, int32_t *status, void *stream);
int rn_reinterp_rows(const int64_t *offsets, const double *frame_ts, const double *fields, const int32_t *mate,
                     const int32_t *inst_a, const double *inst_time, const int64_t *prefix, int64_t F, int64_t R, int64_t T,
                     int64_t U, double *out_fields, int32_t *out_src, int32_t *out_inst, int32_t *status, void *stream);
int rn_track_rows(const double *fields, const double *direction, const int32_t *mat_index, const double *P, const double *P2,
                  int64_t n_mats, int64_t N, float *state, float *space, double *im, double *box, uint8_t *keep,
                  int32_t *status, void *stream);

/* ---- output frames (csrc/render.hip): MC_Crop_Tracker.plot (MC3D_crop_tracker.py:733-917), Homography.plot_boxes
 * (homography.py:670-714) without cv2.  The drawing rules are this library's own, in exact integer arithmetic (DESIGN.md:
 * "Rendering"); layer order, colours, blend weights and geometry are the reference's.
 * Painting goes into a mask plane uint16 [n_cam,H,W], one bit per layer (RN_RENDER_*), with 32-bit atomicOr on the word that
 * holds two pixels: a pixel's mask, and so the picture, does not depend on the order the primitives arrive in.  The plane's
 * base is 4-byte aligned and its buffer reaches to a multiple of 4 bytes (one spare pixel when n_cam*H*W is odd); the caller
 * clears it.  H, W <= RN_RENDER_MAX_DIM; coordinates are int32; a camera index outside [0, n_cam) paints nothing.  `bit` is a
 * layer's bit NUMBER, 0..15 (the RN_RENDER_* values below are the masks 1 << bit the compose pass tests).
 *   rn_render_edges    the 14 edges (RN_RENDER_EDGES pairs, the reference's DRAW table) of n boxes, corners fp64 [n,8,2] image
 *                      points, cam int32 [n].  Endpoints truncate toward zero; an edge with a non-finite endpoint or one
 *                      outside [-8192, 8191] is skipped whole.  Pixel (x, y) is covered when 4 d^2 <= thickness^2, d the
 *                      distance to the segment, in int64 without division: 4 cross^2 <= t^2 len^2 where the projection
 *                      falls inside, the endpoint distance otherwise (a zero-length edge is a disc).  One workgroup per
 *                      edge, over a per-row interval around the segment clipped to the frame.  1 <= thickness <= 255.
 *   rn_render_rects    rects int32 [n,8] = (x0, y0, x1, y1, cam, mode, anchor, bit): the half-open rectangle [x0,x1) x [y0,y1),
 *                      mode 0 filled, 1 its first/last row and column.  anchor >= 0: x and y are offsets from (int(min x),
 *                      int(max y)) of the eight corners of box `anchor` of anchors fp64 [n_anchor,8,2]; a box with a
 *                      non-finite corner, or one outside [-8192, 8191], anchors nothing.  Empty and off-frame: no-ops.
 *   rn_render_text     runs int32 [n,9] = (x, y, cam, anchor, scale, dilate, bit, start, length): bytes text[start .. start +
 *                      length) on the baseline origin (x, y) (anchored as above).  font uint8 [95,8]: ASCII 32..126, 8 rows
 *                      top to bottom of 6 bits, bit 5 the left column; other bytes draw as '?'.  Character i fills columns
 *                      [x + 6 s i, x + 6 s (i + 1)) and rows [y - 8 s, y); dilate 1 adds every pixel with a covered
 *                      8-neighbour.  1 <= scale <= 64, dilate 0 or 1, start + length <= n_text; clipped at the frame.
 *   rn_render_compose  frames fp32 [n_cam,3,H,W] (normalised RGB) + mask -> out uint8 [R*H, C*W, 3], camera i in tile (i / C,
 *                      i % C), R = ceil(n_cam / C), unused tiles 0.  Per channel, one fp32 rounding per operation:
 *                        u = clamp(floor((x*std + mean)*255 + 0.5), 0, 255); v = u / 255
 *                        PRIOR bit -> (255,255,0); CROP_EDGE -> 255; TRACK -> (0,200,25); DET -> (255,0,0)   (unsaturated)
 *                        crops_present and IN_CROP clear: v = 0.3f*v
 *                        LABEL or LABEL_TEXT: a = TEXT ? 0 : v; b = TEXT ? 0 : (LABEL ? 1 : v); v = 0.7f*a + 0.3f*b
 *                        BANNER_EDGE -> 1; BANNER_TEXT -> 0;   out = (uint8)(clamp(v, 0, 1)*255 + 0.5)
 *                      An empty mask gives the uint8 frame back exactly. */
#define RN_RENDER_PRIOR 1
#define RN_RENDER_CROP_EDGE 2
#define RN_RENDER_TRACK 4
#define RN_RENDER_DET 8
#define RN_RENDER_IN_CROP 16
#define RN_RENDER_LABEL 32
#define RN_RENDER_LABEL_TEXT 64
#define RN_RENDER_BANNER_EDGE 128
#define RN_RENDER_BANNER_TEXT 256
#define RN_RENDER_MAX_DIM 16384
int rn_render_edges(const double *corners, const int32_t *cam, int64_t n, int thickness, int bit, uint16_t *mask, int n_cam,
                    int H, int W, void *stream);
int rn_render_rects(const int32_t *rects, int64_t n, const double *anchors, int64_t n_anchor, uint16_t *mask, int n_cam, int H,
                    int W, void *stream);
int rn_render_text(const int32_t *runs, int64_t n, const uint8_t *text, int64_t n_text, const uint8_t *font,
                   const double *anchors, int64_t n_anchor, uint16_t *mask, int n_cam, int H, int W, void *stream);
int rn_render_compose(const float *frames, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                      const uint16_t *mask, int crops_present, uint8_t *out, int n_cam, int H, int W, int C, void *stream);

/* ---- tracking CSV replay (csrc/replay.hip): Data_Reader.plot_in, Camera_Wrapper and test_integrity (datareader.py:24-89,
 * 253-399, 586-653) without cv2.  Boxes, rectangles and text are painted by rn_render_edges / _rects / _text into a mask plane
 * whose bits mean RN_REPLAY_* here (a bit is a number to the painters).
 *   rn_replay_boxes    state7 fp32 [n,7] = (x, y, l, w, h, direction, v), the objects of one label instant; dt fp64 [n_cam];
 *                      P1 / P2 fp64 [n_cam,3,4] (P2 may be nullptr).  Row c*n + i of the outputs is object i seen by camera c:
 *                      views fp32 [n_cam*n,7] with x' = fl32(fl32(fl32(v * fl32(dt[c])) * direction) + x) (:345: torch's fp32
 *                      arithmetic, the Python scalar rounded to fp32 first); im fp64 [n_cam*n,8,2] = rn_state_to_im of the
 *                      view through camera c's matrices (P2 where corner 0's y > 60); side int32 = 1 where the view's y > 60
 *                      (plot_state_boxes' split, homography.py:874); cam int32 = c.
 *   rn_replay_compose  frames uint8 [n_cam,H,W,3] (swap_rb: B,G,R bytes) + mask uint16 [n_cam,H,W] -> out uint8 [OH,OW,3] RGB.
 *                      Per channel v of a pixel, lowest layer first, integers throughout:
 *                        PRIMARY -> (0,0,255); SECONDARY -> (0,255,0); LABEL -> (7 v + 3*255 + 5) / 10; LABEL_TEXT -> 0
 *                      other mask bits are ignored.  The canvas is R x C tiles of H x W, C = ceil(n_cam / R), camera i in tile
 *                      (row i % R, column i / R) (:371-374), unused tiles 0; CW = C W, CH = R H <= RN_REPLAY_MAX_CANVAS.
 *                      Output pixel (X, Y), per axis (x shown): num = clamp((2X + 1) CW - OW, 0, 2 OW (CW - 1)); x0 = num /
 *                      (2 OW); w1 = num - 2 OW x0; w0 = 2 OW - w1; x1 = min(x0 + 1, CW - 1);
 *                        out = (sum over the four taps of wx wy p + 2 OW OH) / (4 OW OH)            (int64; p composed pixels)
 *                      OW == CW and OH == CH is the identity.  The canvas is never written at another output size.
 *   rn_frame_absdiff   out int64 [1] = sum |a - b| over rows [y0,y1) x columns [x0,x1) x 3 channels of two uint8 [H,W,3]
 *                      frames, the window clipped to the frame (empty: 0).  partial: RN_REPLAY_ABSDIFF_BLOCKS int64 of
 *                      workspace.  Integer adds in two stages: the same result every run.
 *   rn_running_frame   running fp64 [n] <- first ? frame : fl(fl(0.95 running) + fl(0.05 frame)), frame uint8 [n] (:74-77). */
#define RN_REPLAY_PRIMARY 1
#define RN_REPLAY_SECONDARY 2
#define RN_REPLAY_LABEL 4
#define RN_REPLAY_LABEL_TEXT 8
#define RN_REPLAY_MAX_CANVAS 1048576
#define RN_REPLAY_ABSDIFF_BLOCKS 1024
int rn_replay_boxes(const float *state7, int64_t n, const double *dt, const double *P1, const double *P2, int n_cam, float *views,
                    double *im, int32_t *side, int32_t *cam, void *stream);
int rn_replay_compose(const uint8_t *frames, int swap_rb, const uint16_t *mask, uint8_t *out, int n_cam, int H, int W, int R,
                      int OW, int OH, void *stream);
int rn_frame_absdiff(const uint8_t *a, const uint8_t *b, int H, int W, int y0, int y1, int x0, int x1, int64_t *partial,
                     int64_t *out, void *stream);
int rn_running_frame(double *running, const uint8_t *frame, int64_t n, int first, void *stream);

/* ---- multi-camera label audit (csrc/label_audit.hip): the batch passes of the annotator, seems_to_be_working.py ----------
 * Annotator.estimate_ts_bias (:1845-1947), est_y_error (:1950-2036), estimate_projection_error (:2249-2357), remove_outliers
 * (:2192-2233), interpolate (:780-836).  The host packs the labels once into a CSR table of tracklets: tracklet t = object *
 * n_cam + camera, offsets int64 [T+1], rows in ascending frame, cols fp64 [R,3] = (x, y, timestamp), frame int32 [R].  fp64 with
 * one rounding per operation.  All three share one status word (int32, zeroed by the caller, bits OR-ed in): a bad index is
 * never used, its item is left out.
 *   rn_label_pair_samples  one wave per (camera pair, object), pair = cam * (cam - 1) / 2 + prev for prev < cam, entry = pair *
 *                          n_ids + object.  Key column key_col, value columns val0 and val1 (-1: none).  Both tracklets longer
 *                          than one row and max(prev's key) > min(cam's key) (:1889), else the entry's flags are 0.  lo = max of the
 *                          minima, hi = min of the maxima, points lo + ((hi - lo) / 4) * i, i < RN_LABEL_POINTS (:1892-1901); for
 *                          each point and tracklet the LAST i with (K[i] - pt) * (K[i-1] - pt) <= 0 (:1907-1910), ratio = (pt -
 *                          K[i-1]) / (K[i] - K[i-1] + 1e-08), value = V[i-1] + (V[i] - V[i-1]) * ratio.  flags uint8 [entries,
 *                          RN_LABEL_POINTS] (RN_LABEL_GUARD | RN_LABEL_FOUND_CUR | RN_LABEL_FOUND_PREV), values fp64 [entries,
 *                          RN_LABEL_POINTS, 4] = (cam's val0, prev's val0, cam's val1, prev's val1), 0.0 where nothing was found.
 *   rn_label_outliers      one lane per tracklet, serial over its rows (:2195-2231): a row of frame f < n_visit is deleted when
 *                          its key exists in frame f - 1 (frame 0: in the LAST frame, F - 1) and was not itself deleted, and |x -
 *                          x'| > 15 or y - y' > 5 (one-sided, as written); else when the same holds against frame f + 1.  del
 *                          uint8 [R]; n_visit = the frames the reference's walk reaches before its break (:2197-2198).
 *   rn_label_interpolate   every missing frame between two present frames of a tracklet (:800-828): total int64 [1] = their
 *                          number; row u, in tracklet order and frame ascending: t1, t2, ti from all_ts fp64 [F, n_cam] at the
 *                          tracklet's camera, p1 = (t2 - ti) / (t2 - t1), p2 = 1.0 - p1, out fp64 [U,3] = (p1 x' + p2 x, the same
 *                          for y, ti), out_src int32 [U] = the row BEFORE the gap (-1: left out), out_frame int32 [U].  U = the
 *                          caller's row count; total > U sets RN_LABEL_BAD_PREFIX and the rows beyond U are left out. */
#define RN_LABEL_POINTS 5
#define RN_LABEL_MAX_CAMS 1024
#define RN_LABEL_GUARD 1              /* flags: the overlap guard passed */
#define RN_LABEL_FOUND_CUR 2          /* a segment of the camera's tracklet brackets the point */
#define RN_LABEL_FOUND_PREV 4         /* ... of the partner's */
#define RN_LABEL_BAD_OFFSETS 1        /* status: tracklet offsets not monotone or outside the R rows */
#define RN_LABEL_BAD_FRAME 2          /* a frame index outside the F frames or not ascending along its tracklet */
#define RN_LABEL_BAD_PREFIX 4         /* more missing frames than the U output rows */
int rn_label_pair_samples(const int64_t *offsets, const double *cols, int64_t R, int n_cam, int64_t n_ids, int key_col, int val0,
                          int val1, uint8_t *flags, double *values, int32_t *status, void *stream);
int rn_label_outliers(const int64_t *offsets, const double *cols, const int32_t *frame, int64_t T, int64_t R, int64_t F,
                      int64_t n_visit, uint8_t *del, int32_t *status, void *stream);
int64_t rn_label_interpolate_workspace_bytes(int64_t T, int64_t R);
int rn_label_interpolate(const int64_t *offsets, const double *cols, const int32_t *frame, const double *all_ts, int64_t T,
                         int64_t R, int64_t F, int n_cam, int64_t U, void *workspace, double *out, int32_t *out_src,
                         int32_t *out_frame, int64_t *total, int32_t *status, void *stream);

/* ---- re-basing multi-camera labels (csrc/label_rebase.hip): the passes of the annotator that act on the audit ---------------
 * Annotator.replace_homgraphy (seems_to_be_working.py:1629-1730) and offset_box_y (:1779-1805, the arithmetic of replace_y,
 * :1733-1776).  fp64 with one rounding per operation.  rn_label_rebase ORs its bits into the status word of the audit (int32,
 * zeroed by the caller): a bad item is left out, its centre and err stay NaN and its idx -1.
 *   rn_label_rebase    one wave per box.  state6 fp64 [n,6] = (x, y, l, w, h, direction), cam int32 [n]; P1_old, P2_old, P1_new,
 *                      P2_new fp64 [n_cam,12], a P2 of NULL: no Homography_Wrapper switch.  The old box's image footprint
 *                      (:1677-1678): the six values rounded to fp32, the fp32 corners of homography.py:305-320, projected
 *                      with the old matrices (homography.py:438-476, 849-856).  Per round r < rounds, around the centre (the
 *                      box's x, y at first): x = np.linspace(cx - radii[r], cx + radii[r], grid), element k = k * step + start
 *                      with step = (stop - start) / (grid - 1), the last element stop itself; y alike; candidate ix * grid + iy
 *                      is the fp64 state (x[ix], y[iy], l, w, h, direction) (:1685-1691), its corners computed in fp64 and each
 *                      rounded once to fp32 (homography.py:307-318 writes them into a float32 tensor), the wrapper switch taken
 *                      per candidate on that corner-0 y > 60, projected with the new matrices.  Its error (:1701): m_k = (dx *
 *                      dx + dy * dy) / 2 over the bottom corners k < 4, err = (((m0 + m1) + m2) + m3) / 4.  The first smallest
 *                      index wins, as torch.argmin picks it (:1704), and the centre moves to (x[idx / grid], y[idx % grid])
 *                      (:1705).  centre fp64 [n,2], err fp64 [n] = the last round's minimum (:1709), idx int32 [n, rounds].
 *                      2 <= grid <= RN_LABEL_REBASE_MAX_GRID, 1 <= rounds <= RN_LABEL_REBASE_MAX_ROUNDS; the caller computes
 *                      radii with the reference's own `search_rad /= 5` (:1682, :1706).
 *   rn_label_offset_y  one thread per box (:1792-1802): xy fp64 [n,2], coef fp64 [n,3] = the (p2, p1, p0) the host looked up
 *                      under camera + "_EB" | "_WB", y_offset = ((x * x) * p2 + x * p1) + p0, minus y_straight[i] where
 *                      direction[i] == -1; out fp64 [n] = y - y_offset, or y + y_offset with reverse. */
#define RN_LABEL_REBASE_MAX_GRID 16
#define RN_LABEL_REBASE_MAX_ROUNDS 8
#define RN_LABEL_BAD_CAMERA 8         /* status: a camera index outside the n_cam cameras */
#define RN_LABEL_BAD_ERROR 16         /* the error at a round's winning candidate is not finite */
int rn_label_rebase(const double *state6, const int32_t *cam, int64_t n, const double *P1_old, const double *P2_old,
                    const double *P1_new, const double *P2_new, int n_cam, const double *radii, int rounds, int grid,
                    double *centre, double *err, int32_t *idx, int32_t *status, void *stream);
int rn_label_offset_y(const double *xy, const double *coef, const double *y_straight, const int32_t *direction, int64_t n,
                      int reverse, double *out, void *stream);

/* ---- detector-assisted labelling (csrc/label_assist.hip): the annotator's path that MAKES labels -----------------------------
 * Annotator.automate, crop_detect and paste_in_2D_bbox of manual_annotator_state_v3.py (seems_to_be_working.py holds the same
 * code at other line numbers), for n boxes at once.  float32 throughout, one rounding per operation, except inside state_to_im,
 * whose camera matrices are float64.  The status word is the audit's (int32, zeroed by the caller).
 *   rn_label_crop_windows  one thread per box (automate :662-673, crop_detect :707-717).  state6 fp32 [n,6] = (x, y, l, w, h,
 *                          direction), cam int32 [n], P1 / P2 fp64 [n_cam,12] (P2 NULL: no wrapper switch).  The fp32 corners of
 *                          homography.py:305-320 go through P (homography.py:438-476, 849-856); crop_box fp32 [n,4] = min / max
 *                          over the eight fp64 image points, rounded once.  skipped uint8 [n] = 1 where x1 < 0, y1 < 0, x2 >
 *                          width or y2 > height (:672; the reference's 1920 and 1080) or the camera is bad
 *                          (RN_LABEL_BAD_CAMERA); such a box keeps NaN in rois and win.  Otherwise scale = max(w, h) * ber (h
 *                          only where h > w), the window is (cx - scale / 2, cy - scale / 2, cx + scale / 2, cy + scale / 2)
 *                          about cx = (x2 + x1) / 2, cy = (y2 + y1) / 2; rois fp32 [n,5] = (camera, window), win fp32 [n,3] =
 *                          (minx, miny, scale).
 *   rn_label_best_anchor   one wave per crop (crop_detect :731-740).  cls fp32 [n,A,C], reg fp32 [n,A,4] = the LOCALIZE outputs,
 *                          win as above.  conf = the maximum over the C classes (torch.max: a NaN counts as largest, equal
 *                          values go to the lower index), the anchor is torch.argmax of conf by the same rule; box fp32 [n,4] =
 *                          reg[anchor] * scale / cs, x plus minx, y plus miny; anchor int32 [n], conf fp32 [n], klass int32 [n].
 *   rn_label_fit_box2d     one wave per box (paste_in_2D_bbox :603-632).  tmpl fp32 [n,4] = (l, w, h, direction), centre0 fp32
 *                          [n,2], target fp32 [n,4] = (x1, y1, x2, y2).  Per round r < rounds around the centre: x = np.linspace
 *                          (cx - radii[r], cx + radii[r], grid) in fp32 (element k = k * step + start, step = (stop - start) /
 *                          (grid - 1), the last element stop), y alike; candidate ix * grid + iy is the fp32 state (x[ix], y[iy],
 *                          tmpl), its 2D extent as in rn_label_crop_windows with the wrapper switch per candidate; err = (((d0 *
 *                          d0 + d1 * d1) + d2 * d2) + d3 * d3) / 4 with d = extent - target in fp32.  The first smallest index
 *                          wins (torch.argmin: a NaN counts as smallest) and the centre moves to (x[idx / grid], y[idx % grid]).
 *                          centre fp32 [n,2], err fp32 [n] = the last round's minimum, idx int32 [n, rounds].  A bad camera
 *                          (RN_LABEL_BAD_CAMERA) or a winning error that is not finite (RN_LABEL_BAD_ERROR) leaves the box out:
 *                          NaN, NaN, -1.  Limits as rn_label_rebase's: 2 <= grid <= RN_LABEL_REBASE_MAX_GRID, 1 <= rounds <=
 *                          RN_LABEL_REBASE_MAX_ROUNDS; radii fp64 [rounds], each rounded to fp32 first.  skip uint8 [n] or NULL:
 *                          a box whose byte is set (rn_label_crop_windows' skipped) is left out too, without a status bit. */
int rn_label_crop_windows(const float *state6, const int32_t *cam, int64_t n, const double *P1, const double *P2, int n_cam,
                          float ber, float width, float height, float *crop_box, float *rois, float *win, uint8_t *skipped,
                          int32_t *status, void *stream);
int rn_label_best_anchor(const float *cls, const float *reg, const float *win, int64_t n, int A, int C, float cs, float *box,
                         int32_t *anchor, float *conf, int32_t *klass, void *stream);
int rn_label_fit_box2d(const float *tmpl, const int32_t *cam, const float *centre0, const float *target, const uint8_t *skip,
                       int64_t n, const double *P1, const double *P2, int n_cam, const double *radii, int rounds, int grid, float *centre,
                       float *err, int32_t *idx, int32_t *status, void *stream);

/* ---- smoothing-spline trajectories of multi-camera labels (csrc/label_spline.hip) -------------------------------------------
 * Annotator.create_trajectory (seems_to_be_working.py:1137-1314), get_splines (:1338-1350), gen_trajectories (:1317-1336),
 * adjust_ts_with_trajectories (:1353-1458).  fp64 with one rounding per operation, in FITPACK's order.  The status word is the
 * audit's (int32, zeroed by the caller, bits OR-ed in); a bad item is left out.
 *   rn_label_box_weights  one thread per box (:1186-1196): state6 fp64 [n,6] rounded to fp32, the fp32 corners of
 *                         homography.py:305-320 projected in fp64 with the box's own camera (P2 of NULL: no wrapper switch);
 *                         out fp64 [n,4] = (x_weight, y_weight, x_diff, y_diff): diff = the norm of the mean of the two corner
 *                         differences (corners 0,1 - 2,3 along the length, 0,2 - 1,3 across), weight = diff / l or / w.
 *   rn_spline_fit         FITPACK curfit (fpcurf, iopt = 0, xb = x[0], xe = x[m-1], tol = 1e-3, maxit = 20, nest = max(m + k + 1,
 *                         2k + 3)), one lane per candidate smoothing factor.  grp int32 [G, RN_SPLINE_GRP] = (row0, m, k, ncap,
 *                         cand0, ncand, wave0, axis) per (object, axis): rows [row0, row0 + m) of tx / val / wt fp64 [R] (abscissae
 *                         ascending, ordinates, weights), k in {2, 3}, candidates s[cand0 .. cand0 + ncand), lanes [wave0 * 64,
 *                         ...).  waves int32 [NW, 2] = (group, first candidate) of every wave.  A lane whose knot count n would
 *                         pass ncap (<= the launch's ncap <= RN_SPLINE_MAX_NCAP; the caller sets it to the reference's knot limit
 *                         + 2k, at most m + k + 1) stops with ier RN_SPLINE_REJECTED; RN_SPLINE_STUCK where FITPACK's fpknot
 *                         finds no interval to split (it reads an unset index there); RN_SPLINE_UNUSED on a padding lane.
 *                         workspace: RN_SPLINE_WS_COLS columns of ncap doubles per lane, element e of lane L at [e * NW * 64 + L],
 *                         columns t, c, z, fpint, nrdata, a (4), g (5), b (5).  out_n / out_ier / out_iter int32 [NW * 64], out_fp
 *                         fp64 [NW * 64]; out_iter = least-squares rounds + iterations on p.
 *   rn_spline_select      one workgroup per group: a candidate survives with ier <= 3 and a value at 0 that is not NaN (:1238);
 *                         its score over the group's rows with the weights wscore, summed in ascending row order: metric 0
 *                         sqrt(sum / m), metric 1 sqrt(max) on axis 0 and max on axis 1 (:1246-1255, :1269-1278); the first
 *                         smallest below +inf wins.  scores fp64 [NC] (NaN: skipped), win int32 [G,3] = (candidate or -1, n, ier),
 *                         wfig fp64 [G, RN_SPLINE_FIGS] = (fp, score, sqrt(mean r^2), sqrt(mean (wt r)^2), sqrt(max (wt r)^2)) of the
 *                         winner (:1282-1294), wt_out / wc_out fp64 [G, ncap] = its knots and coefficients, zero-filled.
 *   rn_spline_eval        one thread per query: FITPACK splev with extrapolation; st / sc fp64 [S, ncap], snk int32 [S,2] = (n, k),
 *                         qs int32 [Q] (outside [0, S) or n = 0: NaN), qt fp64 [Q] -> out fp64 [Q].
 *   rn_label_ts_shift     one wave per (frame, camera) entry e < E (:1416-1442): rows [off[e], off[e+1]) = its kept objects, rs
 *                         int32 the spline, rx fp64 the label x.  Trial j < trials: time = (base[e] + shifts[j]) + run[e] (without
 *                         use_run: base[e] + shifts[j]), error = sqrt(mean d^2) (metric 1: sqrt(max d^2)), d = fp32(spline(time)) -
 *                         x in fp64, ascending rows; the first smallest below +inf wins.  best_t fp64 [E] (no winner: base[e]), errs
 *                         fp64 [E,2] = (best, initial: sqrt(mean d^2) at base[e]), best_i int32 [E] (-1: none).  trials < 64. */
#define RN_SPLINE_GRP 8
#define RN_SPLINE_WS_COLS 19
#define RN_SPLINE_FIGS 5
#define RN_SPLINE_MAX_NCAP 4096
#define RN_SPLINE_UNUSED 97           /* ier of a lane without a candidate */
#define RN_SPLINE_STUCK 98            /* ... whose knot insertion found no interval */
#define RN_SPLINE_REJECTED 99         /* ... stopped at the knot limit */
#define RN_SPLINE_BAD_TABLE 32        /* status: a group, wave or row range outside its table */
int64_t rn_spline_fit_workspace_bytes(int64_t n_waves, int ncap);
int rn_label_box_weights(const double *state6, const int32_t *cam, int64_t n, const double *P1, const double *P2, int n_cam,
                         double *out, int32_t *status, void *stream);
int rn_spline_fit(const int32_t *grp, int64_t G, const int32_t *waves, int64_t NW, const double *tx, const double *val,
                  const double *wt, int64_t R, const double *s, int64_t NC, int ncap, void *workspace, int32_t *out_n,
                  int32_t *out_ier, double *out_fp, int32_t *out_iter, int32_t *status, void *stream);
int rn_spline_select(const int32_t *grp, int64_t G, const double *tx, const double *val, const double *wt, const double *wscore,
                     int64_t R, int64_t NC, int64_t NW, int ncap, const void *workspace, const int32_t *out_n,
                     const int32_t *out_ier, const double *out_fp, int metric, double *scores, int32_t *win, double *wfig,
                     double *wt_out, double *wc_out, int32_t *status, void *stream);
int rn_spline_eval(const double *st, const double *sc, const int32_t *snk, int64_t S, int ncap, const int32_t *qs,
                   const double *qt, int64_t Q, double *out, void *stream);
int rn_label_ts_shift(const double *st, const double *sc, const int32_t *snk, int64_t S, int ncap, const int64_t *off,
                      const int32_t *rs, const double *rx, int64_t E, int64_t Rr, const double *base, const double *run,
                      const double *shifts, int trials, int use_run, int metric, double *best_t, double *errs, int32_t *best_i,
                      int32_t *status, void *stream);

/* ---- scoring a multi-camera label set (csrc/label_quality.hip): the metrics of the later annotator --------------------------
 * manual_annotator_state_v3.py: calculate_total_variation (:3843-3889), calculate_feasibility (:3891-3979), the data half of
 * plot_trajectories_unified (:3634-3711, smooth = 1), the reduction of annotator_rmse (:3981-4007).  fp64 with one rounding per
 * operation (atan2 aside).  The status word is the audit's (int32, zeroed by the caller, bits OR-ed in).
 *   rn_label_series      one workgroup per object on the audit's table (offsets int64 [n_ids * n_cam + 1], cols fp64 [R,3] = (x, y,
 *                        timestamp)): the rows of object j are [offsets[j * n_cam], offsets[(j + 1) * n_cam]), camera outer, frame
 *                        inner.  With lane_on only rows with lane_lo < y < lane_hi take part (:3645-3646).  The n rows that do are
 *                        sorted by (timestamp, position in the object's rows) -- the stable sort by time -- in LDS when the
 *                        object's row count, rounded up to a power of two, is at most lds_rows (a power of two, 2 ..
 *                        RN_LABEL_SERIES_MAX_LDS_ROWS), else in the workspace.  order int32 [R]: at [offsets[j * n_cam] + i], i <
 *                        n, the row of the i-th sorted box, -1 behind; keep uint8 [R]: 1 for i = 0 and where t[i] >= t[i-1] +
 *                        0.01 against the previous SORTED row (:3875-3878), 0 behind n.  series fp64 [RN_LABEL_SERIES_PLANES, R]:
 *                        planes t, x, y, v, vy, a, theta of the m kept rows from the same first position, 0.0 behind: dt[i] =
 *                        (t[i+1] - t[i]) + 1e-08, v[i] = -((x[i+1] - x[i]) / dt[i]), vy[i] = (y[i+1] - y[i]) / dt[i], a[i] =
 *                        (v[i+1] - v[i]) / dt[i] on the extended v, the last value of each repeated (all 0.0 for m = 1); theta =
 *                        atan2(vy, v) * 180 / pi.  counts int32 [n_ids,3] = (n, m, feasible segments: of the m - 1, those with v
 *                        in (0, 140) and theta in (-25, 25) at both ends -- the reference's acceleration mask never enters, :3975);
 *                        figs fp64 [n_ids,2] = (max(x) - min(x), sum |x[i] - x[i-1]| in ascending order) over the kept rows.
 *                        offsets[0] != 0, offsets[n_ids * n_cam] != R or an object's range out of order: RN_LABEL_BAD_OFFSETS.
 *   rn_label_group_rmse  one workgroup per group: im fp64 [n,8,2] image corners, group int32 [n] ascending ids in [0, n_groups)
 *                        (else RN_LABEL_BAD_GROUP).  im_pos = (corner 2 + corner 3) / 2 (:3997); mean fp64 [n_groups,2] = sum /
 *                        count, rmse fp64 [n_groups] = sqrt(sum(dx * dx + dy * dy) / count), sums in ascending row order; count
 *                        int32 [n_groups]; an empty group: NaN, NaN, 0. */
#define RN_LABEL_SERIES_PLANES 7
#define RN_LABEL_SERIES_MAX_LDS_ROWS 4096   /* 48 KiB of keys and indices: three workgroups share the 160 KiB of a CU */
#define RN_LABEL_BAD_GROUP 64         /* status: group ids that do not ascend or lie outside the groups */
int64_t rn_label_series_workspace_bytes(int64_t R);
int rn_label_series(const int64_t *offsets, const double *cols, int64_t R, int n_cam, int64_t n_ids, int lane_on, double lane_lo,
                    double lane_hi, int lds_rows, void *workspace, int32_t *order, uint8_t *keep, double *series, int32_t *counts,
                    double *figs, int32_t *status, void *stream);
int rn_label_group_rmse(const double *im, const int32_t *group, int64_t n, int64_t n_groups, double *rmse, double *mean,
                        int32_t *count, int32_t *status, void *stream);

/* ---- track stitching (csrc/stitch.hip): joining the fragments of one vehicle (track_stitch.py) -----------------------------------
 * Beyond the reference.  A tracklet is all rows of one id in time order; the host packs offsets int64 [N+1], cols fp64 [R,7] = (t, x,
 * y, l, w, h, v), direction int32 [R], N <= RN_STITCH_MAX_TRACKLETS.  fp64 with one rounding per operation, every expression in
 * the order tests/stitch_cases.py writes it.  All entry points that take one share a status word (int32, zeroed by the caller, bits
 * OR-ed in): a bad index is never used, its item is left out.  The seven scales of a cost follow N in this order: max_gap (s),
 * back_tol, sigma_x0, sigma_x1 (per second of gap), sigma_y, sigma_size (feet), max_cost.
 *   rn_stitch_endpoints    ep fp64 [N,2,RN_STITCH_EP]: end 0 = the head (first rows), end 1 = the tail.  Over the k = min(n, fit_n)
 *                          rows nearest the end, sums sequential in ascending row order: mt, mx, Stt = sum (t - mt)^2, Stx = sum
 *                          (t - mt)(x - mx); vx = Stx / Stt, or sgn * v of the end row when k < 2 or Stt <= 0; sgn = +1 when the
 *                          sum of the tracklet's directions is >= 0, else -1.  Fields: 0 t of the end row, 1 x^ = mx + vx (t - mt),
 *                          2 vx, 3..6 the means of y, l, w, h, 7..11 the end row's x, y, l, w, h, 12 sgn, 13 k, 14..15 zero.
 *                          1 <= fit_n <= RN_STITCH_MAX_FIT.  A NaN or infinity anywhere in cols: RN_STITCH_NONFINITE.
 *   rn_stitch_costs        W fp64 [N,N], W[a,b] for a's tail -> b's head with gap = t_s[b] - t_e[a]: linkable when a != b, sgn
 *                          equal, 0 < gap <= max_gap, sgn (x^_s[b] - x^_e[a]) >= -back_tol and cost < max_cost, where cost =
 *                          ((|x^_e + vx_e gap - x^_s| + |x^_s - vx_s gap - x^_e|) / 2) / (sigma_x0 + sigma_x1 gap) + |y_e - y_s| /
 *                          sigma_y + (|dl| + |dw| + |dh|) / sigma_size.  W = cost - max_cost when linkable, else 0.
 *   rn_stitch_candidates   the same pairs without the matrix: has uint8 [2,N] (workspace: row_has, col_has), then cand int32
 *                          [2,2,N] = per direction (sgn = +1 first) the tails and the heads that have a candidate, ascending, -1
 *                          behind; ncand int32 [4] = (nr'+, nc'+, nr'-, nc'-).
 *   rn_stitch_compact      Wc fp64: direction + at 0 as [nr'+, nc'+], direction - behind it as [nr'-, nc'-]; cap = the doubles Wc
 *                          holds.  The cells are those of W, bit for bit.
 *   rn_stitch_assign       scipy.optimize.linear_sum_assignment(Wc) per direction on one wave64 (lsap_dev.h; it transposes when
 *                          nr' > nc'); a link is an assigned cell with W < 0.  next / prev int32 [N] (-1: none), link_cost fp64 [N]
 *                          at the tail's index.  min(nr', nc') > RN_LSAP_MAX_MIN: RN_STITCH_TOO_MANY, no links for that direction.
 *   rn_stitch_chains       root int32 [N] = the chain's earliest fragment, rank int32 [N] = the position in the chain, new_id int64
 *                          [N] = ids[root]; pointer jumping in one launch, workspace int32 [4 N].
 *   rn_stitch_fill_count   count int32 [N] at the tail's index = how many k >= 1 have t_e + k (1.0 / fill_rate) < t_s (at most
 *                          RN_STITCH_MAX_FILL, else RN_STITCH_FILL_OVERFLOW and 0); prefix int64 [N+1] its exclusive prefix.
 *   rn_stitch_fill_rows    one thread per new row of the U the arrays hold (prefix[N] <= U): t_k, u = (t_k - t_e) / g, g = t_s -
 *                          t_e; fields fp64 [U,6] = (x, y, l, w, h, v): x the cubic Hermite through the end rows' x with the fitted
 *                          slopes, v = |dx/dt|, the others (1 - u) A + u B of the end rows; time fp64 [U]; link int32 [U] = the tail's
 *                          tracklet; side uint8 [U] = 0 when u <= 0.5, else 1. */
#define RN_STITCH_EP 16
#define RN_STITCH_MAX_TRACKLETS 32768
#define RN_STITCH_MAX_FIT 64
#define RN_STITCH_MAX_FILL 1048576
#define RN_STITCH_NONFINITE 1         /* a NaN or an infinity in cols */
#define RN_STITCH_BAD_OFFSETS 2       /* tracklet offsets not monotone, an empty tracklet, or rows outside R */
#define RN_STITCH_TOO_MANY 4          /* min(nr', nc') of a direction above RN_LSAP_MAX_MIN */
#define RN_STITCH_SOLVER 8            /* the solver found no complete assignment (not reachable with finite cells) */
#define RN_STITCH_BAD_CANDIDATES 16   /* candidate counts or entries outside the tracklets or outside cap */
#define RN_STITCH_BAD_LINK 32         /* a next / prev entry outside the tracklets, or pointing at itself */
#define RN_STITCH_BAD_PREFIX 64       /* a new row outside its prefix slot or outside the U rows */
#define RN_STITCH_FILL_OVERFLOW 128   /* a link with RN_STITCH_MAX_FILL new rows or more */
int rn_stitch_endpoints(const int64_t *offsets, const double *cols, const int32_t *direction, int64_t N, int64_t R, int fit_n,
                        double *ep, int32_t *status, void *stream);
int rn_stitch_costs(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1, double sigma_y,
                    double sigma_size, double max_cost, double *W, void *stream);
int rn_stitch_candidates(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1,
                         double sigma_y, double sigma_size, double max_cost, uint8_t *has, int32_t *cand, int32_t *ncand,
                         void *stream);
int rn_stitch_compact(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1, double sigma_y,
                      double sigma_size, double max_cost, const int32_t *cand, const int32_t *ncand, int64_t cap, double *Wc,
                      int32_t *status, void *stream);
int64_t rn_stitch_assign_workspace_bytes(int64_t N);
int rn_stitch_assign(const double *ep, int64_t N, double max_gap, double back_tol, double sigma_x0, double sigma_x1, double sigma_y,
                     double sigma_size, double max_cost, const int32_t *cand, const int32_t *ncand, const double *Wc, int64_t cap,
                     void *workspace, int32_t *next, int32_t *prev, double *link_cost, int32_t *status, void *stream);
int rn_stitch_chains(const int32_t *prev, const int64_t *ids, int64_t N, int32_t *workspace, int32_t *root, int32_t *rank,
                     int64_t *new_id, int32_t *status, void *stream);
int rn_stitch_fill_count(const double *ep, const int32_t *next, int64_t N, double fill_rate, int32_t *count, int64_t *prefix,
                         int32_t *status, void *stream);
int rn_stitch_fill_rows(const double *ep, const int32_t *next, const int64_t *prefix, int64_t N, int64_t U, double fill_rate,
                        double *fields, double *time, int32_t *link, uint8_t *side, int32_t *status, void *stream);

/* ---- fixed-interval smoothing (csrc/smooth.hip): a Rauch-Tung-Striebel pass over every tracklet (track_smooth.py) ---------------
 * Beyond the reference.  Tracklets as for stitching: offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v), direction int32
 * [R], N <= RN_SMOOTH_MAX_TRACKLETS, R < 2^31.  order int32 [N]: lane i of the grid works on tracklet order[i] (the host passes the
 * stable argsort of descending length; any permutation gives the same bytes).  model fp64 [RN_SMOOTH_MODEL] = q_scale Q [6,6],
 * r_scale R [5,5], P0 [6,6], row-major, each symmetric.  State (x, y, l, w, h, v), measurement (x, y, l, w, h) of the row: H = [I5 | 0]
 * is fixed.  d = +1 when the sum of the tracklet's directions is >= 0, else -1; F = I with F[0][5] = f = d dt, dt = t_k - t_(k-1); Qk =
 * ((q_scale Q[a][b]) dt) / dt_default.  fp64 with one rounding per operation, every expression in the order tests/smooth_cases.py
 * writes it; a covariance is its 21 entries a <= b, row-major.
 *   rn_smooth_filter   row 0: s = the row's (x, y, l, w, h, v), P = P0.  Row k >= 1: s[0] += f s[5]; P- = F P F^T + Qk in the sparse
 *                      form (row 0 of F P, then column 0); y = z - s-[:5], S = P-[:5,:5] + R = L D L^T (Cholesky-Crout, no square
 *                      roots); nis = y^T S^-1 y; gate > 0 and nis > gate: flag = 1 and s = s-, P = P- (the row counts as missing);
 *                      else K = P-[:,:5] S^-1, s = s- + K y, P = (I - K H) P- (I - K H)^T + K R K^T.  filt fp64 [R,RN_SMOOTH_FILT] = 6
 *                      means + the 21 entries, nis fp64 [R] (0 at a first row), flag uint8 [R].  gate = 0: no gating.
 *   rn_smooth_rts      k = n-2 .. 0 from filt: P-(k+1) recomputed as above, C = P_k F^T (P-(k+1))^-1 by a 6x6 L D L^T, s^s_k = s_k + C
 *                      (s^s_(k+1) - F s_k), P^s_k = P_k + C (P^s_(k+1) - P-(k+1)) C^T; row n-1 keeps its filtered values.  out fp64
 *                      [R,RN_SMOOTH_OUT] = the 6 smoothed means and the 6 smoothed variances.
 * Both OR bits into the status word (int32, zeroed by the caller); the lane of a refused tracklet ends there and what its rows
 * hold is unspecified. */
#define RN_SMOOTH_MODEL 97
#define RN_SMOOTH_FILT 27
#define RN_SMOOTH_OUT 12
#define RN_SMOOTH_MAX_TRACKLETS 1048576
#define RN_SMOOTH_NONFINITE 1         /* a NaN or an infinity in a row's fields */
#define RN_SMOOTH_BAD_OFFSETS 2       /* tracklet offsets out of order, an empty tracklet, or rows outside R */
#define RN_SMOOTH_BAD_DT 4            /* a time step <= 0 inside a tracklet */
#define RN_SMOOTH_PIVOT 8             /* a pivot of S or of P- that is not a positive finite number */
#define RN_SMOOTH_BAD_ORDER 16        /* an order entry outside the tracklets */
int rn_smooth_filter(const int64_t *offsets, const int32_t *order, const double *cols, const int32_t *direction, const double *model,
                     double gate, double dt_default, int64_t N, int64_t R, double *filt, double *nis, uint8_t *flag, int32_t *status,
                     void *stream);
int rn_smooth_rts(const int64_t *offsets, const int32_t *order, const double *cols, const int32_t *direction, const double *model,
                  double dt_default, int64_t N, int64_t R, const double *filt, double *out, int32_t *status, void *stream);

/* ---- traffic state from tracking output (csrc/traffic.hip): Edie's fields per lane, leaders and gaps (traffic_state.py) -----------
 * Beyond the reference.  Tracklets as for stitching: offsets int64 [N+1] (offsets[0] = 0, offsets[N] = R, ascending), cols fp64
 * [R,7] = (t, x, y, l, w, h, v), direction int32 [R], R < 2^31.  Lane edges: two fp64 arrays, edges_pos [n_pos] for direction +1 and
 * edges_neg [n_neg] for -1, each ascending, at most RN_TRAFFIC_MAX_EDGES entries; the lane of y is the first k with edges[k] <= y <
 * edges[k+1], else -1; L = max(n_pos, n_neg) - 1 (0 when that is negative).  fp64 with one rounding per operation, every expression
 * in the order tests/traffic_cases.py writes it.
 *   rn_traffic_lanes    dir int32 [N] = +1 when the sum of the tracklet's directions is >= 0, else -1; lane int32 [R] = the lane of
 *                       the row's own y under its tracklet's dir.  Every field of every row is checked for a NaN or an infinity.
 *   rn_traffic_cells    one thread per segment (rows a, b = a + 1 of one tracklet) over the grid t0 + it dt, x0 + ix dx, it < nt, ix <
 *                       nx.  Tt = t_b - t_a, X = x_b - x_a; not 0 < Tt <= max_gap: skipped_gap; the lane of ym = (y_a + y_b) 0.5 under
 *                       dir is -1: skipped_lane.  Cuts s in (0, 1): ((t0 + k dt) - t_a) / Tt for k = ka + 1 .. kb, ka = floor((t_a - t0)
 *                       / dt), kb likewise of t_b, and ((x0 + m dx) - x_a) / X for m = ma + 1 .. mb of lo = min(x_a, x_b) and hi =
 *                       max(x_a, x_b); k and m are formed as ka + (double)i.  Pieces [u, v] between consecutive values of {0, cuts, 1}
 *                       in ascending order, those with v <= u dropped; with sm = (u + v) 0.5 a piece belongs to it = floor(((t_a + sm
 *                       Tt) - t0) / dt), ix = floor(((x_a + sm X) - x0) / dx); outside the grid: `outside`; else T += rint(((v - u) Tt)
 *                       Q), D += rint(((v - u) |X|) Q), n += 1 at [dir index (0 for +1, 1 for -1), lane, it, ix], Q = RN_TRAFFIC_Q.
 *                       T, D int64 and n int32 [2,L,nt,nx] and counters int64 [RN_TRAFFIC_COUNTERS] = (segments, used, skipped_gap,
 *                       skipped_lane, pieces, outside, 0, 0) are ADDED to: the caller zeroes them.  2 L nt nx < 2^31.  The sums are
 *                       integers, so they do not depend on the order the atomics land in.
 *   rn_traffic_leaders  one workgroup per frame f, whose rows are frame_rows[frame_off[f] .. frame_off[f+1]) (int64 [F+1] into int32
 *                       [Rf] packed row indices, every packed row at most once).  For row i the candidates are the frame's rows j !=
 *                       i with dir_j == dir_i, lane_j == lane_i >= 0 and s = dir_i (x_j - x_i) > 0; the leader is the one with the
 *                       smallest s, then the smaller tracklet index, then the smaller row.  leader int32 [R] (packed row, -1: none),
 *                       spacing = s, gap = s - l_i, headway = s / v_i when v_i > 0 else +inf, ttc = gap / (v_i - v_j) when v_i > v_j
 *                       and gap > 0 else +inf: fp64 [R] each.  Rows outside every frame are not written: the caller fills -1 and
 *                       +inf.  counters int64 [RN_TRAFFIC_COUNTERS] = (rows with a leader, rows with gap < 0, 0 ...), added to.
 * All OR bits into the status word (int32, zeroed by the caller); a refused row or segment is left out. */
#define RN_TRAFFIC_Q 1048576
#define RN_TRAFFIC_COUNTERS 8
#define RN_TRAFFIC_MAX_EDGES 64
#define RN_TRAFFIC_MAX_CUTS 4096
#define RN_TRAFFIC_NONFINITE 1        /* a NaN or an infinity in a row's fields */
#define RN_TRAFFIC_BAD_OFFSETS 2      /* tracklet offsets out of order or not covering the R rows */
#define RN_TRAFFIC_BAD_FRAME 4        /* frame offsets out of order, or a frame row outside the packed rows */
#define RN_TRAFFIC_TOO_MANY_CUTS 8    /* a segment crosses more than RN_TRAFFIC_MAX_CUTS grid lines */
#define RN_TRAFFIC_RANGE 16           /* a segment of 2^20 s or ft or more: its fixed-point share is not trusted */
#define RN_TRAFFIC_BAD_DIR 32         /* a dir entry that is neither +1 nor -1 */
int rn_traffic_lanes(const int64_t *offsets, const double *cols, const int32_t *direction, const double *edges_pos, int n_pos,
                     const double *edges_neg, int n_neg, int64_t N, int64_t R, int32_t *dir, int32_t *lane, int32_t *status,
                     void *stream);
int rn_traffic_cells(const int64_t *offsets, const double *cols, const int32_t *dir, const double *edges_pos, int n_pos,
                     const double *edges_neg, int n_neg, int64_t N, int64_t R, double t0, double dt, int64_t nt, double x0, double dx,
                     int64_t nx, double max_gap, int64_t *T, int64_t *D, int32_t *n, int64_t *counters, int32_t *status, void *stream);
int rn_traffic_leaders(const int64_t *offsets, const double *cols, const int32_t *dir, const int32_t *lane, const int64_t *frame_off,
                       const int32_t *frame_rows, int64_t N, int64_t R, int64_t F, int64_t Rf, int32_t *leader, double *spacing,
                       double *gap, double *headway, double *ttc, int64_t *counters, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif

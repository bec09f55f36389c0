"""The HIP entry points as PyTorch custom operators: ``torch.ops.retinanet_mi355x.*`` (north_star: "exposed to Python through
PyTorch-ROCm custom ops").

Registered with ``torch.library.custom_op`` over the SAME C ABI the rest of the package binds (``_hip.py`` /
``include/retinanet_mi355x.h``): an operator is a schema + a CUDA(HIP)-device implementation that launches the library's
kernel on the current stream + a fake (meta) implementation that only derives output shapes, so the ops show up in
``torch.ops``, carry dispatcher-level schemas and device checks, are visible to ``torch.compile`` / export tracing as
opaque nodes, and ``focal_loss`` carries its hand-written backward through ``register_autograd``.  There is no CPU
kernel registered: calling an op with CPU tensors fails in the dispatcher ("no kernel for CPU"), which is this package's
no-fallback rule at the operator level.

Operator                                         reference code it stands for
  anchors(H, W, device)                          Anchors.forward                       D/anchors.py:21-40
  pairwise_iou(a, b)                             calc_iou                              D/losses.py:5-22
  focal_loss(cls, reg, anchors, ann, dir)        FocalLoss.forward (+ autograd)        D/losses.py:27-362, R/losses.py:27-177
  decode_dir(anchors, reg) / decode_2d(...)      BBoxTransform.forward                 D/utils.py:102-149, R/utils.py:102-126
  clip_boxes_(boxes, H, W)                       ClipBoxes.forward (in place)          R/utils.py:134-144
  nms(boxes, scores, thr)                        torchvision.ops.nms as the path uses it   D/model.py:383
  linear_sum_assignment(cost)                    scipy.optimize.linear_sum_assignment  MC3D_crop_tracker.py:706
  estimate_ts_bias(boxes, cams, objs, ts, bias..) MC_Crop_Tracker.estimate_ts_bias      MC3D_crop_tracker.py:237-315
  track_crop_prior(X, D, T, F, centers, ts, bias) crop frame: view, nearest camera, dt  MC3D_crop_tracker.py:1150-1171
  fit_nearest(gt, det, offsets)                  nearest-box search of the R fit       fit_filter_3D.py:356-375
  residual_moments(E, group, groups)             mean / covariance loops               fit_filter_3D.py:292-299, 377-384, 426-434
  state_to_space / state_to_im / im_to_state     Homography transforms                 homography.py:305-320, 479-500
  frame_ingest(frames_u8, swap_rb, nhwc4)        to_tensor + normalize of the loaders  util_track/mp_loader.py:239-243
  frame_ingest_half(frames_u8, swap_rb, nhwc4)   cv2.resize (exact halving) + the above   util_track/mp_loader.py:237-243
  parse_frame_timestamps(frames_u8, geometry, ..) parse_frame_timestamp, sets tried in turn  timestamp_utilities.py:46-115
  augment_frames(frames_u8, records, tx, ty, ..) Detection_Dataset.__getitem__'s image chain  corrected_3D_dataset.py:330-478
  augment_crops(frames_u8, records, 4 tables, ..) ... with CROP > 0 (the crop detector's)     corrected_3D_dataset.py:501-594
  eval_select(scores, labels, boxes, table, ..)  _get_detections' selection (in place)  R/csv_eval.py:102-123
  eval_match(table, img_rows, ann_box, off, ..)  evaluate's greedy matching             R/csv_eval.py:189-213, 21-35
  eval_ap(table, state, tp, num_annotations)     per-class sort + _compute_ap           R/csv_eval.py:216-235, 38-62
  eval_corners / eval_cuboid_overlap / eval_cuboid_assign / eval_cuboid_errors          (no counterpart: eval3d.py)
                                                 3D validation: cuboid IoU, matching, corner errors
  mot_prepare / mot_iou / mot_assign /           MOT_Evaluator.evaluate, all frames    mot_evaluator.py:120-412
  mot_frame_metrics / mot_reduce
  mot_id_counts / mot_id_assign /                IDF1 and HOTA of the same frames      beyond the reference (csrc/mot_assoc.hip)
  mot_hota_align / mot_hota_assign /
  mot_hota_reduce
  vanishing_points(lines, offsets)               find_vanishing_point, many sets       homography.py:96-154
  hg_reproj_error(boxes, heights, H, P, C)       test_transformation's arithmetic      homography.py:581-587
  hg_scale_z(boxes, heights, H, P, gran, max)    scale_Z's search                      homography.py:607-666
  fit_homography(src, dst, offsets, refine)      cv2.findHomography (parity unpinned)  homography.py:354-355
  reinterp_mate / reinterp_offsets /             Data_Reader.reinterpolate, all rows   datareader.py:411-434
  reinterp_rows
  track_rows(fields, direction, P, P2, index)    Data_Reader.write_to_file's row math  datareader.py:530-550
  render_edges / render_rects / render_text /    MC_Crop_Tracker.plot, plot_boxes      MC3D_crop_tracker.py:733-917
  render_compose                                 (own drawing rules, no cv2)           homography.py:670-714
  replay_boxes / replay_compose /                Data_Reader.plot_in, Camera_Wrapper,  datareader.py:24-89, 253-399
  frame_absdiff / running_frame                  test_integrity                        datareader.py:586-653
  label_pair_samples(offsets, cols, n_cam, ..)   Annotator.estimate_ts_bias, est_y_error,   seems_to_be_working.py:1845-2036,
                                                 estimate_projection_error (the samples)    2249-2357
  label_outliers(offsets, cols, frame, F, visit) Annotator.remove_outliers             seems_to_be_working.py:2192-2233
  label_interpolate(offsets, cols, frame, ts, n) Annotator.interpolate, every object   seems_to_be_working.py:780-836
  label_rebase(state6, cam, 4 x P, radii, grid)  Annotator.replace_homgraphy's search  seems_to_be_working.py:1677-1709
  label_offset_y(xy, coef, y_straight, dir, rev) Annotator.offset_box_y, every box     seems_to_be_working.py:1779-1805
  label_crop_windows(state6, cam, P1, P2, ..)    Annotator.automate's crop box and edge     manual_annotator_state_v3.py:662-673,
                                                 test, crop_detect's square window          707-717
  label_best_anchor(cls, reg, win, cs)           Annotator.crop_detect's best anchor   manual_annotator_state_v3.py:731-740
  label_fit_box2d(tmpl, cam, centre, target, ..) Annotator.paste_in_2D_bbox's search   manual_annotator_state_v3.py:603-632
  label_box_weights(state6, cam, P1, P2)         Annotator.create_trajectory's weights seems_to_be_working.py:1186-1196
  spline_fit / spline_select / spline_eval       ... its UnivariateSpline fits (FITPACK     seems_to_be_working.py:1233-1294
                                                 curfit), scores and winner; splev
  label_ts_shift(splines, entries, shifts, ..)   Annotator.adjust_ts_with_trajectories seems_to_be_working.py:1416-1442
  stitch_endpoints / stitch_costs /              joining the fragments of one vehicle  beyond the reference (csrc/stitch.hip,
  stitch_candidates / stitch_compact /           (link costs, assignment, chains, gap  track_stitch.py)
  stitch_assign / stitch_chains /                fill)
  stitch_fill_count / stitch_fill_rows
  smooth_filter / smooth_rts                     fixed-interval (RTS) smoothing of     beyond the reference (csrc/smooth.hip,
                                                 every tracklet                        track_smooth.py)
  traffic_lanes / traffic_cells /                flow, density and speed per lane      beyond the reference (csrc/traffic.hip,
  traffic_leaders                                over a grid; leader, gap, headway     traffic_state.py)

The whole-network training call stays one ``torch.autograd.Function`` (modules._NetFn): its inputs are the module's ~200
parameters and its saved state is a Python structure of activations, which is a scheduler, not an operator.
"""
from typing import List, Optional, Tuple

import torch

from . import ops

NS = "retinanet_mi355x"
_lib = torch.library


@_lib.custom_op(NS + "::anchors", mutates_args=(), device_types="cuda")
def anchors(height: int, width: int, device: torch.device) -> torch.Tensor:
    return ops.anchors(height, width, device)


@anchors.register_fake
def _(height, width, device):
    return torch.empty((1, ops.anchor_count(height, width), 4), dtype=torch.float32, device=device)


@_lib.custom_op(NS + "::pairwise_iou", mutates_args=(), device_types="cuda")
def pairwise_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return ops.pairwise_iou(a, b)


@pairwise_iou.register_fake
def _(a, b):
    return a.new_empty((a.shape[0], b.shape[0]), dtype=torch.float32)


# ---- focal loss: forward returns the three losses and the workspace its backward reads
@_lib.custom_op(NS + "::focal_loss_fwd", mutates_args=(), device_types="cuda")
def focal_loss_fwd(cls: torch.Tensor, reg: torch.Tensor, anchor_boxes: torch.Tensor, ann: torch.Tensor,
                   directional: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.focal_loss_forward_raw(cls, reg, anchor_boxes, ann, directional)


@focal_loss_fwd.register_fake
def _(cls, reg, anchor_boxes, ann, directional):
    return cls.new_empty(3, dtype=torch.float32), cls.new_empty(ops.focal_workspace_bytes(cls.shape[0], cls.shape[1]), dtype=torch.uint8)


@_lib.custom_op(NS + "::focal_loss_bwd", mutates_args=(), device_types="cuda")
def focal_loss_bwd(cls: torch.Tensor, reg: torch.Tensor, anchor_boxes: torch.Tensor, ann: torch.Tensor, directional: bool,
                   ws: torch.Tensor, grad_losses: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.focal_loss_backward_raw(cls, reg, anchor_boxes, ann, directional, ws, grad_losses)


@focal_loss_bwd.register_fake
def _(cls, reg, anchor_boxes, ann, directional, ws, grad_losses):
    return torch.empty_like(cls), torch.empty_like(reg)


def _focal_setup(ctx, inputs, output):
    cls, reg, anchor_boxes, ann, directional = inputs
    ctx.save_for_backward(cls, reg, anchor_boxes, ann, output[1])
    ctx.directional = directional


def _focal_backward(ctx, g_losses, g_ws):
    cls, reg, anchor_boxes, ann, ws = ctx.saved_tensors
    dcls, dreg = torch.ops.retinanet_mi355x.focal_loss_bwd(cls, reg, anchor_boxes, ann, ctx.directional, ws, g_losses.contiguous())
    return dcls, dreg, None, None, None


focal_loss_fwd.register_autograd(_focal_backward, setup_context=_focal_setup)


def focal_loss(cls, reg, anchor_boxes, ann, directional=True):
    """(cls_loss[1], reg_loss[1], vp_loss[1]) -- or the first two for the 2D variant -- through the registered operator."""
    ops.check_labels(ann, directional, eager=True)
    losses, _ = torch.ops.retinanet_mi355x.focal_loss_fwd(cls, reg, anchor_boxes, ann, bool(directional))
    out = (losses[0:1], losses[1:2], losses[2:3])
    return out if directional else out[:2]


# ---- decode / clip / nms
@_lib.custom_op(NS + "::decode_dir", mutates_args=(), device_types="cuda")
def decode_dir(anchor_boxes: torch.Tensor, reg: torch.Tensor) -> torch.Tensor:
    return ops.decode_dir(anchor_boxes, reg)


@decode_dir.register_fake
def _(anchor_boxes, reg):
    return reg.new_empty((reg.shape[0], reg.shape[1], 20), dtype=torch.float32)


@_lib.custom_op(NS + "::decode_2d", mutates_args=(), device_types="cuda")
def decode_2d(anchor_boxes: torch.Tensor, deltas: torch.Tensor, clip: bool, height: int, width: int) -> torch.Tensor:
    return ops.decode_2d(anchor_boxes, deltas, clip_hw=(height, width) if clip else None)


@decode_2d.register_fake
def _(anchor_boxes, deltas, clip, height, width):
    return deltas.new_empty(tuple(deltas.shape), dtype=torch.float32)


@_lib.custom_op(NS + "::clip_boxes_", mutates_args=("boxes",), device_types="cuda")
def clip_boxes_(boxes: torch.Tensor, height: int, width: int) -> None:
    ops.clip_boxes_(boxes, height, width)


@_lib.custom_op(NS + "::nms", mutates_args=(), device_types="cuda")
def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    return ops.nms(boxes, scores, iou_threshold)


@nms.register_fake
def _(boxes, scores, iou_threshold):
    n = torch.library.get_ctx().new_dynamic_size()
    return boxes.new_empty((n,), dtype=torch.int64)


@_lib.custom_op(NS + "::linear_sum_assignment", mutates_args=(), device_types="cuda")
def linear_sum_assignment(cost: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.linear_sum_assignment(cost)


@linear_sum_assignment.register_fake
def _(cost):
    n = torch.library.get_ctx().new_dynamic_size()
    return cost.new_empty((n,), dtype=torch.int64), cost.new_empty((n,), dtype=torch.int64)


@_lib.custom_op(NS + "::estimate_ts_bias", mutates_args=("ts_bias",), device_types="cuda")
def estimate_ts_bias(boxes: torch.Tensor, camera_idxs: torch.Tensor, objs: torch.Tensor, timestamps: torch.Tensor,
                     ts_bias: torch.Tensor, phi: float, alpha: float, mu_v: float, max_pairs: int) -> torch.Tensor:
    return ops.estimate_ts_bias(boxes, camera_idxs, objs, timestamps, ts_bias, phi, alpha, mu_v, max_pairs=max_pairs)


@estimate_ts_bias.register_fake
def _(boxes, camera_idxs, objs, timestamps, ts_bias, phi, alpha, mu_v, max_pairs):
    return boxes.new_empty((2,), dtype=torch.int32)


@_lib.custom_op(NS + "::track_crop_prior", mutates_args=(), device_types="cuda")
def track_crop_prior(X: torch.Tensor, D: torch.Tensor, T: torch.Tensor, F: torch.Tensor, centers: torch.Tensor,
                     stamps: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.track_crop_prior(X, D, T, F, centers, stamps, bias)


@track_crop_prior.register_fake
def _(X, D, T, F, centers, stamps, bias):
    n = X.shape[0]
    return X.new_empty((n, 7)), X.new_empty((n,), dtype=torch.int32), X.new_empty((n,), dtype=torch.float64)


# ---- fitting the filter
@_lib.custom_op(NS + "::fit_nearest", mutates_args=(), device_types="cuda")
def fit_nearest(gt: torch.Tensor, det: torch.Tensor, offsets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.fit_nearest(gt, det, offsets)


@fit_nearest.register_fake
def _(gt, det, offsets):
    B = gt.shape[0]
    return gt.new_empty((B,), dtype=torch.int32), gt.new_empty((B, 5), dtype=torch.float32), gt.new_empty((3,), dtype=torch.int32)


@_lib.custom_op(NS + "::residual_moments", mutates_args=(), device_types="cuda")
def residual_moments(E: torch.Tensor, group: Optional[torch.Tensor], groups: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Always the grouped layout (mean [G,k], cov [G,k,k], count [G]); group None = one group."""
    if group is None:
        mean, cov, count = ops.residual_moments(E)
        return mean[None].clone(), cov[None].clone(), count
    return ops.residual_moments(E, group, groups)


@residual_moments.register_fake
def _(E, group, groups):
    G, k = (1 if group is None else groups), E.shape[1]
    return (E.new_empty((G, k), dtype=torch.float32), E.new_empty((G, k, k), dtype=torch.float32),
            E.new_empty((G,), dtype=torch.int32))


# ---- homography
@_lib.custom_op(NS + "::state_to_space", mutates_args=(), device_types="cuda")
def state_to_space(state: torch.Tensor) -> torch.Tensor:
    return ops.hg_state_to_space(state)


@state_to_space.register_fake
def _(state):
    return state.new_empty((state.shape[0], 8, 3), dtype=torch.float32)


@_lib.custom_op(NS + "::state_to_im", mutates_args=(), device_types="cuda")
def state_to_im(state: torch.Tensor, P: torch.Tensor, P2: Optional[torch.Tensor], mat_index: Optional[torch.Tensor]) -> torch.Tensor:
    return ops.hg_to_im(state, P, P2, mat_index, from_state=True)


@state_to_im.register_fake
def _(state, P, P2, mat_index):
    return state.new_empty((state.shape[0], 8, 2), dtype=torch.float64)


@_lib.custom_op(NS + "::im_to_state", mutates_args=(), device_types="cuda")
def im_to_state(im: torch.Tensor, heights: torch.Tensor, H: torch.Tensor, H2: Optional[torch.Tensor],
                mat_index: Optional[torch.Tensor]) -> torch.Tensor:
    return ops.hg_from_im(im, heights, H, H2, mat_index, to_state=True)


@im_to_state.register_fake
def _(im, heights, H, H2, mat_index):
    return im.new_empty((im.shape[0], 6), dtype=torch.float32)


# ---- frame ingest
@_lib.custom_op(NS + "::frame_ingest", mutates_args=(), device_types="cuda")
def frame_ingest(frames_u8: torch.Tensor, swap_rb: bool, nhwc4: bool) -> torch.Tensor:
    return ops.frame_ingest(frames_u8, swap_rb=swap_rb, nhwc4=nhwc4)


@frame_ingest.register_fake
def _(frames_u8, swap_rb, nhwc4):
    B, H, W, _ = frames_u8.shape
    return frames_u8.new_empty((B, H, W, 4) if nhwc4 else (B, 3, H, W), dtype=torch.float32)


@_lib.custom_op(NS + "::frame_ingest_half", mutates_args=(), device_types="cuda")
def frame_ingest_half(frames_u8: torch.Tensor, swap_rb: bool, nhwc4: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """Always with the reduced uint8 frame (the reference's original_im)."""
    return ops.frame_ingest_half(frames_u8, swap_rb=swap_rb, nhwc4=nhwc4, keep_u8=True)


@frame_ingest_half.register_fake
def _(frames_u8, swap_rb, nhwc4):
    B, H2, W2, _ = frames_u8.shape
    H, W = H2 // 2, W2 // 2
    return (frames_u8.new_empty((B, H, W, 4) if nhwc4 else (B, 3, H, W), dtype=torch.float32), frames_u8.new_empty((B, H, W, 3)))


@_lib.custom_op(NS + "::parse_frame_timestamps", mutates_args=(), device_types="cuda")
def parse_frame_timestamps(frames_u8: torch.Tensor, geometry: List[int], tables: torch.Tensor, prev: Optional[torch.Tensor],
                           swap_rb: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """geometry: the rows of ``ops.pack_timestamp_sets`` flattened (9 ints per set); tables: its table on the device.  Always
    with the first set's mask."""
    import numpy as np
    geo = np.asarray(geometry, np.int32).reshape(-1, 9)
    return ops.parse_frame_timestamps(frames_u8, (geo, tables), prev=prev, swap_rb=swap_rb, want_mask=True)


@parse_frame_timestamps.register_fake
def _(frames_u8, geometry, tables, prev, swap_rb):
    B = frames_u8.shape[0]
    w, h, n = geometry[2], geometry[3], geometry[4]
    return (frames_u8.new_empty((B,), dtype=torch.float64), frames_u8.new_empty((B,), dtype=torch.int32),
            frames_u8.new_empty((B,), dtype=torch.int32), frames_u8.new_empty((B, ops.TS_MAX_CELLS), dtype=torch.int8),
            frames_u8.new_empty((B,), dtype=torch.int32), frames_u8.new_empty((B, h, n * w)))


@_lib.custom_op(NS + "::augment_frames", mutates_args=(), device_types="cuda")
def augment_frames(frames_u8: torch.Tensor, records: torch.Tensor, table_x: torch.Tensor, table_y: torch.Tensor,
                   noise: Optional[torch.Tensor], seed: int) -> torch.Tensor:
    return ops.augment_frames(frames_u8, (records, table_x, table_y), noise=noise, seed=seed)


@augment_frames.register_fake
def _(frames_u8, records, table_x, table_y, noise, seed):
    B, H, W, _ = frames_u8.shape
    return frames_u8.new_empty((B, 3, H, W), dtype=torch.float32)


@_lib.custom_op(NS + "::augment_crops", mutates_args=(), device_types="cuda")
def augment_crops(frames_u8: torch.Tensor, records: torch.Tensor, table_x: torch.Tensor, table_y: torch.Tensor,
                  table_cx: torch.Tensor, table_cy: torch.Tensor, K: int, win_max: int, crop: int, noise: Optional[torch.Tensor],
                  occlusion: Optional[torch.Tensor], seed: int) -> torch.Tensor:
    return ops.augment_crops(frames_u8, (records, table_x, table_y, table_cx, table_cy), K, win_max, crop, noise=noise,
                             occlusion=occlusion, seed=seed)


@augment_crops.register_fake
def _(frames_u8, records, table_x, table_y, table_cx, table_cy, K, win_max, crop, noise, occlusion, seed):
    return frames_u8.new_empty((frames_u8.shape[0], 3, crop, crop), dtype=torch.float32)


# ---- detector validation (mAP)
@_lib.custom_op(NS + "::eval_select", mutates_args=("table", "img_rows", "state"), device_types="cuda")
def eval_select(scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor, table: torch.Tensor, img_rows: torch.Tensor,
                state: torch.Tensor, image: int, num_classes: int, score_threshold: float, max_detections: int,
                box_col: int) -> None:
    ops.eval_select(scores, labels, boxes, table, img_rows, state, image, num_classes, score_threshold, max_detections,
                    box_cols=(box_col, box_col + 4))


@_lib.custom_op(NS + "::eval_match", mutates_args=(), device_types="cuda")
def eval_match(table: torch.Tensor, img_rows: torch.Tensor, ann_box: torch.Tensor, ann_offsets: torch.Tensor, num_classes: int,
               iou_threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.eval_match(table, img_rows, ann_box, ann_offsets, num_classes, iou_threshold)


@eval_match.register_fake
def _(table, img_rows, ann_box, ann_offsets, num_classes, iou_threshold):
    return table.new_empty((table.shape[0],), dtype=torch.uint8), table.new_empty((num_classes,), dtype=torch.int32)


@_lib.custom_op(NS + "::eval_ap", mutates_args=(), device_types="cuda")
def eval_ap(table: torch.Tensor, state: torch.Tensor, tp: torch.Tensor, num_annotations: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.eval_ap(table, state, tp, num_annotations)


@eval_ap.register_fake
def _(table, state, tp, num_annotations):
    return (table.new_empty((num_annotations.shape[0],), dtype=torch.float64), table.new_empty((table.shape[0],), dtype=torch.int32))


# ---- detector validation in 3D (cuboid AP, corner errors)
@_lib.custom_op(NS + "::eval_corners", mutates_args=("corners",), device_types="cuda")
def eval_corners(boxes: torch.Tensor, table: torch.Tensor, img_rows: torch.Tensor, image: int, corners: torch.Tensor) -> None:
    ops.eval_corners(boxes, table, img_rows, image, corners)


@_lib.custom_op(NS + "::eval_cuboid_overlap", mutates_args=(), device_types="cuda")
def eval_cuboid_overlap(table: torch.Tensor, img_rows: torch.Tensor, corners: torch.Tensor, ann_corners: torch.Tensor,
                        ann_offsets: torch.Tensor, num_classes: int, overlap: str) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.eval_cuboid_overlap(table, img_rows, corners, ann_corners, ann_offsets, num_classes, overlap)


@eval_cuboid_overlap.register_fake
def _(table, img_rows, corners, ann_corners, ann_offsets, num_classes, overlap):
    return table.new_empty((table.shape[0],), dtype=torch.float64), table.new_empty((table.shape[0],), dtype=torch.int32)


@_lib.custom_op(NS + "::eval_cuboid_assign", mutates_args=(), device_types="cuda")
def eval_cuboid_assign(table: torch.Tensor, img_rows: torch.Tensor, best_iou: torch.Tensor, best_ann: torch.Tensor,
                       ann_offsets: torch.Tensor, num_annotated: int, num_classes: int,
                       thresholds: List[float]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.eval_cuboid_assign(table, img_rows, best_iou, best_ann, ann_offsets, num_annotated, num_classes, thresholds)


@eval_cuboid_assign.register_fake
def _(table, img_rows, best_iou, best_ann, ann_offsets, num_annotated, num_classes, thresholds):
    rows = table.shape[0]
    return (table.new_empty((len(thresholds), rows), dtype=torch.uint8), table.new_empty((num_classes,), dtype=torch.int32),
            table.new_empty((rows,), dtype=torch.int32))


@_lib.custom_op(NS + "::eval_cuboid_errors", mutates_args=(), device_types="cuda")
def eval_cuboid_errors(table: torch.Tensor, state: torch.Tensor, img_rows: torch.Tensor, corners: torch.Tensor,
                       ann_corners: torch.Tensor, ann_offsets: torch.Tensor, num_classes: int, tp: torch.Tensor,
                       matched: torch.Tensor, best_iou: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.eval_cuboid_errors(table, state, img_rows, corners, ann_corners, ann_offsets, num_classes, tp, matched, best_iou)


@eval_cuboid_errors.register_fake
def _(table, state, img_rows, corners, ann_corners, ann_offsets, num_classes, tp, matched, best_iou):
    return table.new_empty((table.shape[0], 4), dtype=torch.float64), table.new_empty((num_classes, 5), dtype=torch.float64)


# ---- tracking evaluation (MOT metrics): the per-frame counts travel as host int lists, as ops.mot_offsets takes them
def _mot_layout(n_gt, n_pred, device):
    return ops.mot_offsets(n_gt, n_pred, device)


@_lib.custom_op(NS + "::mot_prepare", mutates_args=(), device_types="cuda")
def mot_prepare(gt_im: torch.Tensor, gt_h0: torch.Tensor, gt_vel: torch.Tensor, pred_state: torch.Tensor, H: torch.Tensor,
                P: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.mot_prepare(gt_im, gt_h0, gt_vel, pred_state, H, P)


@mot_prepare.register_fake
def _(gt_im, gt_h0, gt_vel, pred_state, H, P):
    G, M = gt_im.shape[0], pred_state.shape[0]
    return (gt_im.new_empty((G, 7), dtype=torch.float32), gt_im.new_empty((G, 4), dtype=torch.float32),
            gt_im.new_empty((M, 4), dtype=torch.float32), gt_im.new_empty((M, 8, 2), dtype=torch.float64))


@_lib.custom_op(NS + "::mot_iou", mutates_args=(), device_types="cuda")
def mot_iou(gt_box: torch.Tensor, pred_box: torch.Tensor, n_gt: List[int], n_pred: List[int]) -> torch.Tensor:
    offsets, totals = _mot_layout(n_gt, n_pred, gt_box.device)
    return ops.mot_iou(gt_box, pred_box, offsets, totals)


@mot_iou.register_fake
def _(gt_box, pred_box, n_gt, n_pred):
    return gt_box.new_empty((sum(a * b for a, b in zip(n_gt, n_pred)),), dtype=torch.float64)


@_lib.custom_op(NS + "::mot_assign", mutates_args=(), device_types="cuda")
def mot_assign(iou: torch.Tensor, n_gt: List[int], n_pred: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    offsets, totals = _mot_layout(n_gt, n_pred, iou.device)
    return ops.mot_assign(iou, offsets, totals, sum(n_pred))


@mot_assign.register_fake
def _(iou, n_gt, n_pred):
    S = sum(min(a, b) for a, b in zip(n_gt, n_pred))
    return (iou.new_empty((S,), dtype=torch.int32), iou.new_empty((S,), dtype=torch.int32),
            iou.new_empty((sum(n_pred),), dtype=torch.uint8), iou.new_empty((len(n_gt),), dtype=torch.int32))


@_lib.custom_op(NS + "::mot_frame_metrics", mutates_args=(), device_types="cuda")
def mot_frame_metrics(iou: torch.Tensor, n_gt: List[int], n_pred: List[int], slot_row: torch.Tensor, slot_col: torch.Tensor,
                      pred_assigned: torch.Tensor, frame_status: torch.Tensor, match_iou: float, gt_state: torch.Tensor,
                      pred_state: torch.Tensor, gt_im: torch.Tensor, pred_im: torch.Tensor, gt_cls: torch.Tensor,
                      pred_cls: torch.Tensor, gt_id: torch.Tensor, pred_id: torch.Tensor) -> List[torch.Tensor]:
    offsets, totals = _mot_layout(n_gt, n_pred, iou.device)
    return list(ops.mot_frame_metrics(iou, offsets, totals, (slot_row, slot_col, pred_assigned, frame_status), match_iou, gt_state,
                                      pred_state, gt_im, pred_im, gt_cls, pred_cls, gt_id, pred_id))


@mot_frame_metrics.register_fake
def _(iou, n_gt, n_pred, slot_row, slot_col, pred_assigned, frame_status, match_iou, gt_state, pred_state, gt_im, pred_im, gt_cls,
      pred_cls, gt_id, pred_id):
    S, F = slot_row.shape[0], len(n_gt)
    e = iou.new_empty
    return [e((S,), dtype=torch.float64), e((S,), dtype=torch.int32), e((S,), dtype=torch.int32), e((S, 7), dtype=torch.float32),
            e((S,), dtype=torch.float64), e((S,), dtype=torch.float64), e((S,), dtype=torch.uint8), e((F,), dtype=torch.int32),
            e((F,), dtype=torch.int32)]


@_lib.custom_op(NS + "::mot_reduce", mutates_args=(), device_types="cuda")
def mot_reduce(n_gt: List[int], n_pred: List[int], slot_row: torch.Tensor, slot_col: torch.Tensor, pred_assigned: torch.Tensor,
               frame_status: torch.Tensor, per_slot: List[torch.Tensor], gt_id: torch.Tensor, pred_id: torch.Tensor, n_gid: int,
               n_pid: int) -> torch.Tensor:
    offsets, totals = _mot_layout(n_gt, n_pred, gt_id.device)
    return ops.mot_reduce(offsets, totals, (slot_row, slot_col, pred_assigned, frame_status), tuple(per_slot), gt_id, pred_id,
                          n_gid, n_pid)


@mot_reduce.register_fake
def _(n_gt, n_pred, slot_row, slot_col, pred_assigned, frame_status, per_slot, gt_id, pred_id, n_gid, n_pid):
    return gt_id.new_empty((ops.MOT_RESULT,), dtype=torch.float64)


# ---- identity and association scores (IDF1, HOTA): the same host int lists for the layout
@_lib.custom_op(NS + "::mot_id_counts", mutates_args=(), device_types="cuda")
def mot_id_counts(iou: torch.Tensor, n_gt: List[int], n_pred: List[int], gt_id: torch.Tensor, pred_id: torch.Tensor, n_gid: int,
                  n_pid: int, id_iou: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    offsets, totals = _mot_layout(n_gt, n_pred, iou.device)
    return ops.mot_id_counts(iou, offsets, totals, gt_id, pred_id, n_gid, n_pid, id_iou)


@mot_id_counts.register_fake
def _(iou, n_gt, n_pred, gt_id, pred_id, n_gid, n_pid, id_iou):
    e = iou.new_empty
    return (e((n_gid,), dtype=torch.int32), e((n_pid,), dtype=torch.int32), e((n_gid, n_pid), dtype=torch.int32),
            e((2,), dtype=torch.int32))


@_lib.custom_op(NS + "::mot_id_assign", mutates_args=(), device_types="cuda")
def mot_id_assign(C: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.mot_id_assign(C)


@mot_id_assign.register_fake
def _(C):
    return C.new_empty((C.shape[0],), dtype=torch.int32), C.new_empty((2,), dtype=torch.int64)


@_lib.custom_op(NS + "::mot_hota_align", mutates_args=(), device_types="cuda")
def mot_hota_align(iou: torch.Tensor, n_gt: List[int], n_pred: List[int], gt_id: torch.Tensor, pred_id: torch.Tensor,
                   csr_off: torch.Tensor, csr_frame: torch.Tensor, csr_row: torch.Tensor, n_gid: int,
                   n_pid: int) -> Tuple[torch.Tensor, torch.Tensor]:
    offsets, totals = _mot_layout(n_gt, n_pred, iou.device)
    return ops.mot_hota_align(iou, offsets, totals, gt_id, pred_id, (csr_off, csr_frame, csr_row), n_gid, n_pid)


@mot_hota_align.register_fake
def _(iou, n_gt, n_pred, gt_id, pred_id, csr_off, csr_frame, csr_row, n_gid, n_pid):
    return iou.new_empty((n_gid, n_pid), dtype=torch.float64), iou.new_empty((2,), dtype=torch.int32)


@_lib.custom_op(NS + "::mot_hota_assign", mutates_args=(), device_types="cuda")
def mot_hota_assign(iou: torch.Tensor, n_gt: List[int], n_pred: List[int], gt_id: torch.Tensor, pred_id: torch.Tensor,
                    gc: torch.Tensor, pc: torch.Tensor, pot: torch.Tensor,
                    alphas: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    offsets, totals = _mot_layout(n_gt, n_pred, iou.device)
    return ops.mot_hota_assign(iou, offsets, totals, gt_id, pred_id, gc, pc, pot, alphas)


@mot_hota_assign.register_fake
def _(iou, n_gt, n_pred, gt_id, pred_id, gc, pc, pot, alphas):
    S, e = sum(min(a, b) for a, b in zip(n_gt, n_pred)), iou.new_empty
    return (e((S,), dtype=torch.int32), e((S,), dtype=torch.int32), e((S,), dtype=torch.float64), e((S,), dtype=torch.int32),
            e((len(n_gt),), dtype=torch.int32))


@_lib.custom_op(NS + "::mot_hota_reduce", mutates_args=(), device_types="cuda")
def mot_hota_reduce(n_gt: List[int], n_pred: List[int], slot_row: torch.Tensor, slot_col: torch.Tensor, slot_s: torch.Tensor,
                    slot_n: torch.Tensor, frame_status: torch.Tensor, gt_id: torch.Tensor, pred_id: torch.Tensor, gc: torch.Tensor,
                    pc: torch.Tensor) -> torch.Tensor:
    offsets, totals = _mot_layout(n_gt, n_pred, gt_id.device)
    return ops.mot_hota_reduce(offsets, totals, (slot_row, slot_col, slot_s, slot_n, frame_status), gt_id, pred_id, gc, pc)


@mot_hota_reduce.register_fake
def _(n_gt, n_pred, slot_row, slot_col, slot_s, slot_n, frame_status, gt_id, pred_id, gc, pc):
    return gt_id.new_empty((ops.MOT_ASSOC_RESULT,), dtype=torch.float64)


# ---- camera calibration
@_lib.custom_op(NS + "::vanishing_points", mutates_args=(), device_types="cuda")
def vanishing_points(lines: torch.Tensor, offsets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.vanishing_points(lines, offsets)


@vanishing_points.register_fake
def _(lines, offsets):
    S = offsets.shape[0] - 1
    return (lines.new_empty((S, 3), dtype=torch.float64), lines.new_empty((S, ops.VP_LEVELS, 3), dtype=torch.float64),
            lines.new_empty((S,), dtype=torch.int32))


@_lib.custom_op(NS + "::hg_reproj_error", mutates_args=(), device_types="cuda")
def hg_reproj_error(boxes: torch.Tensor, heights: torch.Tensor, H: torch.Tensor, P_orig: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    return ops.hg_reproj_error(boxes, heights, H, P_orig, C)


@hg_reproj_error.register_fake
def _(boxes, heights, H, P_orig, C):
    return boxes.new_empty((C.shape[0], 2), dtype=torch.float64)


@_lib.custom_op(NS + "::hg_scale_z", mutates_args=(), device_types="cuda")
def hg_scale_z(boxes: torch.Tensor, heights: torch.Tensor, H: torch.Tensor, P_orig: torch.Tensor, granularity: float,
               max_scale: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.hg_scale_z(boxes, heights, H, P_orig, granularity, max_scale)


@hg_scale_z.register_fake
def _(boxes, heights, H, P_orig, granularity, max_scale):
    return (boxes.new_empty((ops.SZ_MAX_ITERS, 10, 2), dtype=torch.float64), boxes.new_empty((3,), dtype=torch.float64),
            boxes.new_empty((2,), dtype=torch.int32))


@_lib.custom_op(NS + "::fit_homography", mutates_args=(), device_types="cuda")
def fit_homography(src: torch.Tensor, dst: torch.Tensor, offsets: torch.Tensor, refine: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.fit_homography(src, dst, offsets, refine)


@fit_homography.register_fake
def _(src, dst, offsets, refine):
    B = offsets.shape[0] - 1
    return src.new_empty((B, 3, 3), dtype=torch.float64), src.new_empty((B,), dtype=torch.int32)


# ---- tracking CSV resampling and rewrite: every op returns the status word last (ops.reinterp_check raises on it)
@_lib.custom_op(NS + "::reinterp_mate", mutates_args=(), device_types="cuda")
def reinterp_mate(offsets: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.reinterp_mate(offsets, ids)


@reinterp_mate.register_fake
def _(offsets, ids):
    return ids.new_empty((ids.shape[0],), dtype=torch.int32), ids.new_empty((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::reinterp_offsets", mutates_args=(), device_types="cuda")
def reinterp_offsets(offsets: torch.Tensor, mate: torch.Tensor, inst_a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.reinterp_offsets(offsets, mate, inst_a)


@reinterp_offsets.register_fake
def _(offsets, mate, inst_a):
    T = inst_a.shape[0]
    return (mate.new_empty((T,), dtype=torch.int32), mate.new_empty((T + 1,), dtype=torch.int64), mate.new_empty((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::reinterp_rows", mutates_args=(), device_types="cuda")
def reinterp_rows(offsets: torch.Tensor, frame_ts: torch.Tensor, fields: torch.Tensor, mate: torch.Tensor, inst_a: torch.Tensor,
                  inst_time: torch.Tensor, prefix: torch.Tensor, rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.reinterp_rows(offsets, frame_ts, fields, mate, inst_a, inst_time, prefix, rows)


@reinterp_rows.register_fake
def _(offsets, frame_ts, fields, mate, inst_a, inst_time, prefix, rows):
    e = fields.new_empty
    return e((rows, 6), dtype=torch.float64), e((rows,), dtype=torch.int32), e((rows,), dtype=torch.int32), e((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::track_rows", mutates_args=(), device_types="cuda")
def track_rows(fields: torch.Tensor, direction: torch.Tensor, P: torch.Tensor, P2: Optional[torch.Tensor],
               mat_index: Optional[torch.Tensor]) -> List[torch.Tensor]:
    return list(ops.track_rows(fields, direction, P, P2, mat_index))


@track_rows.register_fake
def _(fields, direction, P, P2, mat_index):
    N, e = direction.shape[0], fields.new_empty
    return [e((N, 7), dtype=torch.float32), e((N, 4, 2), dtype=torch.float32), e((N, 8, 2), dtype=torch.float64),
            e((N, 4), dtype=torch.float64), e((N,), dtype=torch.uint8), e((1,), dtype=torch.int32)]


OPERATORS = ("anchors", "pairwise_iou", "focal_loss_fwd", "focal_loss_bwd", "decode_dir", "decode_2d", "clip_boxes_", "nms",
             "linear_sum_assignment", "estimate_ts_bias", "track_crop_prior", "fit_nearest", "residual_moments", "state_to_space", "state_to_im", "im_to_state", "frame_ingest", "frame_ingest_half", "parse_frame_timestamps", "augment_frames", "augment_crops",
             "eval_select", "eval_match", "eval_ap", "mot_prepare", "mot_iou", "mot_assign", "mot_frame_metrics", "mot_reduce",
             "vanishing_points", "hg_reproj_error", "hg_scale_z", "fit_homography", "reinterp_mate", "reinterp_offsets", "reinterp_rows",
             "track_rows", "render_edges", "render_rects", "render_text", "render_compose")
OPERATORS += ("mot_id_counts", "mot_id_assign", "mot_hota_align", "mot_hota_assign", "mot_hota_reduce")
OPERATORS += ("eval_corners", "eval_cuboid_overlap", "eval_cuboid_assign", "eval_cuboid_errors")


# ---- output frames: the painters OR into the mask plane in place
@_lib.custom_op(NS + "::render_edges", mutates_args=("mask",), device_types="cuda")
def render_edges(corners: torch.Tensor, cam: torch.Tensor, thickness: int, bit: int, mask: torch.Tensor) -> None:
    ops.render_edges(corners, cam, thickness, bit, mask)


@_lib.custom_op(NS + "::render_rects", mutates_args=("mask",), device_types="cuda")
def render_rects(rects: torch.Tensor, mask: torch.Tensor, anchors: Optional[torch.Tensor]) -> None:
    ops.render_rects(rects, mask, anchors)


@_lib.custom_op(NS + "::render_text", mutates_args=("mask",), device_types="cuda")
def render_text(runs: torch.Tensor, text: torch.Tensor, font: torch.Tensor, mask: torch.Tensor, anchors: Optional[torch.Tensor]) -> None:
    ops.render_text(runs, text, font, mask, anchors)


@_lib.custom_op(NS + "::render_compose", mutates_args=(), device_types="cuda")
def render_compose(frames: torch.Tensor, mask: torch.Tensor, crops_present: bool, cols: int) -> torch.Tensor:
    return ops.render_compose(frames, mask, crops_present, cols)


@render_compose.register_fake
def _(frames, mask, crops_present, cols):
    n_cam, H, W = mask.shape
    return frames.new_empty((-(-n_cam // cols) * H, cols * W, 3), dtype=torch.uint8)


# ---- tracking CSV replay (csrc/replay.hip)
OPERATORS += ("replay_boxes", "replay_compose", "frame_absdiff", "running_frame")


@_lib.custom_op(NS + "::replay_boxes", mutates_args=(), device_types="cuda")
def replay_boxes(state7: torch.Tensor, dt: torch.Tensor, P1: torch.Tensor, P2: Optional[torch.Tensor], offset: int,
                 count: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.replay_boxes(state7, dt, P1, P2, offset, count)


@replay_boxes.register_fake
def _(state7, dt, P1, P2, offset, count):
    m, e = dt.shape[0] * count, state7.new_empty
    return e((m, 7), dtype=torch.float32), e((m, 8, 2), dtype=torch.float64), e((m,), dtype=torch.int32), e((m,), dtype=torch.int32)


@_lib.custom_op(NS + "::replay_compose", mutates_args=(), device_types="cuda")
def replay_compose(frames: torch.Tensor, mask: torch.Tensor, width: int, height: int, swap_rb: bool) -> torch.Tensor:
    return ops.replay_compose(frames, mask, (width, height), swap_rb)


@replay_compose.register_fake
def _(frames, mask, width, height, swap_rb):
    return frames.new_empty((height, width, 3), dtype=torch.uint8)


@_lib.custom_op(NS + "::frame_absdiff", mutates_args=(), device_types="cuda")
def frame_absdiff(a: torch.Tensor, b: torch.Tensor, y0: int, y1: int, x0: int, x1: int) -> torch.Tensor:
    return ops.frame_absdiff(a, b, y0, y1, x0, x1)


@frame_absdiff.register_fake
def _(a, b, y0, y1, x0, x1):
    return a.new_empty((1,), dtype=torch.int64)


@_lib.custom_op(NS + "::running_frame", mutates_args=("running",), device_types="cuda")
def running_frame(running: torch.Tensor, frame: torch.Tensor, first: bool) -> None:
    ops.running_frame(running, frame, first)


# ---- multi-camera label audit (csrc/label_audit.hip): every op returns the status word last (ops.label_check raises on it)
OPERATORS += ("label_pair_samples", "label_outliers", "label_interpolate")


@_lib.custom_op(NS + "::label_pair_samples", mutates_args=(), device_types="cuda")
def label_pair_samples(offsets: torch.Tensor, cols: torch.Tensor, n_cam: int, key_col: int, val0: int,
                       val1: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.label_pair_samples(offsets, cols, n_cam, key_col, val0, val1)


@label_pair_samples.register_fake
def _(offsets, cols, n_cam, key_col, val0, val1):
    P, n, e = n_cam * (n_cam - 1) // 2, (offsets.shape[0] - 1) // n_cam, cols.new_empty
    return (e((P, n, ops.LABEL_POINTS), dtype=torch.uint8), e((P, n, ops.LABEL_POINTS, 4), dtype=torch.float64),
            e((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::label_outliers", mutates_args=(), device_types="cuda")
def label_outliers(offsets: torch.Tensor, cols: torch.Tensor, frame: torch.Tensor, n_frames: int,
                   n_visit: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.label_outliers(offsets, cols, frame, n_frames, n_visit)


@label_outliers.register_fake
def _(offsets, cols, frame, n_frames, n_visit):
    return cols.new_empty((cols.shape[0],), dtype=torch.uint8), cols.new_empty((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::label_interpolate", mutates_args=(), device_types="cuda")
def label_interpolate(offsets: torch.Tensor, cols: torch.Tensor, frame: torch.Tensor, all_ts: torch.Tensor,
                      rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.label_interpolate(offsets, cols, frame, all_ts, rows)


@label_interpolate.register_fake
def _(offsets, cols, frame, all_ts, rows):
    e = cols.new_empty
    return (e((rows, 3), dtype=torch.float64), e((rows,), dtype=torch.int32), e((rows,), dtype=torch.int32),
            e((1,), dtype=torch.int64), e((1,), dtype=torch.int32))


# ---- re-basing labels (csrc/label_rebase.hip): label_rebase returns the status word last, like the audit's ops
OPERATORS += ("label_rebase", "label_offset_y")


@_lib.custom_op(NS + "::label_rebase", mutates_args=(), device_types="cuda")
def label_rebase(state6: torch.Tensor, cam: torch.Tensor, P1_old: torch.Tensor, P2_old: Optional[torch.Tensor],
                 P1_new: torch.Tensor, P2_new: Optional[torch.Tensor], radii: torch.Tensor,
                 grid: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.label_rebase(state6, cam, P1_old, P2_old, P1_new, P2_new, radii, grid)


@label_rebase.register_fake
def _(state6, cam, P1_old, P2_old, P1_new, P2_new, radii, grid):
    n, e = state6.shape[0], state6.new_empty
    return (e((n, 2), dtype=torch.float64), e((n,), dtype=torch.float64), e((n, radii.shape[0]), dtype=torch.int32),
            e((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::label_offset_y", mutates_args=(), device_types="cuda")
def label_offset_y(xy: torch.Tensor, coef: torch.Tensor, y_straight: torch.Tensor, direction: torch.Tensor,
                   reverse: bool) -> torch.Tensor:
    return ops.label_offset_y(xy, coef, y_straight, direction, reverse)


@label_offset_y.register_fake
def _(xy, coef, y_straight, direction, reverse):
    return xy.new_empty((xy.shape[0],), dtype=torch.float64)


# ---- detector-assisted labelling (csrc/label_assist.hip): the status word of the audit comes last where an op has one
OPERATORS += ("label_crop_windows", "label_best_anchor", "label_fit_box2d")


@_lib.custom_op(NS + "::label_crop_windows", mutates_args=(), device_types="cuda")
def label_crop_windows(state6: torch.Tensor, cam: torch.Tensor, P1: torch.Tensor, P2: Optional[torch.Tensor], ber: float,
                       width: float, height: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.label_crop_windows(state6, cam, P1, P2, ber, width, height)


@label_crop_windows.register_fake
def _(state6, cam, P1, P2, ber, width, height):
    n, e = state6.shape[0], state6.new_empty
    return (e((n, 4), dtype=torch.float32), e((n, 5), dtype=torch.float32), e((n, 3), dtype=torch.float32),
            e((n,), dtype=torch.uint8), e((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::label_best_anchor", mutates_args=(), device_types="cuda")
def label_best_anchor(cls: torch.Tensor, reg: torch.Tensor, win: torch.Tensor,
                      cs: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.label_best_anchor(cls, reg, win, cs)


@label_best_anchor.register_fake
def _(cls, reg, win, cs):
    n, e = cls.shape[0], cls.new_empty
    return (e((n, 4), dtype=torch.float32), e((n,), dtype=torch.int32), e((n,), dtype=torch.float32), e((n,), dtype=torch.int32))


@_lib.custom_op(NS + "::label_fit_box2d", mutates_args=(), device_types="cuda")
def label_fit_box2d(tmpl: torch.Tensor, cam: torch.Tensor, centre: torch.Tensor, target: torch.Tensor, P1: torch.Tensor,
                    P2: Optional[torch.Tensor], radii: torch.Tensor, grid: int,
                    skip: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, radii, grid, skip)


@label_fit_box2d.register_fake
def _(tmpl, cam, centre, target, P1, P2, radii, grid, skip):
    n, e = tmpl.shape[0], tmpl.new_empty
    return (e((n, 2), dtype=torch.float32), e((n,), dtype=torch.float32), e((n, radii.shape[0]), dtype=torch.int32),
            e((1,), dtype=torch.int32))


# ---- spline trajectories (csrc/label_spline.hip): the status word of the audit comes last where an op has one
OPERATORS += ("label_box_weights", "spline_fit", "spline_select", "spline_eval", "label_ts_shift")


@_lib.custom_op(NS + "::label_box_weights", mutates_args=(), device_types="cuda")
def label_box_weights(state6: torch.Tensor, cam: torch.Tensor, P1: torch.Tensor,
                      P2: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.label_box_weights(state6, cam, P1, P2)


@label_box_weights.register_fake
def _(state6, cam, P1, P2):
    return state6.new_empty((state6.shape[0], 4), dtype=torch.float64), state6.new_empty((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::spline_fit", mutates_args=(), device_types="cuda")
def spline_fit(grp: torch.Tensor, waves: torch.Tensor, tx: torch.Tensor, val: torch.Tensor, wt: torch.Tensor, s: torch.Tensor,
               ncap: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.spline_fit(grp, waves, tx, val, wt, s, ncap)


@spline_fit.register_fake
def _(grp, waves, tx, val, wt, s, ncap):
    NL, e = waves.shape[0] * 64, tx.new_empty
    return (e((ops.SPLINE_WS_COLS * ncap, NL), dtype=torch.float64), e((NL,), dtype=torch.int32), e((NL,), dtype=torch.int32),
            e((NL,), dtype=torch.float64), e((NL,), dtype=torch.int32), e((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::spline_select", mutates_args=(), device_types="cuda")
def spline_select(grp: torch.Tensor, tx: torch.Tensor, val: torch.Tensor, wt: torch.Tensor, wscore: torch.Tensor, n_cand: int,
                  ncap: int, workspace: torch.Tensor, n: torch.Tensor, ier: torch.Tensor, fp: torch.Tensor,
                  metric: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.spline_select(grp, tx, val, wt, wscore, n_cand, ncap, workspace, n, ier, fp, metric)


@spline_select.register_fake
def _(grp, tx, val, wt, wscore, n_cand, ncap, workspace, n, ier, fp, metric):
    G, e = grp.shape[0], tx.new_empty
    return (e((n_cand,), dtype=torch.float64), e((G, 3), dtype=torch.int32), e((G, ops.SPLINE_FIGS), dtype=torch.float64),
            e((G, ncap), dtype=torch.float64), e((G, ncap), dtype=torch.float64), e((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::spline_eval", mutates_args=(), device_types="cuda")
def spline_eval(st: torch.Tensor, sc: torch.Tensor, snk: torch.Tensor, qs: torch.Tensor, qt: torch.Tensor) -> torch.Tensor:
    return ops.spline_eval(st, sc, snk, qs, qt)


@spline_eval.register_fake
def _(st, sc, snk, qs, qt):
    return qt.new_empty((qs.shape[0],), dtype=torch.float64)


@_lib.custom_op(NS + "::label_ts_shift", mutates_args=(), device_types="cuda")
def label_ts_shift(st: torch.Tensor, sc: torch.Tensor, snk: torch.Tensor, off: torch.Tensor, rs: torch.Tensor, rx: torch.Tensor,
                   base: torch.Tensor, run: torch.Tensor, shifts: torch.Tensor, use_run: bool,
                   metric: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.label_ts_shift(st, sc, snk, off, rs, rx, base, run, shifts, use_run, metric)


@label_ts_shift.register_fake
def _(st, sc, snk, off, rs, rx, base, run, shifts, use_run, metric):
    E, e = base.shape[0], base.new_empty
    return (e((E,), dtype=torch.float64), e((E, 2), dtype=torch.float64), e((E,), dtype=torch.int32), e((1,), dtype=torch.int32))


# ---- track stitching (csrc/stitch.hip, beyond the reference: track_stitch.py): the status word comes last where an op has one;
# scales = the seven floats of ops.STITCH_SCALES
OPERATORS += ("stitch_endpoints", "stitch_costs", "stitch_candidates", "stitch_compact", "stitch_assign", "stitch_chains",
              "stitch_fill_count", "stitch_fill_rows")


@_lib.custom_op(NS + "::stitch_endpoints", mutates_args=(), device_types="cuda")
def stitch_endpoints(offsets: torch.Tensor, cols: torch.Tensor, direction: torch.Tensor, fit_n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.stitch_endpoints(offsets, cols, direction, fit_n)


@stitch_endpoints.register_fake
def _(offsets, cols, direction, fit_n):
    return cols.new_empty((offsets.shape[0] - 1, 2, ops.STITCH_EP), dtype=torch.float64), cols.new_empty((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::stitch_costs", mutates_args=(), device_types="cuda")
def stitch_costs(ep: torch.Tensor, scales: List[float]) -> torch.Tensor:
    return ops.stitch_costs(ep, scales)


@stitch_costs.register_fake
def _(ep, scales):
    return ep.new_empty((ep.shape[0], ep.shape[0]), dtype=torch.float64)


@_lib.custom_op(NS + "::stitch_candidates", mutates_args=(), device_types="cuda")
def stitch_candidates(ep: torch.Tensor, scales: List[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.stitch_candidates(ep, scales)


@stitch_candidates.register_fake
def _(ep, scales):
    return ep.new_empty((2, 2, ep.shape[0]), dtype=torch.int32), ep.new_empty((4,), dtype=torch.int32)


@_lib.custom_op(NS + "::stitch_compact", mutates_args=(), device_types="cuda")
def stitch_compact(ep: torch.Tensor, scales: List[float], cand: torch.Tensor, ncand: torch.Tensor, cap: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.stitch_compact(ep, scales, cand, ncand, cap)


@stitch_compact.register_fake
def _(ep, scales, cand, ncand, cap):
    return ep.new_empty((cap,), dtype=torch.float64), ep.new_empty((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::stitch_assign", mutates_args=(), device_types="cuda")
def stitch_assign(ep: torch.Tensor, scales: List[float], cand: torch.Tensor, ncand: torch.Tensor,
                  Wc: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.stitch_assign(ep, scales, cand, ncand, Wc)


@stitch_assign.register_fake
def _(ep, scales, cand, ncand, Wc):
    N, e = ep.shape[0], ep.new_empty
    return e((N,), dtype=torch.int32), e((N,), dtype=torch.int32), e((N,), dtype=torch.float64), e((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::stitch_chains", mutates_args=(), device_types="cuda")
def stitch_chains(prev: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.stitch_chains(prev, ids)


@stitch_chains.register_fake
def _(prev, ids):
    N, e = prev.shape[0], prev.new_empty
    return e((N,), dtype=torch.int32), e((N,), dtype=torch.int32), e((N,), dtype=torch.int64), e((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::stitch_fill_count", mutates_args=(), device_types="cuda")
def stitch_fill_count(ep: torch.Tensor, nxt: torch.Tensor, fill_rate: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.stitch_fill_count(ep, nxt, fill_rate)


@stitch_fill_count.register_fake
def _(ep, nxt, fill_rate):
    N, e = ep.shape[0], ep.new_empty
    return e((N,), dtype=torch.int32), e((N + 1,), dtype=torch.int64), e((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::stitch_fill_rows", mutates_args=(), device_types="cuda")
def stitch_fill_rows(ep: torch.Tensor, nxt: torch.Tensor, prefix: torch.Tensor, fill_rate: float,
                     rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.stitch_fill_rows(ep, nxt, prefix, fill_rate, rows)


@stitch_fill_rows.register_fake
def _(ep, nxt, prefix, fill_rate, rows):
    e = ep.new_empty
    return (e((rows, 6), dtype=torch.float64), e((rows,), dtype=torch.float64), e((rows,), dtype=torch.int32), e((rows,), dtype=torch.uint8),
            e((1,), dtype=torch.int32))


# ---- fixed-interval smoothing (csrc/smooth.hip, beyond the reference: track_smooth.py): the status word comes last
OPERATORS += ("smooth_filter", "smooth_rts")


@_lib.custom_op(NS + "::smooth_filter", mutates_args=(), device_types="cuda")
def smooth_filter(offsets: torch.Tensor, order: torch.Tensor, cols: torch.Tensor, direction: torch.Tensor, model: torch.Tensor,
                  gate: float, dt_default: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.smooth_filter(offsets, order, cols, direction, model, gate, dt_default)


@smooth_filter.register_fake
def _(offsets, order, cols, direction, model, gate, dt_default):
    R, e = cols.shape[0], cols.new_empty
    return (e((R, ops.SMOOTH_FILT), dtype=torch.float64), e((R,), dtype=torch.float64), e((R,), dtype=torch.uint8),
            e((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::smooth_rts", mutates_args=(), device_types="cuda")
def smooth_rts(offsets: torch.Tensor, order: torch.Tensor, cols: torch.Tensor, direction: torch.Tensor, model: torch.Tensor,
               dt_default: float, filt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.smooth_rts(offsets, order, cols, direction, model, dt_default, filt)


@smooth_rts.register_fake
def _(offsets, order, cols, direction, model, dt_default, filt):
    return cols.new_empty((cols.shape[0], ops.SMOOTH_OUT), dtype=torch.float64), cols.new_empty((1,), dtype=torch.int32)


# ---- traffic state (csrc/traffic.hip, beyond the reference: traffic_state.py): the status word comes last
OPERATORS += ("traffic_lanes", "traffic_cells", "traffic_leaders")


@_lib.custom_op(NS + "::traffic_lanes", mutates_args=(), device_types="cuda")
def traffic_lanes(offsets: torch.Tensor, cols: torch.Tensor, direction: torch.Tensor, edges_pos: torch.Tensor,
                  edges_neg: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.traffic_lanes(offsets, cols, direction, edges_pos, edges_neg)


@traffic_lanes.register_fake
def _(offsets, cols, direction, edges_pos, edges_neg):
    e = cols.new_empty
    return e((offsets.shape[0] - 1,), dtype=torch.int32), e((cols.shape[0],), dtype=torch.int32), e((1,), dtype=torch.int32)


@_lib.custom_op(NS + "::traffic_cells", mutates_args=(), device_types="cuda")
def traffic_cells(offsets: torch.Tensor, cols: torch.Tensor, dir: torch.Tensor, edges_pos: torch.Tensor, edges_neg: torch.Tensor,
                  t0: float, dt: float, nt: int, x0: float, dx: float, nx: int,
                  max_gap: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.traffic_cells(offsets, cols, dir, edges_pos, edges_neg, t0, dt, nt, x0, dx, nx, max_gap)


@traffic_cells.register_fake
def _(offsets, cols, dir, edges_pos, edges_neg, t0, dt, nt, x0, dx, nx, max_gap):
    e, shape = cols.new_empty, (2, max(edges_pos.shape[0], edges_neg.shape[0], 1) - 1, nt, nx)
    return (e(shape, dtype=torch.int64), e(shape, dtype=torch.int64), e(shape, dtype=torch.int32),
            e((ops.TRAFFIC_COUNTERS,), dtype=torch.int64), e((1,), dtype=torch.int32))


@_lib.custom_op(NS + "::traffic_leaders", mutates_args=(), device_types="cuda")
def traffic_leaders(offsets: torch.Tensor, cols: torch.Tensor, dir: torch.Tensor, lane: torch.Tensor, frame_off: torch.Tensor,
                    frame_rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                                       torch.Tensor, torch.Tensor]:
    return ops.traffic_leaders(offsets, cols, dir, lane, frame_off, frame_rows)


@traffic_leaders.register_fake
def _(offsets, cols, dir, lane, frame_off, frame_rows):
    R, e = cols.shape[0], cols.new_empty
    return ((e((R,), dtype=torch.int32),) + tuple(e((R,), dtype=torch.float64) for _ in range(4))
            + (e((ops.TRAFFIC_COUNTERS,), dtype=torch.int64), e((1,), dtype=torch.int32)))

"""Functional layer over the C ABI: device tensors in, device tensors out.

Each function mirrors one piece of the reference's Python surface (file:line in the docstrings) and calls one
or a few entry points of ``libretinanet_mi355x.so`` on the current HIP stream.  torch supplies device memory,
streams and autograd bookkeeping only.
"""
import os

import numpy as np
import torch

from . import _hip

NMS_MAX = 16384
EVAL_MAX_K = 1 << 20          # RN_EVAL_MAX_K: detections of ONE image eval_select takes (64 classes x NMS_MAX)
KEEP = 10000                  # D/model.py:368


# ------------------------------------------------------------------------------------------------ anchors
def anchors(height, width, device):
    """[1,A,4] fp32 anchors of an H x W image (Anchors.forward, D/anchors.py:21-40)."""
    lib = _hip.load()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("anchors are generated on the MI355X (no CPU fallback); got device %s" % device)
    n = lib.rn_anchor_count(int(height), int(width))
    out = torch.empty((1, n, 4), dtype=torch.float32, device=device)
    _hip.call("rn_anchors_fwd", out, int(height), int(width), device=device)
    return out


def anchor_count(height, width):
    return int(_hip.load().rn_anchor_count(int(height), int(width)))


def pairwise_iou(a, b):
    """calc_iou (D/losses.py:5-22): [A,4] x [N,4] -> [A,N]."""
    _hip.need_gpu(a, b)
    a, b = _hip.f32c(a), _hip.f32c(b)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    if out.numel():
        _hip.call("rn_pairwise_iou", a, b, out, a.shape[0], b.shape[0], device=a.device)
    return out


def assign(anchor_boxes, ann, directional=True):
    """(iou_max [B,A] f32, argmax [B,A] i32 among valid rows, state [B,A] i32 in {-1,0,1}) -- D/losses.py:109-124."""
    _hip.need_gpu(anchor_boxes, ann)
    anc = _hip.f32c(anchor_boxes.reshape(-1, 4))
    ann = _hip.f32c(ann)
    B, N = ann.shape[0], ann.shape[1]
    A = anc.shape[0]
    iou = torch.empty((B, A), dtype=torch.float32, device=anc.device)
    arg = torch.empty((B, A), dtype=torch.int32, device=anc.device)
    st = torch.empty((B, A), dtype=torch.int32, device=anc.device)
    _hip.call("rn_assign", anc, ann, B, A, N, int(directional), iou, arg, st, device=anc.device)
    return iou, arg, st


# ------------------------------------------------------------------------------------------------ loss
def focal_workspace(B, A, device):
    """Workspace of rn_focal_loss_fwd / _bwd.  Its head holds the forward's completion counters and must be zero on entry
    (the kernel leaves it zero); the rest needs no initialisation."""
    lib = _hip.load()
    ws = torch.empty(lib.rn_focal_workspace_bytes(B, A), dtype=torch.uint8, device=device)
    ws[:lib.rn_focal_workspace_zero_bytes(B)].zero_()
    return ws


def focal_workspace_bytes(B, A):
    return int(_hip.load().rn_focal_workspace_bytes(int(B), int(A)))


def focal_loss_forward_raw(cls, reg, anchor_boxes, ann, directional):
    """rn_focal_loss_fwd: -> (losses [3] fp32, workspace for the backward).  No autograd, no label check."""
    _hip.need_gpu(cls, reg, anchor_boxes, ann)
    cls_c, reg_c = _hip.f32c(cls), _hip.f32c(reg)
    anc = _hip.f32c(anchor_boxes.reshape(-1, 4))
    ann_c = _hip.f32c(ann)
    B, A, C = cls_c.shape
    N = ann_c.shape[1]
    n_reg, cols = (12, 27) if directional else (4, 5)
    if reg_c.shape != (B, A, n_reg) or anc.shape[0] != A or ann_c.shape[2] != cols or ann_c.shape[0] != B:
        raise RuntimeError("focal loss: shapes cls %s reg %s anchors %s ann %s do not fit the %s variant"
                           % (tuple(cls.shape), tuple(reg.shape), tuple(anchor_boxes.shape), tuple(ann.shape),
                              "directional" if directional else "2D"))
    ws = focal_workspace(B, A, cls_c.device)
    losses = torch.empty(3, dtype=torch.float32, device=cls_c.device)
    _hip.call("rn_focal_loss_fwd", cls_c, reg_c, anc, ann_c, B, A, C, N, int(directional), ws, losses, device=cls_c.device)
    return losses, ws


def focal_loss_backward_raw(cls, reg, anchor_boxes, ann, directional, ws, grad_losses):
    """rn_focal_loss_bwd: grad_losses [3] device floats -> (dcls, dreg)."""
    cls_c, reg_c = _hip.f32c(cls), _hip.f32c(reg)
    anc = _hip.f32c(anchor_boxes.reshape(-1, 4))
    ann_c = _hip.f32c(ann)
    B, A, C = cls_c.shape
    g = _hip.f32c(grad_losses.reshape(3))
    dcls, dreg = torch.empty_like(cls_c), torch.empty_like(reg_c)
    _hip.call("rn_focal_loss_bwd", cls_c, reg_c, anc, ann_c, B, A, C, ann_c.shape[1], int(directional), ws, g, dcls, dreg,
              device=cls_c.device)
    return dcls, dreg


class _FocalLossFn(torch.autograd.Function):
    """FocalLoss.forward (D/losses.py:27-362 / R/losses.py:27-177) with a hand-written backward."""

    @staticmethod
    def forward(ctx, cls, reg, anchor_boxes, ann, directional):
        losses, ws = focal_loss_forward_raw(cls, reg, anchor_boxes, ann, directional)
        ctx.save_for_backward(cls, reg, anchor_boxes, ann, ws)
        ctx.directional = directional
        return losses[0:1], losses[1:2], losses[2:3]

    @staticmethod
    def backward(ctx, g_cls, g_reg, g_vp):
        cls, reg, anchor_boxes, ann, ws = ctx.saved_tensors
        g = torch.cat([t.reshape(1).float() if t is not None else torch.zeros(1, device=cls.device)
                       for t in (g_cls, g_reg, g_vp)])
        dcls, dreg = focal_loss_backward_raw(cls, reg, anchor_boxes, ann, ctx.directional, ws, g)
        return dcls, dreg, None, None, None


_LABEL_FLAGS = []             # [(pinned flag tensor, event)] of training forwards whose label check has not been read yet


def check_labels(ann, directional, eager=None):
    """The reference stacks an empty list when no image of the batch has a label (D/losses.py:362) and raises INSIDE the
    forward, so its trainer's try / except skips backward and optimizer.step for that iteration
    (train_detector_3D_angle.py:367-408).  The default here is the same: the one word the test needs is read from the
    device on the spot and the RuntimeError comes out of this forward (the reference's own loop synchronises every
    iteration anyway, at ``if bool(loss == 0)``, :380).
    RN_DEFERRED_LABEL_CHECK=1 (or eager=False) is the opt-in for loops that must not stall the host -- bench.py and
    captured-graph replays: the word travels asynchronously and is looked at when the NEXT call comes by (or in
    ``flush_label_checks``): the same RuntimeError, one call late; that step's vp loss is NaN (the kernel's 0/0 over
    zero labelled images) and the caller must not apply its gradients."""
    if not directional:
        return
    if ann.shape[1] == 0:
        raise RuntimeError("stack expects a non-empty TensorList (no labels in the batch)")
    if ann.is_cuda and torch.cuda.is_current_stream_capturing():
        return                                          # graph capture: nothing may leave the device; the labels were checked eagerly in the warm-up
    if eager is None:
        eager = os.environ.get("RN_DEFERRED_LABEL_CHECK", "0") != "1" or os.environ.get("RN_EAGER_LABEL_CHECK", "0") == "1"
    flush_label_checks(block=False)
    any_label = (ann[:, :, 20] != -1).any().reshape(1).to(torch.uint8)
    if eager or not ann.is_cuda:
        if not bool(any_label.item()):
            raise RuntimeError(_NO_LABEL_MSG)
        return
    flag = torch.empty(1, dtype=torch.uint8).pin_memory()
    flag.copy_(any_label, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _LABEL_FLAGS.append((flag, ev))


_NO_LABEL_MSG = ("stack expects a non-empty TensorList (no image in the batch has a label; the reference's FocalLoss "
                 "raises here, D/losses.py:362)")


def flush_label_checks(block=True):
    """Look at the label checks that have arrived (block: wait for all of them); raise if one found no label."""
    bad = False
    while _LABEL_FLAGS:
        flag, ev = _LABEL_FLAGS[0]
        if not block and not ev.query():
            break
        ev.synchronize()
        _LABEL_FLAGS.pop(0)
        bad |= not bool(flag.item())
    if bad:
        raise RuntimeError(_NO_LABEL_MSG + " [reported by the deferred check of an earlier training call]")


def _check_labels(ann, directional):
    check_labels(ann, directional, eager=True)


def focal_loss(cls, reg, anchor_boxes, ann, directional=True, check_labels=True):
    """-> (cls_loss[1], reg_loss[1], vp_loss[1]) directional, (cls_loss[1], reg_loss[1]) 2D."""
    if check_labels:
        _check_labels(ann, directional)
    out = _FocalLossFn.apply(cls, reg, anchor_boxes, ann, bool(directional))
    return out if directional else out[:2]


# ------------------------------------------------------------------------------------------------ decode
def decode_dir(anchor_boxes, reg):
    """BBoxTransform.forward, directional (D/utils.py:102-149): [1,A,4],[B,A,12] -> [B,A,20]."""
    _hip.need_gpu(anchor_boxes, reg)
    anc, reg_c = _hip.f32c(anchor_boxes.reshape(-1, 4)), _hip.f32c(reg)
    B, A, _ = reg_c.shape
    out = torch.empty((B, A, 20), dtype=torch.float32, device=reg_c.device)
    _hip.call("rn_decode_dir", anc, reg_c, out, B, A, device=reg_c.device)
    return out


def decode_2d(anchor_boxes, deltas, clip_hw=None):
    """BBoxTransform.forward, 2D (R/utils.py:102-126), optionally with ClipBoxes fused (R/utils.py:134-144)."""
    _hip.need_gpu(anchor_boxes, deltas)
    anc, d = _hip.f32c(anchor_boxes.reshape(-1, 4)), _hip.f32c(deltas)
    B, A, _ = d.shape
    out = torch.empty((B, A, 4), dtype=torch.float32, device=d.device)
    h, w = clip_hw if clip_hw is not None else (0.0, 0.0)
    _hip.call("rn_decode_2d", anc, d, out, B, A, int(clip_hw is not None), float(w), float(h), device=d.device)
    return out


def clip_boxes_check(boxes):
    _hip.need_gpu(boxes)
    if boxes.dtype != torch.float32 or not boxes.is_contiguous() or boxes.shape[-1] != 4:
        raise RuntimeError("clip_boxes_ needs a contiguous fp32 [...,4] tensor")


def clip_boxes_(boxes, height, width):
    """ClipBoxes.forward (R/utils.py:134-144): in place on a contiguous [..,4] fp32 tensor; returns it."""
    clip_boxes_check(boxes)
    if boxes.numel():
        _hip.call("rn_clip_boxes", boxes, boxes.numel() // 4, float(width), float(height), device=boxes.device)
    return boxes


# ------------------------------------------------------------------------------------------------ post-process
class _PostBuffers:
    """Device scratch for C independent select+NMS problems, so one host sync reads every count."""

    def __init__(self, n_scores, n_problems, max_sel, device):
        lib = _hip.load()
        self.ws = torch.empty(lib.rn_post_workspace_bytes(n_scores, NMS_MAX), dtype=torch.uint8, device=device)
        self.count = torch.zeros((n_problems, 2), dtype=torch.int32, device=device)      # [:,0] selected, [:,1] kept
        self.sel = torch.empty((n_problems, max_sel), dtype=torch.int32, device=device)
        self.keep = torch.empty((n_problems, NMS_MAX), dtype=torch.int32, device=device)


def _select(scores_ptr, n, stride, start, fixed, buf, p):
    """Under the caller's device guard, as every call of the post-process below."""
    _hip.call("rn_threshold_select", scores_ptr, n, stride, float(start), KEEP, float(fixed), buf.ws, buf.count[p, 0:1], buf.sel[p])


def _nms(boxes, box_col, scores_ptr, score_stride, category, buf, p, max_cand):
    _hip.call("rn_nms", boxes, boxes.shape[-1], box_col, scores_ptr, score_stride, buf.sel[p], category, buf.count[p, 0:1],
              max_cand, 0.5, buf.ws, buf.keep[p], buf.count[p, 1:2])


def postprocess_single(cls, boxes20):
    """Single-frame eval branch (D/model.py:346-397): per class, adaptive threshold from 1e-25 until <= 10 000
    survive, NMS(0.5) on cols 16:20.  cls [1,A,C], boxes [1,A,20] -> [scores[K], class_idx[K] i64, boxes[K,20]]."""
    _hip.need_gpu(cls, boxes20)
    if cls.shape[0] != 1:
        raise RuntimeError("single-frame post-process assumes batch 1 (D/model.py:366 squeezes the batch away); "
                           "use MULTI_FRAME=True for batches")
    cls, boxes20 = _hip.f32c(cls), _hip.f32c(boxes20)
    A, C = cls.shape[1], cls.shape[2]
    buf = _PostBuffers(A, C, KEEP, cls.device)
    with torch.cuda.device(cls.device):
        for c in range(C):
            sp = cls.data_ptr() + 4 * c
            _select(sp, A, C, 1e-25, -1.0, buf, c)
            _nms(boxes20, 16, sp, C, None, buf, c, KEEP)
    counts = buf.count.cpu().numpy()
    out_s, out_c, out_b = [], [], []
    for c in range(C):
        if counts[c, 0] == 0:
            continue                                                       # D/model.py:376-378
        idx = buf.sel[c].long()[buf.keep[c, :counts[c, 1]].long()]
        out_s.append(cls[0, idx, c])
        out_c.append(torch.full((idx.numel(),), c, dtype=torch.int64, device=cls.device))
        out_b.append(boxes20[0, idx])
    if not out_s:
        e = torch.zeros(0, device=cls.device)
        return [e, torch.zeros(0, dtype=torch.int64, device=cls.device), e.clone()]
    return [torch.cat(out_s), torch.cat(out_c), torch.cat(out_b)]


def postprocess_multi(cls, boxes20):
    """MULTI_FRAME eval branch (D/model.py:311-344): flatten B*A, max over classes, adaptive threshold from 1e-7,
    batched NMS keyed by image.  -> (scores[K], classes[K] i64, boxes[K,20], im_index[K] i64)."""
    _hip.need_gpu(cls, boxes20)
    cls, boxes20 = _hip.f32c(cls), _hip.f32c(boxes20)
    B, A, C = cls.shape
    n = B * A
    dev = cls.device
    scores = torch.empty(n, dtype=torch.float32, device=dev)
    classes = torch.empty(n, dtype=torch.int64, device=dev)
    buf = _PostBuffers(n, 1, KEEP, dev)
    with torch.cuda.device(dev):
        _hip.call("rn_rowmax", cls, n, C, scores, classes)
        _select(scores, n, 1, 1e-7, -1.0, buf, 0)
        # image index of each candidate = flat index // A   (D/model.py:314-316)
        cat = torch.div(buf.sel[0], A, rounding_mode="floor").to(torch.int32)
        _nms(boxes20.reshape(n, 20), 16, scores, 1, cat, buf, 0, KEEP)
    counts = buf.count.cpu().numpy()
    idx = buf.sel[0].long()[buf.keep[0, :counts[0, 1]].long()]
    return scores[idx], classes[idx], boxes20.reshape(n, 20)[idx], torch.div(idx, A, rounding_mode="floor")


def _arange_i32(n, device, _cache={}):
    key = (n, str(device))
    if key not in _cache:
        _cache[key] = torch.arange(n, dtype=torch.int32, device=device)
    return _cache[key]


def detect_multi(cls, reg, anchor_boxes):
    """MULTI_FRAME eval branch (D/model.py:311-344) from the head outputs, decoding ONLY the survivors of the score
    filter: row max over classes -> adaptive threshold (<= 10 000 candidates) -> decode those (rn_decode_dir_select; the
    reference decodes all B*A anchors first, :347) -> batched NMS keyed by image on the compact boxes.  Same survivors,
    bit-identical boxes.  -> (scores[K], classes[K] i64, boxes[K,20], im_index[K] i64)."""
    _hip.need_gpu(cls, reg, anchor_boxes)
    cls, reg = _hip.f32c(cls), _hip.f32c(reg)
    anc = _hip.f32c(anchor_boxes.reshape(-1, 4))
    B, A, C = cls.shape
    n = B * A
    dev = cls.device
    scores = torch.empty(n, dtype=torch.float32, device=dev)
    classes = torch.empty(n, dtype=torch.int64, device=dev)
    buf = _PostBuffers(n, 1, KEEP, dev)
    cboxes = torch.empty((KEEP, 20), dtype=torch.float32, device=dev)
    cscore = torch.empty(KEEP, dtype=torch.float32, device=dev)
    cimage = torch.empty(KEEP, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("rn_rowmax", cls, n, C, scores, classes)
        _select(scores, n, 1, 1e-7, -1.0, buf, 0)
        _hip.call("rn_decode_dir_select", anc, reg, A, scores, 1, buf.sel[0], buf.count[0, 0:1], KEEP, cboxes, cscore, cimage)
        _hip.call("rn_nms", cboxes, 20, 16, cscore, 1, _arange_i32(KEEP, dev), cimage, buf.count[0, 0:1], KEEP, 0.5, buf.ws,
                  buf.keep[0], buf.count[0, 1:2])
    counts = buf.count.cpu().numpy()
    kept = buf.keep[0, :counts[0, 1]].long()                              # candidate positions, decreasing score
    return cscore[kept], classes[buf.sel[0].long()[kept]], cboxes[kept], cimage[kept].long()


def detect_single(cls, reg, anchor_boxes):
    """Single-frame eval branch (D/model.py:346-397) from the head outputs, decoding only each class's survivors.
    cls [1,A,C], reg [1,A,12] -> [scores[K], class_idx[K] i64, boxes[K,20]]."""
    _hip.need_gpu(cls, reg, anchor_boxes)
    if cls.shape[0] != 1:
        raise RuntimeError("single-frame post-process assumes batch 1 (D/model.py:366 squeezes the batch away); "
                           "use MULTI_FRAME=True for batches")
    cls, reg = _hip.f32c(cls), _hip.f32c(reg)
    anc = _hip.f32c(anchor_boxes.reshape(-1, 4))
    A, C = cls.shape[1], cls.shape[2]
    dev = cls.device
    buf = _PostBuffers(A, C, KEEP, dev)
    cboxes = torch.empty((C, KEEP, 20), dtype=torch.float32, device=dev)
    cscore = torch.empty((C, KEEP), dtype=torch.float32, device=dev)
    ar = _arange_i32(KEEP, dev)
    with torch.cuda.device(dev):
        for c in range(C):
            sp = cls.data_ptr() + 4 * c
            _select(sp, A, C, 1e-25, -1.0, buf, c)
            _hip.call("rn_decode_dir_select", anc, reg, A, sp, C, buf.sel[c], buf.count[c, 0:1], KEEP, cboxes[c], cscore[c], None)
            _hip.call("rn_nms", cboxes[c], 20, 16, cscore[c], 1, ar, None, buf.count[c, 0:1], KEEP, 0.5, buf.ws, buf.keep[c],
                      buf.count[c, 1:2])
    counts = buf.count.cpu().numpy()
    out_s, out_c, out_b = [], [], []
    for c in range(C):
        if counts[c, 0] == 0:
            continue                                                       # D/model.py:376-378
        kept = buf.keep[c, :counts[c, 1]].long()
        out_s.append(cscore[c][kept])
        out_c.append(torch.full((kept.numel(),), c, dtype=torch.int64, device=dev))
        out_b.append(cboxes[c][kept])
    if not out_s:
        e = torch.zeros(0, device=dev)
        return [e, torch.zeros(0, dtype=torch.int64, device=dev), e.clone()]
    return [torch.cat(out_s), torch.cat(out_c), torch.cat(out_b)]


def postprocess_2d(cls, boxes4):
    """2D eval branch (R/model.py:283-311): per class score > 0.05, NMS(0.5)."""
    _hip.need_gpu(cls, boxes4)
    if cls.shape[0] != 1:
        raise RuntimeError("the 2D post-process assumes batch 1 (R/model.py:288 squeezes the batch away)")
    cls, boxes4 = _hip.f32c(cls), _hip.f32c(boxes4)
    A, C = cls.shape[1], cls.shape[2]
    buf = _PostBuffers(A, C, A, cls.device)
    with torch.cuda.device(cls.device):
        for c in range(C):
            sp = cls.data_ptr() + 4 * c
            _select(sp, A, C, 0.0, 0.05, buf, c)
        counts = buf.count.cpu().numpy()
        if counts[:, 0].max() > NMS_MAX:
            raise RuntimeError("more than %d boxes above 0.05 in one class (%d): the on-device NMS orders its "
                               "candidates in LDS and does not take more" % (NMS_MAX, counts[:, 0].max()))
        for c in range(C):
            if counts[c, 0]:
                _nms(boxes4, 0, cls.data_ptr() + 4 * c, C, None, buf, c, NMS_MAX)
    counts = buf.count.cpu().numpy()
    out_s, out_c, out_b = [], [], []
    for c in range(C):
        if counts[c, 0] == 0:
            continue
        idx = buf.sel[c].long()[buf.keep[c, :counts[c, 1]].long()]
        out_s.append(cls[0, idx, c])
        out_c.append(torch.full((idx.numel(),), c, dtype=torch.int64, device=cls.device))
        out_b.append(boxes4[0, idx])
    if not out_s:
        e = torch.zeros(0, device=cls.device)
        return [e, torch.zeros(0, dtype=torch.int64, device=cls.device), e.clone()]
    return [torch.cat(out_s), torch.cat(out_c), torch.cat(out_b)]


def nms(boxes, scores, iou_threshold, idxs=None):
    """torchvision.ops.nms / batched_nms (D/model.py:19-57) on device: int64 keep indices, decreasing score."""
    lib = _hip.load()
    _hip.need_gpu(boxes, scores, idxs)
    n = boxes.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    if n > NMS_MAX:
        raise RuntimeError("on-device NMS orders its candidates in LDS and takes at most %d boxes, got %d" % (NMS_MAX, n))
    boxes, scores = _hip.f32c(boxes), _hip.f32c(scores)
    dev = boxes.device
    ws = torch.empty(lib.rn_post_workspace_bytes(n, NMS_MAX), dtype=torch.uint8, device=dev)
    cand = torch.arange(n, dtype=torch.int32, device=dev)
    count = torch.tensor([n, 0], dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    cat = None if idxs is None else idxs.to(torch.int32).contiguous()
    _hip.call("rn_nms", boxes, boxes.shape[1], 0, scores, 1, cand, cat, count[0:1], n, float(iou_threshold), ws, keep, count[1:2],
              device=dev)
    return keep[:int(count[1])].long()


# ------------------------------------------------------------------------------------------------ homography
def _mats(m, device):
    if m is None:
        return None
    return torch.as_tensor(np.ascontiguousarray(m, dtype=np.float64)).to(device)


def _state6(state):
    """[d, >= 6] -> contiguous fp32 [d,6]: the reference's transforms index columns 0..5 of the state and ignore further
    ones (homography.py:305-320; the tracker's states carry the speed as a 7th, MC3D_crop_tracker.py:1278)."""
    if state.dim() != 2 or state.shape[1] < 6:
        raise RuntimeError("state tensors are [d, 6] (x, y, l, w, h, direction[, ...]); got %s" % (tuple(state.shape),))
    return _hip.f32c(state[:, :6])


def hg_state_to_space(state):
    _hip.need_gpu(state)
    s = _state6(state)
    out = torch.empty((s.shape[0], 8, 3), dtype=torch.float32, device=s.device)
    if s.shape[0]:
        _hip.call("rn_state_to_space", s, out, s.shape[0], device=s.device)
    return out


def hg_space_to_state(space):
    _hip.need_gpu(space)
    sp = space.double().contiguous()
    out = torch.empty((sp.shape[0], 6), dtype=torch.float32, device=sp.device)
    if sp.shape[0]:
        _hip.call("rn_space_to_state", sp, out, sp.shape[0], device=sp.device)
    return out


def hg_to_im(points, P, P2=None, mat_index=None, from_state=True):
    """state [d,6] (from_state) or space [d,8,3] fp32 -> image [d,8,2] fp64.  P: device fp64 [n,3,4]."""
    _hip.need_gpu(points, P, P2, mat_index)
    p = _state6(points) if from_state else _hip.f32c(points)
    d = p.shape[0]
    out = torch.empty((d, 8, 2), dtype=torch.float64, device=p.device)
    if d:
        _hip.call("rn_state_to_im" if from_state else "rn_space_to_im", p, P, P2, mat_index, out, d, device=p.device)
    return out


def hg_from_im(im, heights, H, H2=None, mat_index=None, to_state=True):
    """image [d,8,2] fp64 + heights [d] -> state [d,6] fp32 (to_state) or space [d,8,3] fp64."""
    _hip.need_gpu(im, heights, H, H2, mat_index)
    im = im.double().contiguous()
    hts = _hip.f32c(heights)
    d = im.shape[0]
    if to_state:
        out = torch.empty((d, 6), dtype=torch.float32, device=im.device)
    else:
        out = torch.empty((d, 8, 3), dtype=torch.float64, device=im.device)
    if d:
        _hip.call("rn_im_to_state" if to_state else "rn_im_to_space", im, hts, H, H2, mat_index, out, d, device=im.device)
    return out


# ------------------------------------------------------------------------------------------------ tracker: detection parsing
PARSE_MAX = 16384
NMS_IM, NMS_SPACE = 1, 2


def parse_detections(scores, labels, boxes20, camera_idxs, H1, H2, P1, P2, sigma_d, phi_nms_im, phi_nms_space,
                     nms_flags=NMS_IM | NMS_SPACE, refine_height=False, heights=None):
    """MC_Crop_Tracker.parse_detections (MC3D_crop_tracker.py:319-383) on device, see include/retinanet_mi355x.h.
    H*/P*: device fp64 [n_cam,3,3] / [n_cam,3,4] (index = camera index).  Returns device tensors sized for the input
    plus the device count: (state [d,6], labels [d], scores [d], cams [d], count int32[1]); the caller slices."""
    lib = _hip.load()
    _hip.need_gpu(scores, labels, boxes20, camera_idxs, H1, H2, P1, P2, heights)
    d = scores.shape[0]
    if d > PARSE_MAX:
        raise RuntimeError("detection parsing orders its NMS candidates in LDS and takes at most %d detections, got %d"
                           % (PARSE_MAX, d))
    if boxes20.shape != (d, 20) or labels.shape[0] != d or camera_idxs.shape[0] != d:
        raise RuntimeError("parse_detections: scores %s labels %s boxes %s cameras %s do not line up"
                           % (tuple(scores.shape), tuple(labels.shape), tuple(boxes20.shape), tuple(camera_idxs.shape)))
    dev = scores.device
    scores, boxes20 = _hip.f32c(scores), _hip.f32c(boxes20)
    labels, camera_idxs = labels.long().contiguous(), camera_idxs.long().contiguous()
    hts = None if heights is None else _hip.f32c(heights)
    ws = torch.empty(lib.rn_parse_workspace_bytes(d), dtype=torch.uint8, device=dev)
    out_state = torch.empty((d, 6), dtype=torch.float32, device=dev)
    out_labels = torch.empty(d, dtype=torch.int64, device=dev)
    out_scores = torch.empty(d, dtype=torch.float32, device=dev)
    out_cams = torch.empty(d, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _hip.call("rn_parse_detections", scores, labels, boxes20, camera_idxs, d, H1, H2, P1, P2, H1.shape[0], hts, float(sigma_d),
              float(phi_nms_im), float(phi_nms_space), int(nms_flags), int(bool(refine_height)), ws, out_state, out_labels,
              out_scores, out_cams, count, device=dev)
    return out_state, out_labels, out_scores, out_cams, count


def md_iou(a, b):
    """MC_Crop_Tracker.md_iou (MC3D_crop_tracker.py:1030-1049): [B,N,4] x [B,N,4] -> [B,N] fp64."""
    _hip.need_gpu(a, b)
    if a.shape != b.shape or a.shape[-1] != 4:
        raise RuntimeError("md_iou: shapes %s and %s" % (tuple(a.shape), tuple(b.shape)))
    a, b = a.double().contiguous(), b.double().contiguous()
    out = torch.empty(a.shape[:-1], dtype=torch.float64, device=a.device)
    if out.numel():
        _hip.call("rn_md_iou", a, b, out, out.numel(), device=a.device)
    return out


# ------------------------------------------------------------------------------------------------ track association
LSAP_MAX_MIN = 4096                # RN_LSAP_MAX_MIN: min(rows, cols)
LSAP_MAX = PARSE_MAX               # max(rows, cols)
LSAP_OK, LSAP_INVALID, LSAP_INFEASIBLE = 0, 1, 2


def track_cost(pre, det):
    """The cost of MC_Crop_Tracker.match_hungarian (MC3D_crop_tracker.py:680-701): priors [n, >=6] and detections
    [m, >=6] fp32 states (direction at column 5) -> [n,m] fp64 ``1 - md_iou`` of their road-plane footprints."""
    _hip.need_gpu(pre, det)
    if pre.dim() != 2 or det.dim() != 2 or pre.shape[1] < 6 or det.shape[1] < 6:
        raise RuntimeError("track_cost: states are [n, >= 6], got %s and %s" % (tuple(pre.shape), tuple(det.shape)))
    pre, det = _hip.f32c(pre), _hip.f32c(det)
    n, m = pre.shape[0], det.shape[0]
    cost = torch.empty((n, m), dtype=torch.float64, device=pre.device)
    if n and m:
        _hip.call("rn_track_cost", pre, pre.shape[1], det, det.shape[1], n, m, cost, device=pre.device)
    return cost


def _lsap(cost, max_cost):
    """-> (row_match int32 [nr], info int32 [2] = (pairs kept, status)), device tensors, no synchronisation."""
    lib = _hip.load()
    _hip.need_gpu(cost)
    if cost.dim() != 2:
        raise ValueError("expected a matrix (2-D array), got a %d array" % cost.dim())
    nr, nc = cost.shape
    dev = cost.device
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    row_match = torch.full((nr,), -1, dtype=torch.int32, device=dev)
    if nr == 0 or nc == 0:
        return row_match, info
    if min(nr, nc) > LSAP_MAX_MIN or max(nr, nc) > LSAP_MAX:
        raise RuntimeError("linear_sum_assignment takes at most %d x %d (either orientation), got %d x %d"
                           % (LSAP_MAX_MIN, LSAP_MAX, nr, nc))
    c = cost.double().contiguous()
    ws = torch.empty(lib.rn_lsap_workspace_bytes(nr, nc), dtype=torch.uint8, device=dev)
    _hip.call("rn_linear_sum_assignment", c, nr, nc, float(max_cost), ws, row_match, info[0:1], info[1:2], device=dev)
    return row_match, info


def _matched_rows(row_match, k):
    """The k rows with a match, in increasing order, without a synchronisation (a stable sort of the 'unmatched' flag)."""
    return torch.argsort((row_match < 0).to(torch.int8), stable=True)[:k]


def match(cost, max_cost, info=False):
    """linear_sum_assignment + match_hungarian's gate (MC3D_crop_tracker.py:706-723) in one launch, without a
    synchronisation: -> row_match int32 [nr] (matched column or -1; all -1 on invalid / infeasible input, which is the
    reference's ``except ValueError: return []``).  info=True also returns the device int32 [2] (pairs kept, status)."""
    row_match, inf = _lsap(cost, max_cost)
    return (row_match, inf) if info else row_match


def linear_sum_assignment(cost):
    """scipy.optimize.linear_sum_assignment(cost) on the device, same result: (row_ind, col_ind) int64 device tensors
    sorted by row.  Copies one word pair (count, status) to the host; raises ValueError with scipy's wording on a NaN or
    -inf entry or when no finite complete assignment exists."""
    row_match, inf = _lsap(cost, float("inf"))
    k, status = (int(x) for x in inf.cpu())
    if status == LSAP_INVALID:
        raise ValueError("matrix contains invalid numeric entries")
    if status == LSAP_INFEASIBLE:
        raise ValueError("cost matrix is infeasible")
    rows = _matched_rows(row_match, k)
    return rows, row_match[rows].long()


# ------------------------------------------------------------------------------------------------ tracking evaluation
MOT_MAX = 512                      # RN_MOT_MAX: objects of one frame on either side
MOT_MAX_IDS = 16384                # RN_MOT_MAX_IDS
MOT_RESULT = 152                   # RN_MOT_RESULT
MOT_OK, MOT_INVALID, MOT_INFEASIBLE, MOT_TOO_LARGE = 0, 1, 2, 3


def _typed(what, *specs):
    """The dtype and contiguity check of every domain below: specs are (name, tensor, dtype)."""
    for name, t, dtype in specs:
        if t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError("%s: %s is a contiguous %s tensor, got %s" % (what, name, dtype, t.dtype))


def _status_word(what, device, status):
    """The status word a family of entry points ORs its bits into: a zeroed int32 [1] unless one is handed on."""
    if status is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    _hip.need_gpu(status)
    _typed(what, ("status", status, torch.int32))
    if status.numel() != 1:
        raise RuntimeError("%s: status is one int32" % what)
    return status


def _refused(prefix, bits_table, status):
    """Raises on a non-zero status word (an int, or the int32 [1] tensor: one element is read back)."""
    bits = int(status)
    if bits:
        raise RuntimeError(prefix + _bits_text(bits_table, bits) + " (status %d)" % bits)


def _bits_text(bits_table, bits):
    return "; ".join(t for b, t in bits_table if bits & b)


def mot_prepare(gt_im, gt_h0, gt_vel, pred_state, H, P):
    """mot_evaluator.py:155-215 for all objects of a sequence: gt_im fp64 [G,8,2], gt_h0 / gt_vel fp32 [G], pred_state fp32
    [M,7], H fp64 [3,3], P fp64 [3,4] -> (gt_state fp32 [G,7], gt_box fp32 [G,4], pred_box fp32 [M,4], pred_im fp64 [M,8,2])."""
    _hip.need_gpu(gt_im, gt_h0, gt_vel, pred_state, H, P)
    _typed("mot_prepare", ("gt_im", gt_im, torch.float64), ("gt_h0", gt_h0, torch.float32), ("gt_vel", gt_vel, torch.float32),
           ("pred_state", pred_state, torch.float32), ("H", H, torch.float64), ("P", P, torch.float64))
    G, M, dev = gt_im.shape[0], pred_state.shape[0], gt_im.device
    if gt_im.numel() != G * 16 or gt_h0.numel() != G or gt_vel.numel() != G or pred_state.numel() != M * 7 or H.numel() != 9 \
            or P.numel() != 12:
        raise RuntimeError("mot_prepare: gt_im [G,8,2], gt_h0 [G], gt_vel [G], pred_state [M,7], H [3,3], P [3,4]")
    gt_state = torch.empty((G, 7), dtype=torch.float32, device=dev)
    gt_box = torch.empty((G, 4), dtype=torch.float32, device=dev)
    pred_box = torch.empty((M, 4), dtype=torch.float32, device=dev)
    pred_im = torch.empty((M, 8, 2), dtype=torch.float64, device=dev)
    _hip.call("rn_mot_prepare", gt_im, gt_h0, gt_vel, G, pred_state, M, H, P, gt_state, gt_box, pred_box, pred_im, device=dev)
    return gt_state, gt_box, pred_box, pred_im


def mot_offsets(n_gt, n_pred, device):
    """Per-frame object counts (host sequences) -> (gt_off, pr_off int32 [F+1], iou_off int64 [F+1], slot_off int32 [F+1]) on
    the device and the host totals (max_n, max_cells, cells, S).  A frame above MOT_MAX raises here: nothing is launched."""
    ng, npr = np.asarray(n_gt, np.int64).reshape(-1), np.asarray(n_pred, np.int64).reshape(-1)
    if ng.shape != npr.shape or (ng < 0).any() or (npr < 0).any():
        raise RuntimeError("mot_offsets: one non-negative count per frame on both sides")
    max_n = int(max(ng.max(initial=0), npr.max(initial=0)))
    if max_n > MOT_MAX:
        raise RuntimeError("a frame holds %d objects; the assignment takes at most MOT_MAX = %d per side" % (max_n, MOT_MAX))
    cells, slots = ng * npr, np.minimum(ng, npr)
    if ng.sum() >= 2 ** 31 or npr.sum() >= 2 ** 31:
        raise RuntimeError("mot_offsets: more than 2^31 objects")

    def off(x, dtype):
        return torch.from_numpy(np.concatenate(([0], np.cumsum(x))).astype(dtype)).to(device)
    return ((off(ng, np.int32), off(npr, np.int32), off(cells, np.int64), off(slots, np.int32)),
            (max_n, int(cells.max(initial=0)), int(cells.sum()), int(slots.sum())))


def mot_iou(gt_box, pred_box, offsets, totals):
    """Every frame's IoU matrix in self.iou's fp32 arithmetic (mot_evaluator.py:87-118, 219-222) -> flat fp64 [cells]."""
    _hip.need_gpu(gt_box, pred_box, *offsets)
    _typed("mot_iou", ("gt_box", gt_box, torch.float32), ("pred_box", pred_box, torch.float32))
    gt_off, pr_off, iou_off, _ = offsets
    max_n, max_cells, cells, _ = totals
    iou = torch.empty(cells, dtype=torch.float64, device=gt_box.device)
    _hip.call("rn_mot_iou", gt_box, pred_box, gt_off, pr_off, iou_off, gt_off.numel() - 1, max_cells, iou, device=gt_box.device)
    return iou


def mot_assign(iou, offsets, totals, M):
    """linear_sum_assignment(ious, maximize=True) of every frame (mot_evaluator.py:225) ->
    (slot_row, slot_col int32 [S], pred_assigned uint8 [M], frame_status int32 [F])."""
    _hip.need_gpu(iou, *offsets)
    _typed("mot_assign", ("iou", iou, torch.float64))
    gt_off, pr_off, iou_off, slot_off = offsets
    max_n, _, cells, S = totals
    if iou.numel() != cells:
        raise RuntimeError("mot_assign: iou holds %d cells, the offsets describe %d" % (iou.numel(), cells))
    if max_n > MOT_MAX:
        raise RuntimeError("a frame holds %d objects; the assignment takes at most MOT_MAX = %d per side" % (max_n, MOT_MAX))
    dev, F = iou.device, gt_off.numel() - 1
    slot_row = torch.empty(S, dtype=torch.int32, device=dev)
    slot_col = torch.empty(S, dtype=torch.int32, device=dev)
    pred_assigned = torch.empty(M, dtype=torch.uint8, device=dev)
    frame_status = torch.zeros(F, dtype=torch.int32, device=dev)
    _hip.call("rn_mot_assign", iou, gt_off, pr_off, iou_off, slot_off, F, max_n, S, M, slot_row, slot_col, pred_assigned,
              frame_status, device=dev)
    return slot_row, slot_col, pred_assigned, frame_status


def mot_frame_metrics(iou, offsets, totals, assigned, match_iou, gt_state, pred_state, gt_im, pred_im, gt_cls, pred_cls, gt_id, pred_id):
    """mot_evaluator.py:229-238, 283-290, 301-341 per frame.  assigned = what mot_assign returns.  ->
    (slot_iou fp64 [S], slot_gid, slot_pid int32 [S] (-1 below match_iou), state_err fp32 [S,7], bot, top fp64 [S], cell uint8
    [S], frame_edge, frame_match int32 [F])."""
    slot_row, slot_col, pred_assigned, frame_status = assigned
    gt_off, pr_off, iou_off, slot_off = offsets
    _hip.need_gpu(iou, gt_state, pred_state, gt_im, pred_im, gt_cls, pred_cls, gt_id, pred_id, *assigned)
    _typed("mot_frame_metrics", ("iou", iou, torch.float64), ("gt_state", gt_state, torch.float32),
           ("pred_state", pred_state, torch.float32), ("gt_im", gt_im, torch.float64), ("pred_im", pred_im, torch.float64),
           ("gt_cls", gt_cls, torch.int32), ("pred_cls", pred_cls, torch.int32), ("gt_id", gt_id, torch.int32),
           ("pred_id", pred_id, torch.int32))
    G, M = gt_id.numel(), pred_id.numel()
    if gt_state.numel() != G * 7 or pred_state.numel() != M * 7 or gt_im.numel() != G * 16 or pred_im.numel() != M * 16 \
            or gt_cls.numel() != G or pred_cls.numel() != M or pred_assigned.numel() != M:
        raise RuntimeError("mot_frame_metrics: per-object arrays disagree on G = %d / M = %d" % (G, M))
    dev, F, S = iou.device, gt_off.numel() - 1, totals[3]
    slot_iou = torch.empty(S, dtype=torch.float64, device=dev)
    slot_gid = torch.empty(S, dtype=torch.int32, device=dev)
    slot_pid = torch.empty(S, dtype=torch.int32, device=dev)
    state_err = torch.empty((S, 7), dtype=torch.float32, device=dev)
    bot = torch.empty(S, dtype=torch.float64, device=dev)
    top = torch.empty(S, dtype=torch.float64, device=dev)
    cell = torch.empty(S, dtype=torch.uint8, device=dev)
    frame_edge = torch.zeros(F, dtype=torch.int32, device=dev)
    frame_match = torch.zeros(F, dtype=torch.int32, device=dev)
    _hip.call("rn_mot_frame_metrics", iou, gt_off, pr_off, iou_off, slot_off, F, S, slot_row, slot_col, frame_status,
              float(match_iou), gt_state, pred_state, gt_im, pred_im, gt_cls, pred_cls, gt_id, pred_id, pred_assigned, slot_iou,
              slot_gid, slot_pid, state_err, bot, top, cell, frame_edge, frame_match, device=dev)
    return slot_iou, slot_gid, slot_pid, state_err, bot, top, cell, frame_edge, frame_match


def mot_reduce(offsets, totals, assigned, per_slot, gt_id, pred_id, n_gid, n_pid):
    """The sequence-order walk and the sums (mot_evaluator.py:135-152, 294-299, 348-397) -> result fp64 [MOT_RESULT] on the
    device (layout: include/retinanet_mi355x.h).  gt_id / pred_id are dense indices below n_gid / n_pid; the kernel leaves an id
    outside that range out of every count instead of indexing with it, so nothing here reads the device."""
    lib = _hip.load()
    gt_off, pr_off, iou_off, slot_off = offsets
    slot_row, slot_col, pred_assigned, frame_status = assigned
    slot_iou, slot_gid, slot_pid, state_err, bot, top, cell, frame_edge, frame_match = per_slot
    _hip.need_gpu(gt_id, pred_id, *per_slot)
    _typed("mot_reduce", ("gt_id", gt_id, torch.int32), ("pred_id", pred_id, torch.int32))
    if n_gid > MOT_MAX_IDS or n_pid > MOT_MAX_IDS:
        raise RuntimeError("mot_reduce takes at most %d distinct ids per side, got %d and %d" % (MOT_MAX_IDS, n_gid, n_pid))
    dev, F, S = gt_id.device, gt_off.numel() - 1, totals[3]
    ws = torch.empty(max(16, lib.rn_mot_workspace_bytes(n_gid, n_pid)), dtype=torch.uint8, device=dev)
    result = torch.empty(MOT_RESULT, dtype=torch.float64, device=dev)
    _hip.call("rn_mot_reduce", F, S, gt_off, pr_off, slot_off, frame_status, frame_edge, frame_match, slot_row, slot_iou, slot_gid,
              slot_pid, state_err, bot, top, cell, gt_id, pred_id, n_gid, n_pid, ws, result, device=dev)
    return result


# ------------------------------------------------------------------------------------------------ identity and association scores
MOT_ALPHAS = 19                    # RN_MOT_ALPHAS
MOT_ASSOC_RESULT = 135             # RN_MOT_ASSOC_RESULT
MOT_ASSOC_MAX_CELLS = 1 << 20      # RN_MOT_ASSOC_MAX_CELLS: n_gid * n_pid of the dense id x id storage
MOT_DUPLICATE_ID, MOT_BAD_INDEX = 4, 5


def mot_alphas():
    """The HOTA thresholds: what np.arange(0.05, 0.99, 0.05) holds, 0.05 + k * 0.05 in fp64."""
    return np.arange(0.05, 0.99, 0.05)


def mot_assoc_dims(what, n_gid, n_pid):
    """The documented cap of the dense storage: raises before any launch."""
    if n_gid < 0 or n_pid < 0 or n_gid > MOT_MAX_IDS or n_pid > MOT_MAX_IDS or n_gid * n_pid > MOT_ASSOC_MAX_CELLS:
        raise RuntimeError("%s: %d ground-truth ids x %d predicted ids = %d cells; the dense id x id storage takes at most %d cells "
                           "and %d ids per side" % (what, n_gid, n_pid, n_gid * n_pid, MOT_ASSOC_MAX_CELLS, MOT_MAX_IDS))


def _assoc_layout(what, offsets, totals, gt_id, pred_id, iou=None):
    """The frame layout as the rn_mot_id_* / rn_mot_hota_* entries take it: (offset tensors, sizes)."""
    gt_off, pr_off, iou_off, slot_off = offsets
    max_n, _, cells, S = totals
    _hip.need_gpu(gt_id, pred_id, iou, *offsets)
    _typed(what, ("gt_id", gt_id, torch.int32), ("pred_id", pred_id, torch.int32), ("gt_off", gt_off, torch.int32),
           ("pr_off", pr_off, torch.int32), ("iou_off", iou_off, torch.int64), ("slot_off", slot_off, torch.int32))
    if max_n > MOT_MAX:
        raise RuntimeError("a frame holds %d objects; the assignment takes at most MOT_MAX = %d per side" % (max_n, MOT_MAX))
    F = gt_off.numel() - 1
    if F < 0 or pr_off.numel() != F + 1 or iou_off.numel() != F + 1 or slot_off.numel() != F + 1:
        raise RuntimeError("%s: the four offset arrays hold F + 1 entries each" % what)
    if iou is not None:
        _typed(what, ("iou", iou, torch.float64))
        if iou.numel() != cells:
            raise RuntimeError("%s: iou holds %d cells, the offsets describe %d" % (what, iou.numel(), cells))
    return (gt_off, pr_off, iou_off, slot_off), (F, max_n, gt_id.numel(), pred_id.numel(), cells, S)


def mot_id_counts(iou, offsets, totals, gt_id, pred_id, n_gid, n_pid, id_iou=0.5):
    """-> (gc int32 [n_gid], pc int32 [n_pid]: frames holding each id; C int32 [n_gid, n_pid]: frames with S_t[g,p] >= id_iou;
    status int32 [2] = (code, first frame): MOT_DUPLICATE_ID where an id occurs twice in a frame on one side)."""
    mot_assoc_dims("mot_id_counts", n_gid, n_pid)
    offs, sizes = _assoc_layout("mot_id_counts", offsets, totals, gt_id, pred_id, iou)
    dev = gt_id.device
    gc = torch.empty(n_gid, dtype=torch.int32, device=dev)
    pc = torch.empty(n_pid, dtype=torch.int32, device=dev)
    C = torch.empty((n_gid, n_pid), dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _hip.call("rn_mot_id_counts", iou, *offs, *sizes, gt_id, pred_id, n_gid, n_pid, float(id_iou), gc, pc, C, status, device=dev)
    return gc, pc, C, status


def _assoc_workspace(n_gid, n_pid, dev):
    return torch.empty(max(16, _hip.load().rn_mot_assoc_workspace_bytes(n_gid, n_pid)), dtype=torch.uint8, device=dev)


def mot_id_assign(C):
    """linear_sum_assignment(C, maximize=True) on the id x id counts, one wave -> (match int32 [n_gid]: the prediction id matched
    to each ground-truth id or -1; info int64 [2] = (IDTP, status))."""
    _hip.need_gpu(C)
    _typed("mot_id_assign", ("C", C, torch.int32))
    if C.dim() != 2:
        raise RuntimeError("mot_id_assign: C is [n_gid, n_pid]")
    n_gid, n_pid = C.shape
    mot_assoc_dims("mot_id_assign", n_gid, n_pid)
    dev = C.device
    ws = _assoc_workspace(n_gid, n_pid, dev)
    match = torch.empty(n_gid, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    _hip.call("rn_mot_id_assign", C, n_gid, n_pid, ws, match, info, device=dev)
    return match, info


def mot_id_csr(n_gt, n_pred, gt_id, n_gid):
    """Host: per ground-truth id its appearances over the scored frames (both sides present) as a CSR in ascending frame order
    -> (csr_off int32 [n_gid + 1], csr_frame, csr_row int32 [n]) numpy arrays.  gt_id: the packed dense ids, a host array."""
    ng, npr = np.asarray(n_gt, np.int64).reshape(-1), np.asarray(n_pred, np.int64).reshape(-1)
    gid = np.asarray(gt_id, np.int64).reshape(-1)
    frame = np.repeat(np.arange(len(ng)), ng)
    row = np.arange(len(gid)) - np.repeat(np.cumsum(ng) - ng, ng)
    keep = (npr[frame] > 0) & (gid >= 0) & (gid < n_gid) if len(gid) else np.zeros(0, bool)
    frame, row, gid = frame[keep], row[keep], gid[keep]
    order = np.argsort(gid, kind="stable")                                  # objects are in frame order already
    off = np.concatenate(([0], np.cumsum(np.bincount(gid, minlength=n_gid)))) if n_gid else np.zeros(1)
    return off.astype(np.int32), frame[order].astype(np.int32), row[order].astype(np.int32)


def mot_hota_align(iou, offsets, totals, gt_id, pred_id, csr, n_gid, n_pid):
    """The potential-match sums of HOTA's global alignment -> (pot fp64 [n_gid, n_pid], status int32 [2]).  csr = (csr_off,
    csr_frame, csr_row) int32 device tensors (mot_id_csr); row g of pot is summed by one workgroup in ascending frame order."""
    mot_assoc_dims("mot_hota_align", n_gid, n_pid)
    offs, sizes = _assoc_layout("mot_hota_align", offsets, totals, gt_id, pred_id, iou)
    csr_off, csr_frame, csr_row = csr
    _hip.need_gpu(*csr)
    _typed("mot_hota_align", ("csr_off", csr_off, torch.int32), ("csr_frame", csr_frame, torch.int32), ("csr_row", csr_row, torch.int32))
    if csr_off.numel() != n_gid + 1 or csr_frame.numel() != csr_row.numel():
        raise RuntimeError("mot_hota_align: csr_off [n_gid + 1], csr_frame and csr_row of one length")
    dev = gt_id.device
    rowsum = torch.empty(gt_id.numel(), dtype=torch.float64, device=dev)
    colsum = torch.empty(pred_id.numel(), dtype=torch.float64, device=dev)
    pot = torch.empty((n_gid, n_pid), dtype=torch.float64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _hip.call("rn_mot_hota_align", iou, *offs, *sizes, gt_id, pred_id, csr_off, csr_frame, csr_row, csr_frame.numel(), n_gid, n_pid,
              rowsum, colsum, pot, status, device=dev)
    return pot, status


def mot_hota_assign(iou, offsets, totals, gt_id, pred_id, gc, pc, pot, alphas):
    """Per scored frame linear_sum_assignment(-(ga * S)), ga = pot / ((gc + pc) - pot) -> (slot_row, slot_col int32 [S], slot_s
    fp64 [S]: the pair's S, slot_n int32 [S]: how many of the ascending alphas pass S >= alpha - 2^-52, frame_status int32 [F])."""
    _hip.need_gpu(gc, pc, pot, alphas)
    _typed("mot_hota_assign", ("gc", gc, torch.int32), ("pc", pc, torch.int32), ("pot", pot, torch.float64),
           ("alphas", alphas, torch.float64))
    n_gid, n_pid = gc.numel(), pc.numel()
    mot_assoc_dims("mot_hota_assign", n_gid, n_pid)
    if pot.numel() != n_gid * n_pid or alphas.numel() != MOT_ALPHAS:
        raise RuntimeError("mot_hota_assign: pot [n_gid, n_pid], alphas [%d]" % MOT_ALPHAS)
    offs, sizes = _assoc_layout("mot_hota_assign", offsets, totals, gt_id, pred_id, iou)
    dev, F, S = gt_id.device, sizes[0], sizes[5]
    score = torch.empty(sizes[4], dtype=torch.float64, device=dev)
    slot_row = torch.empty(S, dtype=torch.int32, device=dev)
    slot_col = torch.empty(S, dtype=torch.int32, device=dev)
    slot_s = torch.empty(S, dtype=torch.float64, device=dev)
    slot_n = torch.empty(S, dtype=torch.int32, device=dev)
    frame_status = torch.zeros(F, dtype=torch.int32, device=dev)
    _hip.call("rn_mot_hota_assign", iou, *offs, *sizes, gt_id, pred_id, n_gid, n_pid, gc, pc, pot, alphas, score, slot_row, slot_col,
              slot_s, slot_n, frame_status, device=dev)
    return slot_row, slot_col, slot_s, slot_n, frame_status


def mot_hota_reduce(offsets, totals, assigned, gt_id, pred_id, gc, pc):
    """assigned = what mot_hota_assign returns -> result fp64 [MOT_ASSOC_RESULT] on the device: per alpha (TP, FN, FP, Loc,
    AssA-sum, AssRe-sum, AssPr-sum), then the status and the first frame with one (layout: include/retinanet_mi355x.h)."""
    slot_row, slot_col, slot_s, slot_n, frame_status = assigned
    _hip.need_gpu(gc, pc, *assigned)
    _typed("mot_hota_reduce", ("gc", gc, torch.int32), ("pc", pc, torch.int32), ("slot_row", slot_row, torch.int32),
           ("slot_col", slot_col, torch.int32), ("slot_s", slot_s, torch.float64), ("slot_n", slot_n, torch.int32),
           ("frame_status", frame_status, torch.int32))
    n_gid, n_pid = gc.numel(), pc.numel()
    mot_assoc_dims("mot_hota_reduce", n_gid, n_pid)
    offs, sizes = _assoc_layout("mot_hota_reduce", offsets, totals, gt_id, pred_id)
    F, S = sizes[0], sizes[5]
    if frame_status.numel() != F or any(t.numel() != S for t in (slot_row, slot_col, slot_s, slot_n)):
        raise RuntimeError("mot_hota_reduce: frame_status [F = %d] and the four slot arrays [S = %d]" % (F, S))
    dev = gt_id.device
    ws = _assoc_workspace(n_gid, n_pid, dev)
    result = torch.empty(MOT_ASSOC_RESULT, dtype=torch.float64, device=dev)
    _hip.call("rn_mot_hota_reduce", *offs, *sizes, frame_status, slot_row, slot_col, slot_s, slot_n, gt_id, pred_id, gc, pc, n_gid,
              n_pid, ws, result, device=dev)
    return result


# ------------------------------------------------------------------------------------------------ tracking CSV resampling
REINTERP_TILE = 1024               # RN_REINTERP_TILE: ids of the next frame per LDS tile
REINTERP_BAD_OFFSETS, REINTERP_BAD_PAIR, REINTERP_BAD_MATE, REINTERP_BAD_PREFIX, REINTERP_BAD_MAT_INDEX = 1, 2, 4, 8, 16
_REINTERP_BITS = ((REINTERP_BAD_OFFSETS, "frame offsets out of order or outside the rows"),
                  (REINTERP_BAD_PAIR, "an instant's frame pair outside the frames"),
                  (REINTERP_BAD_MATE, "a mate outside the next frame"),
                  (REINTERP_BAD_PREFIX, "a destination outside its prefix slot"),
                  (REINTERP_BAD_MAT_INDEX, "a mat_index outside the matrices"))


def reinterp_status(device, status=None):
    """The status word the four entry points OR their bits into: a zeroed int32 [1] unless one is handed on."""
    return _status_word("reinterp", device, status)


def reinterp_check(status):
    """Raises on a non-zero status word (an int, or the int32 [1] tensor: one element is read back)."""
    _refused("the resampling kernels refused their input: ", _REINTERP_BITS, status)


def _reinterp_frames(what, offsets, R):
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise RuntimeError("%s: offsets is int64 [F+1]" % what)
    if R >= 2 ** 31 or offsets.numel() - 1 >= 2 ** 31:
        raise RuntimeError("%s: more than 2^31 rows or frames" % what)
    return offsets.numel() - 1


def reinterp_mate(offsets, ids, status=None):
    """datareader.py:416-417 for every row: offsets int64 [F+1], ids int64 [R] -> (mate int32 [R] = the row of the next frame
    with the same id or -1, status)."""
    _hip.need_gpu(offsets, ids)
    _typed("reinterp_mate", ("offsets", offsets, torch.int64), ("ids", ids, torch.int64))
    if ids.dim() != 1:
        raise RuntimeError("reinterp_mate: ids is int64 [R]")
    R, F, dev = ids.numel(), _reinterp_frames("reinterp_mate", offsets, ids.numel()), ids.device
    status = reinterp_status(dev, status)
    mate = torch.empty(R, dtype=torch.int32, device=dev)
    _hip.call("rn_reinterp_mate", offsets, ids, F, R, mate, status, device=dev)
    return mate, status


def reinterp_offsets(offsets, mate, inst_a, status=None):
    """offsets int64 [F+1], mate int32 [R], inst_a int32 [T] -> (count int32 [T] = mated rows of frame inst_a[t], prefix int64
    [T+1] = its exclusive prefix, status)."""
    _hip.need_gpu(offsets, mate, inst_a)
    _typed("reinterp_offsets", ("offsets", offsets, torch.int64), ("mate", mate, torch.int32), ("inst_a", inst_a, torch.int32))
    if mate.dim() != 1 or inst_a.dim() != 1:
        raise RuntimeError("reinterp_offsets: mate is int32 [R], inst_a int32 [T]")
    R, T, F, dev = mate.numel(), inst_a.numel(), _reinterp_frames("reinterp_offsets", offsets, mate.numel()), mate.device
    if T >= 2 ** 31:
        raise RuntimeError("reinterp_offsets: more than 2^31 instants")
    status = reinterp_status(dev, status)
    frame_count = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
    count = torch.empty(T, dtype=torch.int32, device=dev)
    prefix = torch.empty(T + 1, dtype=torch.int64, device=dev)
    _hip.call("rn_reinterp_offsets", offsets, mate, F, R, inst_a, T, frame_count, count, prefix, status, device=dev)
    return count, prefix, status


def reinterp_rows(offsets, frame_ts, fields, mate, inst_a, inst_time, prefix, rows, status=None):
    """datareader.py:418-430 for every instant: frame_ts fp64 [F], fields fp64 [R,6], inst_time fp64 [T], prefix as
    reinterp_offsets returns it, rows = the size of the output (at least prefix[T]; the host's upper bound, so that nothing
    is read back in between) -> (out_fields fp64 [rows,6], out_src int32 [rows], out_inst int32 [rows], status); only rows
    below prefix[T] are written."""
    _hip.need_gpu(offsets, frame_ts, fields, mate, inst_a, inst_time, prefix)
    _typed("reinterp_rows", ("offsets", offsets, torch.int64), ("frame_ts", frame_ts, torch.float64),
           ("fields", fields, torch.float64), ("mate", mate, torch.int32), ("inst_a", inst_a, torch.int32),
           ("inst_time", inst_time, torch.float64), ("prefix", prefix, torch.int64))
    R, T, dev = mate.numel(), inst_a.numel(), fields.device
    F = _reinterp_frames("reinterp_rows", offsets, R)
    rows = int(rows)
    if fields.numel() != R * 6 or frame_ts.numel() != F or inst_time.numel() != T or prefix.numel() != T + 1 or rows < 0 \
            or T >= 2 ** 31:
        raise RuntimeError("reinterp_rows: frame_ts [F], fields [R,6], mate [R], inst_a / inst_time [T], prefix [T+1], rows >= 0")
    status = reinterp_status(dev, status)
    out_fields = torch.empty((rows, 6), dtype=torch.float64, device=dev)
    out_src = torch.empty(rows, dtype=torch.int32, device=dev)
    out_inst = torch.empty(rows, dtype=torch.int32, device=dev)
    _hip.call("rn_reinterp_rows", offsets, frame_ts, fields, mate, inst_a, inst_time, prefix, F, R, T, rows, out_fields, out_src,
              out_inst, status, device=dev)
    return out_fields, out_src, out_inst, status


def track_rows(fields, direction, P, P2=None, mat_index=None, status=None):
    """datareader.py:530-550 for N rows: fields fp64 [N,6] (x, y, l, w, h, v), direction fp64 [N], P fp64 [n,3,4] (P2: the
    Homography_Wrapper's second set), mat_index int32 [N] or None (matrix 0) -> (state fp32 [N,7], space fp32 [N,4,2], im fp64
    [N,8,2], box fp64 [N,4], keep uint8 [N], status)."""
    _hip.need_gpu(fields, direction, P, P2, mat_index)
    _typed("track_rows", ("fields", fields, torch.float64), ("direction", direction, torch.float64), ("P", P, torch.float64))
    if P2 is not None:
        _typed("track_rows", ("P2", P2, torch.float64))
    if mat_index is not None:
        _typed("track_rows", ("mat_index", mat_index, torch.int32))
    N, dev = direction.numel(), fields.device
    if P.dim() != 3 or tuple(P.shape[1:]) != (3, 4) or P.shape[0] < 1 or (P2 is not None and P2.shape != P.shape) \
            or fields.numel() != N * 6 or direction.dim() != 1 or (mat_index is not None and tuple(mat_index.shape) != (N,)):
        raise RuntimeError("track_rows: fields [N,6], direction [N], P (and P2) [n,3,4], mat_index [N]")
    status = reinterp_status(dev, status)
    state = torch.empty((N, 7), dtype=torch.float32, device=dev)
    space = torch.empty((N, 4, 2), dtype=torch.float32, device=dev)
    im = torch.empty((N, 8, 2), dtype=torch.float64, device=dev)
    box = torch.empty((N, 4), dtype=torch.float64, device=dev)
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    _hip.call("rn_track_rows", fields, direction, mat_index, P, P2, P.shape[0], N, state, space, im, box, keep, status, device=dev)
    return state, space, im, box, keep, status


# ------------------------------------------------------------------------------------------------ track stitching
STITCH_EP = 16                     # RN_STITCH_EP: doubles of one end point
STITCH_MAX_TRACKLETS = 32768
STITCH_MAX_FIT = 64
STITCH_MAX_FILL = 1048576
STITCH_DENSE_MAX = 8192            # stitch_costs only: the dense matrix stays below 512 MiB
(STITCH_NONFINITE, STITCH_BAD_OFFSETS, STITCH_TOO_MANY, STITCH_SOLVER, STITCH_BAD_CANDIDATES, STITCH_BAD_LINK, STITCH_BAD_PREFIX,
 STITCH_FILL_OVERFLOW) = 1, 2, 4, 8, 16, 32, 64, 128
_STITCH_BITS = ((STITCH_NONFINITE, "a NaN or an infinity among the packed fields"),
                (STITCH_BAD_OFFSETS, "tracklet offsets out of order, an empty tracklet or rows outside the packed ones"),
                (STITCH_TOO_MANY, "more than %d tails and heads with a candidate in one direction" % LSAP_MAX_MIN),
                (STITCH_SOLVER, "the assignment found no complete matching"),
                (STITCH_BAD_CANDIDATES, "candidate counts or entries outside the tracklets"),
                (STITCH_BAD_LINK, "a link outside the tracklets"),
                (STITCH_BAD_PREFIX, "a new row outside its prefix slot"),
                (STITCH_FILL_OVERFLOW, "a link with %d new rows or more" % STITCH_MAX_FILL))
STITCH_SCALES = ("max_gap", "back_tol", "sigma_x0", "sigma_x1", "sigma_y", "sigma_size", "max_cost")


def stitch_status(device, status=None):
    """The status word the stitching entry points OR their bits into: a zeroed int32 [1] unless one is handed on."""
    return _status_word("stitch", device, status)


def stitch_check(status):
    """Raises on a non-zero status word (an int, or the int32 [1] tensor: one element is read back)."""
    _refused("the stitching kernels refused their input: ", _STITCH_BITS, status)


def stitch_scales(scales):
    """The seven scales of a link cost in STITCH_SCALES order, as floats; ValueError unless back_tol >= 0 and the others > 0."""
    s = tuple(float(v) for v in scales)
    if len(s) != len(STITCH_SCALES):
        raise ValueError("a link cost takes the seven scales %s" % (STITCH_SCALES,))
    for name, v in zip(STITCH_SCALES, s):
        if not (v >= 0 if name == "back_tol" else v > 0) or v == float("inf"):
            raise ValueError("stitching scale %s must be a positive finite number, got %r" % (name, v))
    return s


def _stitch_ep(what, ep):
    _hip.need_gpu(ep)
    _typed(what, ("ep", ep, torch.float64))
    if ep.dim() != 3 or tuple(ep.shape[1:]) != (2, STITCH_EP):
        raise RuntimeError("%s: ep is fp64 [N,2,%d], got %s" % (what, STITCH_EP, tuple(ep.shape)))
    if ep.shape[0] > STITCH_MAX_TRACKLETS:
        raise RuntimeError("%s: at most %d tracklets, got %d" % (what, STITCH_MAX_TRACKLETS, ep.shape[0]))
    return ep.shape[0], ep.device


def _stitch_int(what, N, *specs):
    for name, t in specs:
        _hip.need_gpu(t)
        _typed(what, (name, t, torch.int32))
        if tuple(t.shape) != (N,):
            raise RuntimeError("%s: %s is int32 [N = %d], got %s" % (what, name, N, tuple(t.shape)))


def stitch_endpoints(offsets, cols, direction, fit_n, status=None):
    """offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v), direction int32 [R] -> (ep fp64 [N,2,STITCH_EP] = the head
    and the tail of every tracklet (layout: include/retinanet_mi355x.h), status)."""
    _hip.need_gpu(offsets, cols, direction)
    _typed("stitch_endpoints", ("offsets", offsets, torch.int64), ("cols", cols, torch.float64), ("direction", direction, torch.int32))
    fit_n = int(fit_n)
    if not 1 <= fit_n <= STITCH_MAX_FIT:
        raise ValueError("fit_n is 1 .. %d, got %d" % (STITCH_MAX_FIT, fit_n))
    R = direction.numel()
    if offsets.dim() != 1 or offsets.numel() < 1 or cols.dim() != 2 or tuple(cols.shape) != (R, 7) or direction.dim() != 1 or R >= 2 ** 31:
        raise RuntimeError("stitch_endpoints: offsets int64 [N+1], cols fp64 [R,7], direction int32 [R], fewer than 2^31 rows")
    N, dev = offsets.numel() - 1, cols.device
    if N > STITCH_MAX_TRACKLETS:
        raise RuntimeError("stitch_endpoints: at most %d tracklets, got %d" % (STITCH_MAX_TRACKLETS, N))
    status = stitch_status(dev, status)
    ep = torch.empty((N, 2, STITCH_EP), dtype=torch.float64, device=dev)
    _hip.call("rn_stitch_endpoints", offsets, cols, direction, N, R, fit_n, ep, status, device=dev)
    return ep, status


def stitch_costs(ep, scales):
    """The dense matrix of every ordered pair (a's tail -> b's head): W fp64 [N,N], cost - max_cost for a linkable pair and 0
    otherwise.  For tests and small inputs (N <= STITCH_DENSE_MAX); the product path never materialises it."""
    N, dev = _stitch_ep("stitch_costs", ep)
    scales = stitch_scales(scales)
    if N > STITCH_DENSE_MAX:
        raise RuntimeError("stitch_costs: the dense matrix is for at most %d tracklets, got %d" % (STITCH_DENSE_MAX, N))
    W = torch.empty((N, N), dtype=torch.float64, device=dev)
    _hip.call("rn_stitch_costs", ep, N, *scales, W, device=dev)
    return W


def stitch_candidates(ep, scales):
    """-> (cand int32 [2,2,N]: per direction (sgn = +1 first) the tails and the heads with a candidate, ascending, -1 behind;
    ncand int32 [4] = (nr'+, nc'+, nr'-, nc'-))."""
    N, dev = _stitch_ep("stitch_candidates", ep)
    scales = stitch_scales(scales)
    has = torch.empty((2, N), dtype=torch.uint8, device=dev)
    cand = torch.empty((2, 2, N), dtype=torch.int32, device=dev)
    ncand = torch.empty(4, dtype=torch.int32, device=dev)
    _hip.call("rn_stitch_candidates", ep, N, *scales, has, cand, ncand, device=dev)
    return cand, ncand


def _stitch_cand(what, N, cand, ncand):
    _hip.need_gpu(cand, ncand)
    _typed(what, ("cand", cand, torch.int32), ("ncand", ncand, torch.int32))
    if tuple(cand.shape) != (2, 2, N) or tuple(ncand.shape) != (4,):
        raise RuntimeError("%s: cand int32 [2,2,N = %d], ncand int32 [4]" % (what, N))


def stitch_compact(ep, scales, cand, ncand, cap, status=None):
    """The compressed matrices: Wc fp64 [cap], direction + as [nr'+, nc'+] from 0 and direction - as [nr'-, nc'-] behind it; cap
    = the host's upper bound of the cells (n+ ^2 + n- ^2 of the tracklets per direction), so that nothing is read back in
    between.  -> (Wc, status)."""
    N, dev = _stitch_ep("stitch_compact", ep)
    scales = stitch_scales(scales)
    _stitch_cand("stitch_compact", N, cand, ncand)
    cap = int(cap)
    if cap < 0:
        raise RuntimeError("stitch_compact: cap >= 0")
    status = stitch_status(dev, status)
    Wc = torch.empty(cap, dtype=torch.float64, device=dev)
    _hip.call("rn_stitch_compact", ep, N, *scales, cand, ncand, cap, Wc, status, device=dev)
    return Wc, status


def stitch_assign(ep, scales, cand, ncand, Wc, status=None):
    """scipy.optimize.linear_sum_assignment on each direction's Wc; the links are the assigned cells with W < 0 -> (next int32
    [N], prev int32 [N] (-1: none), link_cost fp64 [N] at the tail's index, status)."""
    N, dev = _stitch_ep("stitch_assign", ep)
    scales = stitch_scales(scales)
    _stitch_cand("stitch_assign", N, cand, ncand)
    _hip.need_gpu(Wc)
    _typed("stitch_assign", ("Wc", Wc, torch.float64))
    status = stitch_status(dev, status)
    ws = torch.empty(max(int(_hip.load().rn_stitch_assign_workspace_bytes(N)), 16), dtype=torch.uint8, device=dev)
    nxt = torch.empty(N, dtype=torch.int32, device=dev)
    prev = torch.empty(N, dtype=torch.int32, device=dev)
    link_cost = torch.empty(N, dtype=torch.float64, device=dev)
    _hip.call("rn_stitch_assign", ep, N, *scales, cand, ncand, Wc, Wc.numel(), ws, nxt, prev, link_cost, status, device=dev)
    return nxt, prev, link_cost, status


def stitch_chains(prev, ids, status=None):
    """prev int32 [N], ids int64 [N] -> (root int32 [N] = the chain's earliest fragment, rank int32 [N] = the position in the
    chain, new_id int64 [N] = ids[root], status)."""
    N, dev = prev.numel(), prev.device
    _stitch_int("stitch_chains", N, ("prev", prev))
    _hip.need_gpu(ids)
    _typed("stitch_chains", ("ids", ids, torch.int64))
    if tuple(ids.shape) != (N,) or N > STITCH_MAX_TRACKLETS:
        raise RuntimeError("stitch_chains: ids is int64 [N], N <= %d" % STITCH_MAX_TRACKLETS)
    status = stitch_status(dev, status)
    ws = torch.empty(4 * max(N, 1), dtype=torch.int32, device=dev)
    root = torch.empty(N, dtype=torch.int32, device=dev)
    rank = torch.empty(N, dtype=torch.int32, device=dev)
    new_id = torch.empty(N, dtype=torch.int64, device=dev)
    _hip.call("rn_stitch_chains", prev, ids, N, ws, root, rank, new_id, status, device=dev)
    return root, rank, new_id, status


def _fill_rate(fill_rate):
    fill_rate = float(fill_rate)
    if not 0 < fill_rate < float("inf"):
        raise ValueError("fill_rate must be a positive finite number, got %r" % fill_rate)
    return fill_rate


def stitch_fill_count(ep, nxt, fill_rate, status=None):
    """-> (count int32 [N] = the new rows of the link that starts at tracklet a's tail, prefix int64 [N+1], status)."""
    N, dev = _stitch_ep("stitch_fill_count", ep)
    _stitch_int("stitch_fill_count", N, ("next", nxt))
    fill_rate = _fill_rate(fill_rate)
    status = stitch_status(dev, status)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    prefix = torch.empty(N + 1, dtype=torch.int64, device=dev)
    _hip.call("rn_stitch_fill_count", ep, nxt, N, fill_rate, count, prefix, status, device=dev)
    return count, prefix, status


def stitch_fill_rows(ep, nxt, prefix, fill_rate, rows, status=None):
    """rows = the size of the output (at least prefix[N]; the host's upper bound) -> (fields fp64 [rows,6] in datareader.FIELDS
    order, time fp64 [rows], link int32 [rows] = the tail's tracklet, side uint8 [rows], status); only rows below prefix[N] are
    written."""
    N, dev = _stitch_ep("stitch_fill_rows", ep)
    _stitch_int("stitch_fill_rows", N, ("next", nxt))
    _hip.need_gpu(prefix)
    _typed("stitch_fill_rows", ("prefix", prefix, torch.int64))
    fill_rate, rows = _fill_rate(fill_rate), int(rows)
    if tuple(prefix.shape) != (N + 1,) or rows < 0:
        raise RuntimeError("stitch_fill_rows: prefix int64 [N+1], rows >= 0")
    status = stitch_status(dev, status)
    fields = torch.empty((rows, 6), dtype=torch.float64, device=dev)
    time = torch.empty(rows, dtype=torch.float64, device=dev)
    link = torch.empty(rows, dtype=torch.int32, device=dev)
    side = torch.empty(rows, dtype=torch.uint8, device=dev)
    _hip.call("rn_stitch_fill_rows", ep, nxt, prefix, N, rows, fill_rate, fields, time, link, side, status, device=dev)
    return fields, time, link, side, status


# ------------------------------------------------------------------------------------------------ fixed-interval smoothing
SMOOTH_MODEL = 97                  # RN_SMOOTH_MODEL: q_scale Q [6,6], r_scale R [5,5], P0 [6,6]
SMOOTH_FILT = 27                   # 6 filtered means + the 21 covariance entries a <= b
SMOOTH_OUT = 12                    # 6 smoothed means + 6 smoothed variances
SMOOTH_MAX_TRACKLETS = 1048576
SMOOTH_NONFINITE, SMOOTH_BAD_OFFSETS, SMOOTH_BAD_DT, SMOOTH_PIVOT, SMOOTH_BAD_ORDER = 1, 2, 4, 8, 16
_SMOOTH_BITS = ((SMOOTH_NONFINITE, "a NaN or an infinity among the packed fields"),
                (SMOOTH_BAD_OFFSETS, "tracklet offsets out of order, an empty tracklet or rows outside the packed ones"),
                (SMOOTH_BAD_DT, "a repeated or decreasing time stamp inside a tracklet"),
                (SMOOTH_PIVOT, "a covariance that is not positive definite (a pivot <= 0)"),
                (SMOOTH_BAD_ORDER, "an order entry outside the tracklets"))


def smooth_status(device, status=None):
    """The status word the smoothing entry points OR their bits into: a zeroed int32 [1] unless one is handed on."""
    return _status_word("smooth", device, status)


def smooth_check(status):
    """Raises on a non-zero status word (an int, or the int32 [1] tensor: one element is read back)."""
    _refused("the smoothing kernels refused their input: ", _SMOOTH_BITS, status)


def smooth_model(kf_params, q_scale=1.0, r_scale=1.0):
    """The packed model block of the smoother, a host fp64 array [SMOOTH_MODEL] = q_scale Q [6,6], r_scale R [5,5], P0 = P [6,6],
    row-major.  ``kf_params`` is what ``Torch_KF(INIT=...)`` takes (fit_filter.fit): its float32 ``Q``, ``R`` and ``P`` are widened
    exactly; ``H`` is not read (the measurement is the row's x, y, l, w, h: H = [I5 | 0]), nor are ``mu_Q`` / ``mu_R``.  ValueError
    on a wrong shape, a non-finite entry, a non-positive scale or an asymmetric matrix."""
    scales = []
    for name, v in (("q_scale", q_scale), ("r_scale", r_scale)):
        v = float(v)
        if not 0 < v < float("inf"):
            raise ValueError("%s must be a positive finite number, got %r" % (name, v))
        scales.append(v)
    mats = []
    for name, n in (("Q", 6), ("R", 5), ("P", 6)):
        if name not in kf_params:
            raise ValueError("kf_params holds no %r" % name)
        m = kf_params[name]
        m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
        if m.shape != (n, n):
            raise ValueError("kf_params[%r] is [%d,%d], got %s" % (name, n, n, tuple(m.shape)))
        m = m.astype(np.float64)
        if not np.isfinite(m).all():
            raise ValueError("kf_params[%r] holds a NaN or an infinity" % name)
        if not np.array_equal(m, m.T):
            raise ValueError("kf_params[%r] is not symmetric" % name)
        mats.append(m)
    return np.concatenate(((scales[0] * mats[0]).reshape(-1), (scales[1] * mats[1]).reshape(-1), mats[2].reshape(-1)))


def _smooth_inputs(what, offsets, order, cols, direction, model, dt_default):
    _hip.need_gpu(offsets, order, cols, direction, model)
    _typed(what, ("offsets", offsets, torch.int64), ("order", order, torch.int32), ("cols", cols, torch.float64),
           ("direction", direction, torch.int32), ("model", model, torch.float64))
    R = direction.numel()
    if offsets.dim() != 1 or offsets.numel() < 1 or cols.dim() != 2 or tuple(cols.shape) != (R, 7) or direction.dim() != 1 \
            or R >= 2 ** 31 or tuple(order.shape) != (offsets.numel() - 1,) or tuple(model.shape) != (SMOOTH_MODEL,):
        raise RuntimeError("%s: offsets int64 [N+1], order int32 [N], cols fp64 [R,7], direction int32 [R], model fp64 [%d], fewer "
                           "than 2^31 rows" % (what, SMOOTH_MODEL))
    N = offsets.numel() - 1
    if N > SMOOTH_MAX_TRACKLETS:
        raise RuntimeError("%s: at most %d tracklets, got %d" % (what, SMOOTH_MAX_TRACKLETS, N))
    dt_default = float(dt_default)
    if not 0 < dt_default < float("inf"):
        raise ValueError("dt_default must be a positive finite number, got %r" % dt_default)
    return N, R, cols.device, dt_default


def smooth_filter(offsets, order, cols, direction, model, gate, dt_default, status=None):
    """The forward pass.  offsets int64 [N+1], order int32 [N] (lane i works on tracklet order[i]; track_smooth.lane_order gives the
    stable argsort of descending length, any permutation gives the same bytes), cols fp64 [R,7]
    = (t, x, y, l, w, h, v), direction int32 [R], model fp64 [SMOOTH_MODEL] (``smooth_model``, uploaded), gate >= 0 (0: no gating)
    -> (filt fp64 [R,SMOOTH_FILT], nis fp64 [R], flag uint8 [R], status)."""
    N, R, dev, dt_default = _smooth_inputs("smooth_filter", offsets, order, cols, direction, model, dt_default)
    gate = float(gate)
    if not 0 <= gate < float("inf"):
        raise ValueError("gate is 0 (off) or a positive finite number, got %r" % gate)
    status = smooth_status(dev, status)
    filt = torch.zeros((R, SMOOTH_FILT), dtype=torch.float64, device=dev)
    nis = torch.zeros(R, dtype=torch.float64, device=dev)
    flag = torch.zeros(R, dtype=torch.uint8, device=dev)
    _hip.call("rn_smooth_filter", offsets, order, cols, direction, model, gate, dt_default, N, R, filt, nis, flag, status, device=dev)
    return filt, nis, flag, status


def smooth_rts(offsets, order, cols, direction, model, dt_default, filt, status=None):
    """The backward pass over ``smooth_filter``'s filt -> (out fp64 [R,SMOOTH_OUT] = the 6 smoothed means and variances, status)."""
    N, R, dev, dt_default = _smooth_inputs("smooth_rts", offsets, order, cols, direction, model, dt_default)
    _hip.need_gpu(filt)
    _typed("smooth_rts", ("filt", filt, torch.float64))
    if tuple(filt.shape) != (R, SMOOTH_FILT):
        raise RuntimeError("smooth_rts: filt is fp64 [R = %d, %d], got %s" % (R, SMOOTH_FILT, tuple(filt.shape)))
    status = smooth_status(dev, status)
    out = torch.zeros((R, SMOOTH_OUT), dtype=torch.float64, device=dev)
    _hip.call("rn_smooth_rts", offsets, order, cols, direction, model, dt_default, N, R, filt, out, status, device=dev)
    return out, status


# ------------------------------------------------------------------------------------------------ traffic state
TRAFFIC_Q = 1 << 20                # RN_TRAFFIC_Q: the fixed-point unit of T and D is 2^-20 s or ft
TRAFFIC_COUNTERS = 8
TRAFFIC_MAX_EDGES = 64
TRAFFIC_MAX_CUTS = 4096
TRAFFIC_CELL_COUNTERS = ("segments", "used", "skipped_gap", "skipped_lane", "pieces", "outside")
TRAFFIC_LEADER_COUNTERS = ("with_leader", "overlaps")
TRAFFIC_NONFINITE, TRAFFIC_BAD_OFFSETS, TRAFFIC_BAD_FRAME, TRAFFIC_TOO_MANY_CUTS, TRAFFIC_RANGE, TRAFFIC_BAD_DIR = 1, 2, 4, 8, 16, 32
_TRAFFIC_BITS = ((TRAFFIC_NONFINITE, "a NaN or an infinity among the packed fields"),
                 (TRAFFIC_BAD_OFFSETS, "tracklet offsets out of order or not covering the packed rows"),
                 (TRAFFIC_BAD_FRAME, "frame offsets out of order or a frame row outside the packed rows"),
                 (TRAFFIC_TOO_MANY_CUTS, "a segment that crosses more than %d grid lines" % TRAFFIC_MAX_CUTS),
                 (TRAFFIC_RANGE, "a segment of 2^20 s or ft or more"),
                 (TRAFFIC_BAD_DIR, "a tracklet direction that is neither +1 nor -1"))


def traffic_status(device, status=None):
    """The status word the traffic entry points OR their bits into: a zeroed int32 [1] unless one is handed on."""
    return _status_word("traffic", device, status)


def traffic_check(status):
    """Raises on a non-zero status word (an int, or the int32 [1] tensor: one element is read back)."""
    _refused("the traffic kernels refused their input: ", _TRAFFIC_BITS, status)


def _traffic_inputs(what, offsets, cols, edges_pos, edges_neg):
    _hip.need_gpu(offsets, cols, edges_pos, edges_neg)
    _typed(what, ("offsets", offsets, torch.int64), ("cols", cols, torch.float64), ("edges_pos", edges_pos, torch.float64),
           ("edges_neg", edges_neg, torch.float64))
    if offsets.dim() != 1 or offsets.numel() < 1 or cols.dim() != 2 or cols.shape[1] != 7 or cols.shape[0] >= 2 ** 31 \
            or edges_pos.dim() != 1 or edges_neg.dim() != 1 or max(edges_pos.numel(), edges_neg.numel()) > TRAFFIC_MAX_EDGES:
        raise RuntimeError("%s: offsets int64 [N+1], cols fp64 [R,7], fewer than 2^31 rows, edges_pos and edges_neg fp64 with at most %d "
                           "entries each" % (what, TRAFFIC_MAX_EDGES))
    return offsets.numel() - 1, cols.shape[0], cols.device, max(edges_pos.numel(), edges_neg.numel(), 1) - 1


def _traffic_dir(what, N, dir):
    _hip.need_gpu(dir)
    _typed(what, ("dir", dir, torch.int32))
    if tuple(dir.shape) != (N,):
        raise RuntimeError("%s: dir is int32 [N = %d], got %s" % (what, N, tuple(dir.shape)))


def traffic_lanes(offsets, cols, direction, edges_pos, edges_neg, status=None):
    """offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v), direction int32 [R], the ascending lane edges of direction +1
    and -1 -> (dir int32 [N] = +1 when the tracklet's directions sum to >= 0 else -1, lane int32 [R] = the k with edges[k] <= y <
    edges[k+1] of the row's own y under its tracklet's dir, else -1; status)."""
    N, R, dev, _ = _traffic_inputs("traffic_lanes", offsets, cols, edges_pos, edges_neg)
    _hip.need_gpu(direction)
    _typed("traffic_lanes", ("direction", direction, torch.int32))
    if tuple(direction.shape) != (R,):
        raise RuntimeError("traffic_lanes: direction is int32 [R = %d], got %s" % (R, tuple(direction.shape)))
    status = traffic_status(dev, status)
    dir = torch.ones(N, dtype=torch.int32, device=dev)
    lane = torch.full((R,), -1, dtype=torch.int32, device=dev)
    _hip.call("rn_traffic_lanes", offsets, cols, direction, edges_pos, edges_pos.numel(), edges_neg, edges_neg.numel(), N, R, dir, lane,
              status, device=dev)
    return dir, lane, status


def traffic_cells(offsets, cols, dir, edges_pos, edges_neg, t0, dt, nt, x0, dx, nx, max_gap, status=None):
    """Edie's sums over the grid t0 + it dt (it < nt), x0 + ix dx (ix < nx): every segment (two consecutive rows of a tracklet, at
    most max_gap apart, with a lane) is cut at the grid lines it crosses and each piece adds its time and its distance in units of
    1 / TRAFFIC_Q to one cell -> (T int64 [2,L,nt,nx], D int64 [2,L,nt,nx], n int32 [2,L,nt,nx] = the pieces, counters int64
    [TRAFFIC_COUNTERS] in TRAFFIC_CELL_COUNTERS order, status); index 0 of the first axis is direction +1, L = the lanes of the longer
    edge array.  The rule: include/retinanet_mi355x.h, restated in tests/traffic_cases.py."""
    N, R, dev, L = _traffic_inputs("traffic_cells", offsets, cols, edges_pos, edges_neg)
    _traffic_dir("traffic_cells", N, dir)
    t0, dt, x0, dx, max_gap, nt, nx = float(t0), float(dt), float(x0), float(dx), float(max_gap), int(nt), int(nx)
    inf = float("inf")
    if not (abs(t0) < inf and abs(x0) < inf and 0 < dt < inf and 0 < dx < inf and max_gap > 0):
        raise ValueError("traffic_cells: t0 and x0 finite, dt and dx positive and finite, max_gap positive")
    if nt < 0 or nx < 0 or 2 * L * nt * nx >= 2 ** 31:
        raise RuntimeError("traffic_cells: a grid of 2 x %d x %d x %d cells; fewer than 2^31 are supported" % (L, nt, nx))
    status = traffic_status(dev, status)
    T = torch.zeros((2, L, nt, nx), dtype=torch.int64, device=dev)
    D = torch.zeros((2, L, nt, nx), dtype=torch.int64, device=dev)
    n = torch.zeros((2, L, nt, nx), dtype=torch.int32, device=dev)
    counters = torch.zeros(TRAFFIC_COUNTERS, dtype=torch.int64, device=dev)
    _hip.call("rn_traffic_cells", offsets, cols, dir, edges_pos, edges_pos.numel(), edges_neg, edges_neg.numel(), N, R, t0, dt, nt, x0, dx,
              nx, max_gap, T, D, n, counters, status, device=dev)
    return T, D, n, counters, status


def traffic_leaders(offsets, cols, dir, lane, frame_off, frame_rows, status=None):
    """Every frame taken as one instant: frame_off int64 [F+1] into frame_rows int32 [Rf], the packed rows of each frame (every row
    at most once).  For a row the leader is the nearest row ahead of it (dir (x_j - x) > 0) in the same frame, direction and lane
    >= 0, ties to the smaller tracklet -> (leader int32 [R] = the packed row or -1, spacing, gap = spacing - l, headway = spacing / v
    (inf unless v > 0), ttc = gap / (v - v_leader) (inf unless closing with gap > 0): fp64 [R], inf without a leader; counters int64
    [TRAFFIC_COUNTERS] in TRAFFIC_LEADER_COUNTERS order, status)."""
    _hip.need_gpu(offsets, cols, lane, frame_off, frame_rows)
    _typed("traffic_leaders", ("offsets", offsets, torch.int64), ("cols", cols, torch.float64), ("lane", lane, torch.int32),
           ("frame_off", frame_off, torch.int64), ("frame_rows", frame_rows, torch.int32))
    if offsets.dim() != 1 or offsets.numel() < 1 or cols.dim() != 2 or cols.shape[1] != 7 or cols.shape[0] >= 2 ** 31 \
            or tuple(lane.shape) != (cols.shape[0],) or frame_off.dim() != 1 or frame_off.numel() < 1 or frame_off.numel() > 2 ** 31 \
            or frame_rows.dim() != 1 or frame_rows.numel() >= 2 ** 31:
        raise RuntimeError("traffic_leaders: offsets int64 [N+1], cols fp64 [R,7], lane int32 [R], frame_off int64 [F+1], frame_rows int32 "
                           "[Rf], fewer than 2^31 rows and frames")
    N, R, dev = offsets.numel() - 1, cols.shape[0], cols.device
    _traffic_dir("traffic_leaders", N, dir)
    status = traffic_status(dev, status)
    leader = torch.full((R,), -1, dtype=torch.int32, device=dev)
    spacing, gap, headway, ttc = (torch.full((R,), float("inf"), dtype=torch.float64, device=dev) for _ in range(4))
    counters = torch.zeros(TRAFFIC_COUNTERS, dtype=torch.int64, device=dev)
    _hip.call("rn_traffic_leaders", offsets, cols, dir, lane, frame_off, frame_rows, N, R, frame_off.numel() - 1, frame_rows.numel(), leader,
              spacing, gap, headway, ttc, counters, status, device=dev)
    return leader, spacing, gap, headway, ttc, counters, status


# ------------------------------------------------------------------------------------------------ time stamp bias
TS_MAX_CAMS = 1024                # RN_TS_MAX_CAMS
TS_OK, TS_OVERFLOW, TS_BAD_CAMERA = 0, 1, 2


def estimate_ts_bias(boxes, camera_idxs, objs, timestamps, ts_bias, phi, alpha, mu_v, count=None, max_pairs=None,
                     details=False):
    """MC_Crop_Tracker.estimate_ts_bias (MC3D_crop_tracker.py:237-315) on the device, see include/retinanet_mi355x.h.
    boxes [d, >=6] fp32 states and camera_idxs [d] as the parser leaves them before the space NMS; objs [n, >=7] =
    Torch_KF.view(with_direction=True); timestamps [n_cam] fp64; ts_bias [n_cam] fp64 contiguous, UPDATED IN PLACE;
    count = the parser's device int32 count (rows valid) or None.  max_pairs sizes the pair buffer (default max(256, d)).
    -> info int32 [2] = (number of pairs, status) on the device, no synchronisation; status TS_OVERFLOW (more pairs than
    max_pairs) and TS_BAD_CAMERA leave ts_bias untouched.  details=True -> (info, pairs [max_pairs,2] int32 (i, j),
    time_error [max_pairs,2] fp32 of each pair's two entries)."""
    lib = _hip.load()
    _hip.need_gpu(boxes, camera_idxs, objs, timestamps, ts_bias, count)
    if boxes.dim() != 2 or boxes.shape[1] < 6 or camera_idxs.shape[0] != boxes.shape[0]:
        raise RuntimeError("estimate_ts_bias: boxes are [d, >= 6] with one camera index each, got %s and %s"
                           % (tuple(boxes.shape), tuple(camera_idxs.shape)))
    d = boxes.shape[0]
    n = 0 if objs is None else objs.shape[0]
    if n and (objs.dim() != 2 or objs.shape[1] < 7):
        raise RuntimeError("estimate_ts_bias: the filter view is [n, >= 7] (direction at 5, speed at 6), got %s" % (tuple(objs.shape),))
    if d > PARSE_MAX:
        raise RuntimeError("estimate_ts_bias takes at most %d detections, got %d" % (PARSE_MAX, d))
    n_cam = ts_bias.shape[0]
    if ts_bias.dtype != torch.float64 or not ts_bias.is_contiguous() or ts_bias.dim() != 1:
        raise RuntimeError("estimate_ts_bias updates ts_bias in place: it has to be a contiguous 1-D float64 tensor")
    if timestamps.shape[0] != n_cam or n_cam == 0 or n_cam > TS_MAX_CAMS:
        raise RuntimeError("estimate_ts_bias: %d timestamps for %d biases (1 .. %d cameras)" % (timestamps.shape[0], n_cam, TS_MAX_CAMS))
    dev = boxes.device
    mp = max(256, d) if max_pairs is None else int(max_pairs)
    if mp <= 0:
        raise RuntimeError("estimate_ts_bias: max_pairs has to be positive")
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    pairs = torch.full((mp, 2), -1, dtype=torch.int32, device=dev) if details else None
    te = torch.zeros((mp, 2), dtype=torch.float32, device=dev) if details else None
    if d and n:
        boxes, objs = _hip.f32c(boxes), _hip.f32c(objs)
        cams = camera_idxs.long().contiguous()
        ts = timestamps.double().contiguous()
        cnt = None if count is None else count.to(torch.int32).contiguous()
        ws = torch.empty(lib.rn_ts_bias_workspace_bytes(d, mp), dtype=torch.uint8, device=dev)
        _hip.call("rn_estimate_ts_bias", boxes, boxes.shape[1], cams, d, cnt, objs, objs.shape[1], n, ts, ts_bias, n_cam, float(phi),
                  float(alpha), float(mu_v), ws, mp, pairs, te, info, device=dev)
    return (info, pairs, te) if details else info


# ------------------------------------------------------------------------------------------------ crop frame front end
def track_crop_prior(X, D, T, F, centers, stamps, bias, pre_loc=None):
    """The start of a crop frame of MC_Crop_Tracker.track (MC3D_crop_tracker.py:1150-1171) on the device, see
    include/retinanet_mi355x.h.  X [n,6] fp32, D [n] fp32, T [n] fp64, F [6,6] fp32: the tensors of a ``Torch_KF``;
    centers [c,2] fp32; stamps / bias [c] fp64 (``timestamps`` and ``ts_bias``).  -> (pre_loc [n,7] fp32 = the filter's
    ``view(with_direction=True, dt=1/30.0)``, cam [n] int32 = the nearest camera centre, dt [n] fp64 = the per-object dt
    that rolls each track to its camera's corrected time stamp).  ``pre_loc``: an optional contiguous float32 [n,7] tensor to
    write the view into.  Device tensors, no synchronisation."""
    _hip.need_gpu(X, D, T, F, centers, stamps, bias, pre_loc)
    n = X.shape[0]
    for name, t, dtype, shape in (("X", X, torch.float32, (n, 6)), ("D", D, torch.float32, (n,)), ("T", T, torch.float64, (n,)),
                                  ("F", F, torch.float32, (6, 6))):
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise RuntimeError("track_crop_prior: %s has to be %s of shape %s, got %s %s" % (name, dtype, shape, t.dtype, tuple(t.shape)))
    c = centers.shape[0]
    if centers.dtype != torch.float32 or centers.dim() != 2 or centers.shape[1] != 2 or c < 1:
        raise RuntimeError("track_crop_prior: centers are float32 [c >= 1, 2], got %s %s" % (centers.dtype, tuple(centers.shape)))
    for name, t in (("stamps", stamps), ("bias", bias)):
        if t.dtype != torch.float64 or tuple(t.shape) != (c,):
            raise RuntimeError("track_crop_prior: %s has to be float64 of shape (%d,), got %s %s" % (name, c, t.dtype, tuple(t.shape)))
    dev = X.device
    if pre_loc is None:
        pre_loc = torch.empty((n, 7), dtype=torch.float32, device=dev)
    elif pre_loc.dtype != torch.float32 or tuple(pre_loc.shape) != (n, 7) or not pre_loc.is_contiguous():
        raise RuntimeError("track_crop_prior: pre_loc has to be a contiguous float32 [%d, 7]" % n)
    cam = torch.empty((n,), dtype=torch.int32, device=dev)
    dt = torch.empty((n,), dtype=torch.float64, device=dev)
    if n:
        X, D, T, F = X.contiguous(), D.contiguous(), T.contiguous(), F.contiguous()
        centers, stamps, bias = centers.contiguous(), stamps.contiguous(), bias.contiguous()
        _hip.call("rn_track_crop_prior", X, D, T, F, centers, stamps, bias, c, pre_loc, cam, dt, n, device=dev)
    return pre_loc, cam, dt


# ------------------------------------------------------------------------------------------------ fitting the filter
FIT_MAX = 1 << 24                  # RN_FIT_MAX
MOMENTS_MAX_K, MOMENTS_MAX_G = 8, 16


def fit_nearest(gt, det, offsets):
    """The nearest-box search of fit_filter_3D.py:356-375 on the device, see include/retinanet_mi355x.h.  gt [B, >=6]
    fp32 ground-truth states, one per frame; det [D, >=6] fp32 detection states; offsets [B+1] the CSR bounds of each
    frame's detections.  -> (rows int32 [B]: the chosen row of det or -1, resid fp32 [B,5]: det[row,:5] - gt[:, :5] of
    the matched frames compacted in frame order (the caller slices with info[0]; the rest is zero), info int32 [3] =
    (matched, empty frames, frames without a comparable distance)).  Device tensors, no synchronisation."""
    _hip.need_gpu(gt, det, offsets)
    if gt.dim() != 2 or gt.shape[1] < 6 or det.dim() != 2 or det.shape[1] < 6:
        raise RuntimeError("fit_nearest: states are [n, >= 6], got %s and %s" % (tuple(gt.shape), tuple(det.shape)))
    B, D = gt.shape[0], det.shape[0]
    if offsets.dim() != 1 or offsets.shape[0] != B + 1:
        raise RuntimeError("fit_nearest: %d offsets for %d frames (B + 1 expected)" % (offsets.numel(), B))
    if B > FIT_MAX or D > FIT_MAX:
        raise RuntimeError("fit_nearest takes at most %d frames and detections, got %d and %d" % (FIT_MAX, B, D))
    dev = gt.device
    gt, det = _state6(gt), _state6(det)
    off = offsets.to(torch.int32).contiguous()
    rows = torch.full((B,), -1, dtype=torch.int32, device=dev)
    resid = torch.zeros((B, 5), dtype=torch.float32, device=dev)
    info = torch.zeros(3, dtype=torch.int32, device=dev)
    if B:
        _hip.call("rn_fit_nearest", gt, det, off, B, D, rows, resid, info, device=dev)
    return rows, resid, info


def residual_moments(E, group=None, groups=None):
    """Mean and population covariance of residual rows (fit_filter_3D.py:292-299 and its three repeats) on the device,
    see include/retinanet_mi355x.h.  E [N,k] fp32, k <= 8.  Without ``group``: -> (mean [k], cov [k,k], count int32 [1]).
    With ``group`` [N] integer ids in [0, groups), groups <= 16: -> (mean [G,k], cov [G,k,k], count int32 [G]); a group
    without rows has count 0 and zeros.  fp64 sums in a fixed order, rounded once: two runs give the same bits."""
    _hip.need_gpu(E, group)
    if E.dim() != 2 or not 1 <= E.shape[1] <= MOMENTS_MAX_K:
        raise RuntimeError("residual_moments: E is [N, k] with 1 <= k <= %d, got %s" % (MOMENTS_MAX_K, tuple(E.shape)))
    N, k = E.shape
    if group is None:
        if groups not in (None, 1):
            raise RuntimeError("residual_moments: groups = %r without group ids" % (groups,))
        G = 1
    else:
        G = int(groups) if groups is not None else 0
        if not 1 <= G <= MOMENTS_MAX_G or group.dim() != 1 or group.shape[0] != N:
            raise RuntimeError("residual_moments: one group id per row and 1 <= groups <= %d, got %s ids for %d rows, groups = %r"
                               % (MOMENTS_MAX_G, tuple(group.shape), N, groups))
        group = group.to(torch.int32).contiguous()
    dev = E.device
    E = _hip.f32c(E)
    mean = torch.empty((G, k), dtype=torch.float32, device=dev)
    cov = torch.empty((G, k, k), dtype=torch.float32, device=dev)
    count = torch.empty(G, dtype=torch.int32, device=dev)
    _hip.call("rn_residual_moments", E, N, k, group, G, mean, cov, count, device=dev)
    if group is None:
        return mean[0], cov[0], count
    return mean, cov, count


# ------------------------------------------------------------------------------------------------ detector validation (mAP)
EVAL_MAX_DET = 4096                # RN_EVAL_MAX_DET: max_detections per image
EVAL_MAX_ROWS = 1 << 24            # RN_EVAL_MAX_ROWS: rows of the dataset's detection table
EVAL_MAX_CLASSES = 256             # RN_EVAL_MAX_CLASSES
EVAL_SORT_TILE, EVAL_SORT_SPAN = 64, 2048      # RN_EVAL_SORT_TILE / _SPAN: rows per sort step / per workgroup
EVAL_OK, EVAL_TOO_MANY, EVAL_BAD_LABEL, EVAL_TABLE_FULL = 0, 1, 2, 4       # bits of state[1]
EVAL_ROW_WORDS = 8                 # x1 y1 x2 y2 score (fp32 bits) | label image index (int32)


_EVAL_BITS = ((EVAL_TOO_MANY, "an image with more than %d detections" % EVAL_MAX_K),
              (EVAL_BAD_LABEL, "a selected detection whose label is outside [0, num_classes)"),
              (EVAL_TABLE_FULL, "the detection table is full"))


def eval_status_text(status):
    return _bits_text(_EVAL_BITS, status) or "ok"


def eval_table(rows, num_images, device):
    """-> (table int32 [rows, 8] -- the 32-byte rows of include/retinanet_mi355x.h, the float columns as their bits --,
    img_rows int32 [num_images, 2] zeroed, state int32 [2] = (cursor, status) zeroed)."""
    if not 0 <= rows <= EVAL_MAX_ROWS:
        raise RuntimeError("the detection table takes at most %d rows, got %d" % (EVAL_MAX_ROWS, rows))
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the detection table lives on the MI355X (no CPU fallback); got device %s" % device)
    return (torch.zeros((rows, EVAL_ROW_WORDS), dtype=torch.int32, device=device),
            torch.zeros((num_images, 2), dtype=torch.int32, device=device), torch.zeros(2, dtype=torch.int32, device=device))


def eval_box_cols(boxes, box_cols=None):
    """(first, one past last) column of the 2D box: (0, 4) for [K,4] boxes, (16, 20) -- the 2D envelope the model's own
    NMS uses -- for the directional model's [K,20] rows."""
    if box_cols is None:
        if boxes.dim() != 2 or boxes.shape[1] not in (4, 20):
            raise RuntimeError("eval_select: give box_cols for boxes of shape %s" % (tuple(boxes.shape),))
        box_cols = (0, 4) if boxes.shape[1] == 4 else (16, 20)
    c0, c1 = int(box_cols[0]), int(box_cols[1])
    if c1 - c0 != 4 or c0 < 0 or (boxes.numel() and (boxes.dim() != 2 or c1 > boxes.shape[1])):
        raise RuntimeError("eval_select: box_cols %r does not name four columns of boxes %s" % (box_cols, tuple(boxes.shape)))
    return c0, c1


def eval_select(scores, labels, boxes, table, img_rows, state, image, num_classes, score_threshold=0.05, max_detections=100,
                box_cols=None):
    """_get_detections' selection for ONE image (csv_eval.py:102-123) appended to the dataset's table: score >
    float32(score_threshold), score descending (ties: lower index first), the first max_detections.  table / img_rows /
    state from eval_table, updated in place; calls for different images are ordered by the stream.  Failures are bits in
    state[1] (EVAL_*), and the image then appends nothing.  No synchronisation."""
    _hip.need_gpu(scores, labels, boxes, table, img_rows, state)
    K = scores.shape[0]
    if scores.dim() != 1 or labels.shape != scores.shape or (K and boxes.shape[0] != K):
        raise RuntimeError("eval_select: scores [K], labels [K], boxes [K, n], got %s %s %s"
                           % (tuple(scores.shape), tuple(labels.shape), tuple(boxes.shape)))
    if not 0 <= int(max_detections) <= EVAL_MAX_DET:
        raise RuntimeError("eval_select: max_detections is at most %d, got %d" % (EVAL_MAX_DET, max_detections))
    if not 0 < int(num_classes) <= EVAL_MAX_CLASSES or not 0 <= int(image) < img_rows.shape[0]:
        raise RuntimeError("eval_select: image %d of %d, %d classes (at most %d)" % (image, img_rows.shape[0], num_classes, EVAL_MAX_CLASSES))
    _eval_check_table(table, state)
    c0 = 0
    if K:
        c0, _ = eval_box_cols(boxes, box_cols)
        scores, boxes = _hip.f32c(scores), _hip.f32c(boxes)
        labels = labels.long().contiguous()
    # without detections the boxes may have any shape and any number of rows: the entry point is handed NULL for them
    _hip.call("rn_eval_select", scores, labels, boxes if K else None, boxes.shape[1] if K else 4, c0, K, float(score_threshold),
              int(max_detections), int(image), img_rows.shape[0], int(num_classes), table, table.shape[0], state, img_rows,
              device=table.device)


def _eval_check_table(table, state):
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != EVAL_ROW_WORDS or not table.is_contiguous() or \
            state.dtype != torch.int32 or state.numel() != 2 or not state.is_contiguous() or table.shape[0] > EVAL_MAX_ROWS:
        raise RuntimeError("the detection table is a contiguous int32 [rows <= %d, %d] tensor with an int32 [2] state (ops.eval_table)"
                           % (EVAL_MAX_ROWS, EVAL_ROW_WORDS))


def eval_match(table, img_rows, ann_box, ann_offsets, num_classes, iou_threshold=0.5, num_annotations=None):
    """The greedy matching of evaluate (csv_eval.py:189-213).  ann_box [M,4] fp64 and ann_offsets int32
    [num_images * num_classes + 1] in (image, class) order.  -> (tp uint8 [rows]: 1 true positive / 0 false positive per
    table row, num_annotations int32 [num_classes] (written into the tensor given, if one is)).  No synchronisation."""
    _hip.need_gpu(table, img_rows, ann_box, ann_offsets, num_annotations)
    I, C, M = img_rows.shape[0], int(num_classes), ann_box.shape[0]
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != EVAL_ROW_WORDS or not table.is_contiguous():
        raise RuntimeError("eval_match: the table comes from ops.eval_table")
    if ann_box.dtype != torch.float64 or (M and tuple(ann_box.shape) != (M, 4)) or ann_offsets.dtype != torch.int32 or \
            ann_offsets.numel() != I * C + 1 or not 0 < C <= EVAL_MAX_CLASSES:
        raise RuntimeError("eval_match: ann_box [M,4] float64, ann_offsets int32 [%d * %d + 1], got %s %s and %s %s"
                           % (I, C, ann_box.dtype, tuple(ann_box.shape), ann_offsets.dtype, tuple(ann_offsets.shape)))
    dev = table.device
    ann_box, ann_offsets, img_rows = ann_box.contiguous(), ann_offsets.contiguous(), img_rows.contiguous()
    if num_annotations is None:
        num_annotations = torch.zeros(C, dtype=torch.int32, device=dev)
    elif num_annotations.dtype != torch.int32 or num_annotations.numel() != C or not num_annotations.is_contiguous():
        raise RuntimeError("eval_match: num_annotations is a contiguous int32 [num_classes] tensor")
    rows = table.shape[0]
    tp = torch.zeros(rows, dtype=torch.uint8, device=dev)
    taken = torch.empty(M, dtype=torch.uint8, device=dev)
    _hip.call("rn_eval_match", table, rows, img_rows, I, C, ann_box, ann_offsets, M, float(iou_threshold), taken, tp,
              num_annotations, device=dev)
    return tp, num_annotations


def eval_ap(table, state, tp, num_annotations, ap=None):
    """Per-class average precision (csv_eval.py:216-235, _compute_ap :38-62).  -> (ap float64 [num_classes] (written into
    the tensor given, if one is), order int32 [rows]: the table rows sorted stably by (label, score descending); the first
    state[0] entries are valid, the rest -1).  Bit-identical from run to run.  No synchronisation."""
    lib = _hip.load()
    _hip.need_gpu(table, state, tp, num_annotations, ap)
    _eval_check_table(table, state)
    rows, C = table.shape[0], num_annotations.numel()
    if tp.dtype != torch.uint8 or tp.numel() != rows or not tp.is_contiguous() or num_annotations.dtype != torch.int32 or \
            not num_annotations.is_contiguous() or not 0 < C <= EVAL_MAX_CLASSES:
        raise RuntimeError("eval_ap: tp uint8 [rows] and num_annotations int32 [classes <= %d] as eval_match returns them" % EVAL_MAX_CLASSES)
    dev = table.device
    if ap is None:
        ap = torch.zeros(C, dtype=torch.float64, device=dev)
    elif ap.dtype != torch.float64 or ap.numel() != C or not ap.is_contiguous():
        raise RuntimeError("eval_ap: ap is a contiguous float64 [num_classes] tensor")
    order = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.rn_eval_ap_workspace_bytes(rows), dtype=torch.uint8, device=dev)
    # the workspace has a fixed head, so it is not empty for an empty table, where the entry point is handed NULL
    _hip.call("rn_eval_ap", table, rows, state, tp, num_annotations, C, ws if rows else None, ap, order, device=dev)
    return ap, order


# ------------------------------------------------------------------------------------------------ detector validation in 3D
EVAL_CUBOID_OVERLAPS = {"silhouette": 0, "base": 1, "top": 2}      # RN_EVAL_CUBOID_*: all 8 corners / corners 0..3 / corners 4..7
EVAL_CUBOID_MAX_VERTS = 16         # RN_EVAL_CUBOID_MAX_VERTS
EVAL_CUBOID_MAX_THRESHOLDS = 8     # RN_EVAL_CUBOID_MAX_THRESHOLDS
EVAL_CUBOID_TERMS = ("iou", "corner_px", "corner_rel", "corner_px_reversed")        # columns of eval_cuboid_errors' terms
EVAL_CUBOID_SUMS = ("tp", "iou", "corner_px", "corner_rel", "reversed")             # columns of its per-class sums


def _eval_cuboid_check(name, table, img_rows, ann_corners, ann_offsets, num_classes):
    I, C, M = img_rows.shape[0], int(num_classes), ann_corners.shape[0]
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != EVAL_ROW_WORDS or not table.is_contiguous():
        raise RuntimeError(name + ": the table comes from ops.eval_table")
    if ann_corners.dtype != torch.float64 or (M and tuple(ann_corners.shape) != (M, 16)) or ann_offsets.dtype != torch.int32 or \
            ann_offsets.numel() != I * C + 1 or not 0 < C <= EVAL_MAX_CLASSES or not ann_corners.is_contiguous() or \
            not ann_offsets.is_contiguous() or not img_rows.is_contiguous() or img_rows.dtype != torch.int32:
        raise RuntimeError("%s: contiguous ann_corners [M,16] float64, ann_offsets int32 [%d * %d + 1], got %s %s and %s %s"
                           % (name, I, C, ann_corners.dtype, tuple(ann_corners.shape), ann_offsets.dtype, tuple(ann_offsets.shape)))
    return I, C, M


def _eval_cuboid_rows(name, rows, **tensors):
    """Every tensor is contiguous, of the dtype given and has `rows` leading entries."""
    for what, (t, dtype, shape) in tensors.items():
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError("%s: %s is a contiguous %s %s tensor, got %s %s" % (name, what, dtype, list(shape), t.dtype, tuple(t.shape)))


def eval_corners(boxes, table, img_rows, image, corners):
    """The 16 corner coordinates (columns 0:16 of the directional model's boxes [K, >=16]) of the rows eval_select has just
    appended for `image`, into corners float32 [rows, 16] in place, at the rows' positions.  Same stream as eval_select.
    No synchronisation."""
    _hip.need_gpu(boxes, table, img_rows, corners)
    rows, K = table.shape[0], boxes.shape[0]
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != EVAL_ROW_WORDS or not table.is_contiguous():
        raise RuntimeError("eval_corners: the table comes from ops.eval_table")
    if K and (boxes.dim() != 2 or boxes.shape[1] < 16):
        raise RuntimeError("eval_corners: boxes [K, >=16] with the corners in columns 0:16, got %s" % (tuple(boxes.shape),))
    if K > EVAL_MAX_K or not 0 <= int(image) < img_rows.shape[0]:
        raise RuntimeError("eval_corners: image %d of %d, %d detections (at most %d)" % (image, img_rows.shape[0], K, EVAL_MAX_K))
    _eval_cuboid_rows("eval_corners", rows, corners=(corners, torch.float32, (rows, 16)))
    if K:
        boxes = _hip.f32c(boxes)
    _hip.call("rn_eval_corners", boxes, boxes.shape[1] if K else 16, K, int(image), img_rows.shape[0], img_rows, table, rows, corners,
              device=table.device)


def eval_cuboid_overlap(table, img_rows, corners, ann_corners, ann_offsets, num_classes, overlap="silhouette"):
    """Per table row the first maximum, over all annotations of its (image, class) group, of the IoU of the convex hulls of
    the chosen corners (overlap: "silhouette" all 8, "base" 0..3, "top" 4..7; exact clipping in fp64).  ann_corners [M,16]
    fp64, ann_offsets int32 [num_images * num_classes + 1] in (image, class) order.  -> (best_iou float64 [rows], best_ann
    int32 [rows]: the index inside the group, -1 with 0.0 for a group without annotations).  No synchronisation."""
    _hip.need_gpu(table, img_rows, corners, ann_corners, ann_offsets)
    if overlap not in EVAL_CUBOID_OVERLAPS:
        raise RuntimeError("eval_cuboid_overlap: overlap is one of %s, got %r" % (sorted(EVAL_CUBOID_OVERLAPS), overlap))
    I, C, M = _eval_cuboid_check("eval_cuboid_overlap", table, img_rows, ann_corners, ann_offsets, num_classes)
    rows, dev = table.shape[0], table.device
    _eval_cuboid_rows("eval_cuboid_overlap", rows, corners=(corners, torch.float32, (rows, 16)))
    best_iou = torch.zeros(rows, dtype=torch.float64, device=dev)
    best_ann = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    _hip.call("rn_eval_cuboid_overlap", table, rows, img_rows, I, C, corners, ann_corners, ann_offsets, M,
              EVAL_CUBOID_OVERLAPS[overlap], best_iou, best_ann, device=dev)
    return best_iou, best_ann


def eval_cuboid_assign(table, img_rows, best_iou, best_ann, ann_offsets, num_annotated, num_classes, thresholds,
                       num_annotations=None):
    """The serial walk of csv_eval.py:189-213 per (image, class, threshold) on eval_cuboid_overlap's candidates: a row is a
    true positive at t iff best_iou >= t and its candidate is not yet taken at t.  thresholds: 1..8 floats, or a float64
    device tensor; num_annotated = M, the number of packed annotations.  -> (tp uint8 [T, rows], num_annotations int32
    [num_classes] (written into the tensor given, if one is), matched int32 [rows]: the annotation of the true positives at
    thresholds[0], else -1).  No synchronisation."""
    _hip.need_gpu(table, img_rows, best_iou, best_ann, ann_offsets, num_annotations)
    dev, rows, I, C, M = table.device, table.shape[0], img_rows.shape[0], int(num_classes), int(num_annotated)
    if not torch.is_tensor(thresholds):
        thresholds = torch.tensor([float(t) for t in thresholds], dtype=torch.float64, device=dev)
    T = thresholds.numel()
    if thresholds.dtype != torch.float64 or not thresholds.is_cuda or not thresholds.is_contiguous() or \
            not 1 <= T <= EVAL_CUBOID_MAX_THRESHOLDS:
        raise RuntimeError("eval_cuboid_assign: 1 to %d float64 thresholds, got %s %s"
                           % (EVAL_CUBOID_MAX_THRESHOLDS, thresholds.dtype, tuple(thresholds.shape)))
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != EVAL_ROW_WORDS or not table.is_contiguous():
        raise RuntimeError("eval_cuboid_assign: the table comes from ops.eval_table")
    if ann_offsets.dtype != torch.int32 or ann_offsets.numel() != I * C + 1 or not ann_offsets.is_contiguous() or \
            not 0 < C <= EVAL_MAX_CLASSES or M < 0 or img_rows.dtype != torch.int32 or not img_rows.is_contiguous():
        raise RuntimeError("eval_cuboid_assign: ann_offsets int32 [%d * %d + 1], got %s %s" % (I, C, ann_offsets.dtype, tuple(ann_offsets.shape)))
    _eval_cuboid_rows("eval_cuboid_assign", rows, best_iou=(best_iou, torch.float64, (rows,)), best_ann=(best_ann, torch.int32, (rows,)))
    if num_annotations is None:
        num_annotations = torch.zeros(C, dtype=torch.int32, device=dev)
    elif num_annotations.dtype != torch.int32 or num_annotations.numel() != C or not num_annotations.is_contiguous():
        raise RuntimeError("eval_cuboid_assign: num_annotations is a contiguous int32 [num_classes] tensor")
    tp = torch.zeros((T, rows), dtype=torch.uint8, device=dev)
    matched = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    taken = torch.empty(M * T, dtype=torch.uint8, device=dev)
    _hip.call("rn_eval_cuboid_assign", table, rows, img_rows, I, C, ann_offsets, M, best_iou, best_ann, thresholds, T, taken, tp,
              num_annotations, matched, device=dev)
    return tp, num_annotations, matched


def eval_cuboid_errors(table, state, img_rows, corners, ann_corners, ann_offsets, num_classes, tp, matched, best_iou, sums=None):
    """The error figures of the true positives at thresholds[0] (tp: that threshold's flags, uint8 [rows]).  -> (terms
    float64 [rows, 4]: EVAL_CUBOID_TERMS, zeros for every other row; sums float64 [num_classes, 5]: EVAL_CUBOID_SUMS per class,
    added in table order (written into the tensor given, if one is)).  Bit-identical from run to run.  No synchronisation."""
    _hip.need_gpu(table, state, img_rows, corners, ann_corners, ann_offsets, tp, matched, best_iou, sums)
    _eval_check_table(table, state)
    I, C, M = _eval_cuboid_check("eval_cuboid_errors", table, img_rows, ann_corners, ann_offsets, num_classes)
    rows, dev = table.shape[0], table.device
    _eval_cuboid_rows("eval_cuboid_errors", rows, corners=(corners, torch.float32, (rows, 16)), tp=(tp, torch.uint8, (rows,)),
                      matched=(matched, torch.int32, (rows,)), best_iou=(best_iou, torch.float64, (rows,)))
    if sums is None:
        sums = torch.zeros((C, 5), dtype=torch.float64, device=dev)
    elif sums.dtype != torch.float64 or sums.numel() != 5 * C or not sums.is_contiguous():
        raise RuntimeError("eval_cuboid_errors: sums is a contiguous float64 [num_classes, 5] tensor")
    terms = torch.zeros((rows, 4), dtype=torch.float64, device=dev)
    _hip.call("rn_eval_cuboid_errors", table, rows, state, I, C, corners, ann_corners, ann_offsets, M, tp, matched, best_iou, terms,
              sums, device=dev)
    return terms, sums


# ------------------------------------------------------------------------------------------------ frame ingest
IMAGENET_MEAN = (0.485, 0.456, 0.406)     # util_track/mp_loader.py:241
IMAGENET_STD = (0.229, 0.224, 0.225)
AUGMENT_PARAMS_BYTES = 104                # sizeof(rn_augment_params)
AUGMENT_TAPS = 7                          # RN_AUG_TAPS


def frame_ingest(frames_u8, swap_rb=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, nhwc4=False):
    """F.to_tensor + F.normalize of the reference's loaders on device (include/retinanet_mi355x.h, rn_frame_ingest).
    frames_u8: uint8 [B,H,W,3] (or [H,W,3]) -> float32 [B,3,H,W], or [B,H,W,4] with nhwc4=True."""
    _hip.need_gpu(frames_u8)
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8.unsqueeze(0)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise RuntimeError("frame_ingest takes uint8 [B,H,W,3] frames, got %s %s" % (frames_u8.dtype, tuple(frames_u8.shape)))
    f = frames_u8.contiguous()
    B, H, W, _ = f.shape
    out = torch.empty((B, H, W, 4) if nhwc4 else (B, 3, H, W), dtype=torch.float32, device=f.device)
    _hip.call("rn_frame_ingest", f, B, H, W, int(bool(swap_rb)), *[float(m) for m in mean], *[float(s) for s in std],
              int(bool(nhwc4)), out, device=f.device)
    return out


# ------------------------------------------------------------------------------------------------ 4K frames
TS_MAX_SETS, TS_MAX_CELLS, TS_MAX_KEYS, TS_ROW, TS_MAX_CELL_PIXELS = 4, 16, 64, 8, 4096     # RN_TS_* of the header
TS_READ, TS_FAILED, TS_FELL_BACK = 0, 1, 2
TS_GEOMETRY_KEYS = ("x0", "y0", "w", "h", "n", "h13", "h23", "w12")


def _u8_frames(frames_u8, what):
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8.unsqueeze(0)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise RuntimeError("%s takes uint8 [B,H,W,3] frames, got %s %s" % (what, frames_u8.dtype, tuple(frames_u8.shape)))
    return frames_u8


def frame_ingest_half(frames_u8, swap_rb=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, nhwc4=False, keep_u8=False):
    """The loader's 2x reduction + to_tensor + normalize in one pass (include/retinanet_mi355x.h, rn_frame_ingest_half;
    util_track/mp_loader.py:237-243).  frames_u8: uint8 [B,2H,2W,3] (or [2H,2W,3]) -> float32 [B,3,H,W], or [B,H,W,4] with
    nhwc4=True: ``frame_ingest`` of the reduced frame, bit for bit.  keep_u8=True -> (tensor, reduced uint8 [B,H,W,3])."""
    _hip.need_gpu(frames_u8)
    f = _u8_frames(frames_u8, "frame_ingest_half")
    B, H2, W2, _ = f.shape
    if B < 1 or H2 < 2 or W2 < 2 or H2 % 2 or W2 % 2:
        raise RuntimeError("frame_ingest_half halves exactly: it takes even, non-empty frame sizes, got %s" % (tuple(f.shape),))
    f = f.contiguous()
    H, W = H2 // 2, W2 // 2
    out = torch.empty((B, H, W, 4) if nhwc4 else (B, 3, H, W), dtype=torch.float32, device=f.device)
    u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=f.device) if keep_u8 else None
    _hip.call("rn_frame_ingest_half", f, B, H2, W2, int(bool(swap_rb)), *[float(m) for m in mean], *[float(s) for s in std],
              int(bool(nhwc4)), out, u8, device=f.device)
    return (out, u8) if keep_u8 else out


def pack_timestamp_sets(sets):
    """Host side of ``parse_frame_timestamps``: sets = a sequence of up to 4 (geometry, checksums) pairs -- geometry a mapping
    with x0, y0, w, h, n, h13, h23, w12 (the reference's h12 is read there and never used); checksums a mapping key -> six
    counts (3x2, band major) in the order the reference's ``min`` walks it.  -> (int32 [G,9] geometry rows with K appended,
    int32 [G,64,8] table rows: the six counts, then the key's digit).  ValueError for a key whose ``str()`` is not one decimal
    digit (the fp64 value needs digits) and for sizes the kernel refuses."""
    sets = list(sets)
    if not 1 <= len(sets) <= TS_MAX_SETS:
        raise ValueError("between 1 and %d (geometry, checksums) sets, got %d" % (TS_MAX_SETS, len(sets)))
    geo = np.zeros((len(sets), 9), np.int32)
    tab = np.zeros((len(sets), TS_MAX_KEYS, TS_ROW), np.int32)
    for g, (geom, table) in enumerate(sets):
        x0, y0, w, h, n, h13, h23, w12 = (int(geom[k]) for k in TS_GEOMETRY_KEYS)
        K = len(table)
        if not 1 <= n <= TS_MAX_CELLS or not 1 <= K <= TS_MAX_KEYS:
            raise ValueError("set %d: n = %d cells (1..%d), %d table entries (1..%d)" % (g, n, TS_MAX_CELLS, K, TS_MAX_KEYS))
        if x0 < 0 or y0 < 0 or w < 1 or h < 1 or w * h > TS_MAX_CELL_PIXELS or not 0 <= h13 <= h23 <= h or not 0 <= w12 <= w:
            raise ValueError("set %d: geometry %r is refused (x0, y0 >= 0; 0 <= h13 <= h23 <= h; 0 <= w12 <= w; 1 <= w * h <= %d)"
                             % (g, dict((k, int(geom[k])) for k in TS_GEOMETRY_KEYS), TS_MAX_CELL_PIXELS))
        geo[g] = (x0, y0, w, h, n, h13, h23, w12, K)
        for k, (key, cs) in enumerate(table.items()):
            text = str(key)
            if len(text) != 1 or text not in "0123456789":
                raise ValueError("set %d: table key %r does not read as one decimal digit" % (g, key))
            tab[g, k, :6] = np.asarray(cs, np.int64).reshape(6)
            tab[g, k, 6] = int(text)
    return geo, tab


def parse_frame_timestamps(frames_u8, sets, prev=None, swap_rb=False, want_mask=False):
    """timestamp_utilities.parse_frame_timestamp for B frames and up to 4 sets tried in order, on device
    (include/retinanet_mi355x.h, rn_parse_frame_timestamps).  frames_u8: uint8 [B,H,W,3] on the device, any strides as long
    as a pixel's three bytes are adjacent (a strip sliced from a frame is read in place); sets: (geometry, checksums) pairs,
    or what ``pack_timestamp_sets`` made of them with the table already on the device (geometry int32 [G,9] numpy, table
    int32 [G,64,8] device tensor); prev: optional fp64 [B] on the device.
    -> (times fp64 [B], status i32 [B] (TS_READ / TS_FAILED / TS_FELL_BACK), set index i32 [B], digits i8 [B,16],
        first failing cell of the first set i32 [B], the first set's mask uint8 [B,h,n*w] or None)."""
    _hip.need_gpu(frames_u8, prev)
    f = _u8_frames(frames_u8, "parse_frame_timestamps")
    if isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray) and torch.is_tensor(sets[1]):
        geo, tab = sets
        _hip.need_gpu(tab)
    else:
        geo, tab = pack_timestamp_sets(sets)
        tab = torch.from_numpy(tab).to(f.device)
    geo = np.ascontiguousarray(geo, np.int32)
    if tab.dtype != torch.int32 or tuple(tab.shape) != (geo.shape[0], TS_MAX_KEYS, TS_ROW) or not tab.is_contiguous():
        raise RuntimeError("parse_frame_timestamps: the table is int32 [G,%d,%d], contiguous" % (TS_MAX_KEYS, TS_ROW))
    B, H, W, _ = f.shape
    if B < 1 or H < 1 or W < 1:
        raise RuntimeError("parse_frame_timestamps: empty frames %s" % (tuple(f.shape),))
    if f.stride(3) != 1 or f.stride(2) != 3 or f.stride(1) < 3 * W or (B > 1 and f.stride(0) < (H - 1) * f.stride(1) + 3 * W):
        f = f.contiguous()
    if prev is not None:
        if prev.dtype != torch.float64 or tuple(prev.shape) != (B,):
            raise RuntimeError("parse_frame_timestamps: prev is float64 [B]")
        prev = prev.contiguous()
    dev = f.device
    times = torch.empty(B, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    set_index = torch.empty(B, dtype=torch.int32, device=dev)
    digits = torch.empty((B, TS_MAX_CELLS), dtype=torch.int8, device=dev)
    fail_cell = torch.empty(B, dtype=torch.int32, device=dev)
    mask = torch.empty((B, int(geo[0, 3]), int(geo[0, 4]) * int(geo[0, 2])), dtype=torch.uint8, device=dev) if want_mask else None
    _hip.call("rn_parse_frame_timestamps", f, B, H, W, f.stride(0) if B > 1 else 0, f.stride(1), int(bool(swap_rb)), geo.ctypes.data,
              geo.shape[0], tab, prev, times, status, set_index, digits, fail_cell, mask, device=dev)
    return times, status, set_index, digits, fail_cell, mask


def load_frames_4k(frames_u8, reader, swap_rb=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, nhwc4=False, keep_u8=False):
    """One tracker step's input from one upload (util_track/mp_loader.py:230-243 for every camera): the time stamps of the
    4K frames through ``reader`` (a ``timestamp_utilities.TimestampReader``: tables and the previous stamps on the device)
    and ``frame_ingest_half``, both on the current stream.  swap_rb concerns the detector's tensor only; the reader carries its
    own channel order.  -> (frames, timestamps fp64 [B], status i32 [B]); frames is (tensor, reduced uint8) with keep_u8."""
    _hip.need_gpu(frames_u8)
    timestamps, status = reader(frames_u8)
    frames = frame_ingest_half(frames_u8, swap_rb=swap_rb, mean=mean, std=std, nhwc4=nhwc4, keep_u8=keep_u8)
    return frames, timestamps, status


def augment_frames(frames_u8, params, noise=None, seed=0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The image chain of the reference's training loader on device (include/retinanet_mi355x.h, rn_augment_frames;
    corrected_3D_dataset.py:330-478).  frames_u8: uint8 [B,H,W,3]; params: (records, table_x, table_y) as
    ``augment.pack_params`` makes them -- numpy arrays (uploaded here) or device tensors (records as uint8 [B,104], tables
    int32 [B,W,8] and [B,H,8]); noise: optional uint8 [B,H,W,3] pad bytes, else the device generator keyed by ``seed``.
    -> float32 [B,3,H,W]."""
    lib = _hip.load()
    _hip.need_gpu(frames_u8, noise)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise RuntimeError("augment_frames takes uint8 [B,H,W,3] frames, got %s %s" % (frames_u8.dtype, tuple(frames_u8.shape)))
    f = frames_u8.contiguous()
    B, H, W, _ = f.shape
    rec, tx, ty = params
    if isinstance(rec, np.ndarray):
        rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)).to(f.device)
        tx, ty = torch.from_numpy(np.ascontiguousarray(tx)).to(f.device), torch.from_numpy(np.ascontiguousarray(ty)).to(f.device)
    _hip.need_gpu(rec, tx, ty)
    rec, tx, ty = rec.contiguous(), tx.contiguous(), ty.contiguous()
    if rec.dtype != torch.uint8 or tuple(rec.shape) != (B, AUGMENT_PARAMS_BYTES) or rec.data_ptr() % 8:
        raise RuntimeError("augment_frames: records must be 8-byte aligned uint8 [%d,%d], got %s %s"
                           % (B, AUGMENT_PARAMS_BYTES, rec.dtype, tuple(rec.shape)))
    if tx.dtype != torch.int32 or ty.dtype != torch.int32 or tuple(tx.shape) != (B, W, 1 + AUGMENT_TAPS) or \
            tuple(ty.shape) != (B, H, 1 + AUGMENT_TAPS):
        raise RuntimeError("augment_frames: tables must be int32 [%d,%d,%d] and [%d,%d,%d], got %s and %s"
                           % (B, W, 1 + AUGMENT_TAPS, B, H, 1 + AUGMENT_TAPS, tuple(tx.shape), tuple(ty.shape)))
    if noise is not None:
        if noise.dtype != torch.uint8 or tuple(noise.shape) != (B, H, W, 3):
            raise RuntimeError("augment_frames: noise must be uint8 %s, got %s %s" % ((B, H, W, 3), noise.dtype, tuple(noise.shape)))
        noise = noise.contiguous()
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=f.device)
    if B == 0:
        return out
    ws = torch.empty(int(lib.rn_augment_workspace_bytes(B, H, W)) // 8, dtype=torch.int64, device=f.device)
    _hip.call("rn_augment_frames", f, B, H, W, rec, tx, ty, noise, int(seed) & 0xFFFFFFFFFFFFFFFF, *[float(m) for m in mean],
              *[float(s) for s in std], ws, out, device=f.device)
    return out


AUGMENT_CROP_PARAMS_BYTES = 128           # sizeof(rn_augment_crop_params)
AUGMENT_CROP_WIN_LIMIT = 16384            # the largest window edge and crop size rn_augment_crops takes


def augment_crops(frames_u8, params, K, win_max, crop, noise=None, occlusion=None, seed=0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The crop mode of the reference's training loader on device (include/retinanet_mi355x.h, rn_augment_crops;
    corrected_3D_dataset.py:330-390, 501-594).  frames_u8: uint8 [B,H,W,3]; params: (records, table_x, table_y, table_cx,
    table_cy) as ``augment.pack_crop_params`` makes them -- numpy arrays (uploaded here) or device tensors (records as uint8
    [B,128], tables int32 [B,W,8], [B,H,8] and two [B,crop,1+K]); K: the taps of the second resize's tables, the batch's largest
    ceil(max(size / crop, 1)) * 2 + 1; win_max: at least the largest window edge of the batch;
    noise: optional uint8 [B,H,W,3] pad bytes; occlusion: optional float32 [B,3,crop,crop] values for the occluded regions; both
    come from the device generator keyed by ``seed`` otherwise.  -> float32 [B,3,crop,crop]."""
    lib = _hip.load()
    _hip.need_gpu(frames_u8, noise, occlusion)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise RuntimeError("augment_crops takes uint8 [B,H,W,3] frames, got %s %s" % (frames_u8.dtype, tuple(frames_u8.shape)))
    f = frames_u8.contiguous()
    B, H, W, _ = f.shape
    K, win_max, crop = int(K), int(win_max), int(crop)
    rec, tx, ty, cx, cy = params
    if not (0 < crop <= AUGMENT_CROP_WIN_LIMIT and 0 < win_max <= AUGMENT_CROP_WIN_LIMIT):
        raise RuntimeError("augment_crops: crop and win_max must lie in [1, %d], got %d and %d" % (AUGMENT_CROP_WIN_LIMIT, crop, win_max))
    if isinstance(rec, np.ndarray):
        rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)).to(f.device)
        tx, ty, cx, cy = (torch.from_numpy(np.ascontiguousarray(t)).to(f.device) for t in (tx, ty, cx, cy))
    _hip.need_gpu(rec, tx, ty, cx, cy)
    rec, tx, ty, cx, cy = rec.contiguous(), tx.contiguous(), ty.contiguous(), cx.contiguous(), cy.contiguous()
    if rec.dtype != torch.uint8 or tuple(rec.shape) != (B, AUGMENT_CROP_PARAMS_BYTES) or rec.data_ptr() % 8:
        raise RuntimeError("augment_crops: records must be 8-byte aligned uint8 [%d,%d], got %s %s"
                           % (B, AUGMENT_CROP_PARAMS_BYTES, rec.dtype, tuple(rec.shape)))
    if tx.dtype != torch.int32 or ty.dtype != torch.int32 or tuple(tx.shape) != (B, W, 1 + AUGMENT_TAPS) or \
            tuple(ty.shape) != (B, H, 1 + AUGMENT_TAPS):
        raise RuntimeError("augment_crops: the first resize's tables must be int32 [%d,%d,%d] and [%d,%d,%d], got %s and %s"
                           % (B, W, 1 + AUGMENT_TAPS, B, H, 1 + AUGMENT_TAPS, tuple(tx.shape), tuple(ty.shape)))
    if K < 3 or cx.dtype != torch.int32 or cy.dtype != torch.int32 or tuple(cx.shape) != (B, crop, 1 + K) or \
            tuple(cy.shape) != (B, crop, 1 + K):
        raise RuntimeError("augment_crops: the second resize's tables must both be int32 [%d,%d,%d] (K = %d >= 3), got %s %s and %s %s"
                           % (B, crop, 1 + K, K, cx.dtype, tuple(cx.shape), cy.dtype, tuple(cy.shape)))
    if noise is not None:
        if noise.dtype != torch.uint8 or tuple(noise.shape) != (B, H, W, 3):
            raise RuntimeError("augment_crops: noise must be uint8 %s, got %s %s" % ((B, H, W, 3), noise.dtype, tuple(noise.shape)))
        noise = noise.contiguous()
    if occlusion is not None:
        if occlusion.dtype != torch.float32 or tuple(occlusion.shape) != (B, 3, crop, crop):
            raise RuntimeError("augment_crops: occlusion must be float32 %s, got %s %s"
                               % ((B, 3, crop, crop), occlusion.dtype, tuple(occlusion.shape)))
        occlusion = occlusion.contiguous()
    out = torch.empty((B, 3, crop, crop), dtype=torch.float32, device=f.device)
    if B == 0:
        return out
    ws = torch.empty(int(lib.rn_augment_crops_workspace_bytes(B, win_max, crop)) // 8, dtype=torch.int64, device=f.device)
    _hip.call("rn_augment_crops", f, B, H, W, rec, tx, ty, cx, cy, K, win_max, crop, noise, occlusion,
              int(seed) & 0xFFFFFFFFFFFFFFFF, *[float(m) for m in mean], *[float(s) for s in std], ws, out, device=f.device)
    return out


# ------------------------------------------------------------------------------------------------ tracker: crop refinement
CROP_MAX_A, CROP_MAX_K = 4096, 256


def crop_boxes(im_objs, cam_idxs=None, b=1.25):
    """MC_Crop_Tracker.get_crop_boxes (MC3D_crop_tracker.py:920-944): im_objs [n,8,2] -> crop boxes [n,4] float64; with
    cam_idxs also the [n,5] float32 RoI rows (camera, box) that roi_align takes (:1183-1185)."""
    _hip.need_gpu(im_objs, cam_idxs)
    im = im_objs.double().contiguous()
    n = im.shape[0]
    boxes = torch.empty((n, 4), dtype=torch.float64, device=im.device)
    rois = None if cam_idxs is None else torch.empty((n, 5), dtype=torch.float32, device=im.device)
    cam = None if cam_idxs is None else cam_idxs.long().contiguous()
    if n:
        _hip.call("rn_crop_boxes", im, cam, n, float(b), boxes, rois, device=im.device)
    return boxes if rois is None else (boxes, rois)


def roi_align(frames, rois, output_size, nhwc4=False):
    """torchvision.ops.roi_align(frames, rois, output_size) with its defaults, on device.  frames [N,C,H,W] float32,
    rois [n,5] (batch index, x1, y1, x2, y2) -> [n,C,h,w], or [n,h,w,4] with nhwc4=True (C <= 4)."""
    _hip.need_gpu(frames, rois)
    f, r = _hip.f32c(frames), _hip.f32c(rois)
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    N, C, H, W = f.shape
    n = r.shape[0]
    out = torch.empty((n, oh, ow, 4) if nhwc4 else (n, C, oh, ow), dtype=torch.float32, device=f.device)
    if n:
        _hip.call("rn_roi_align", f, N, C, H, W, r, n, oh, ow, out, int(bool(nhwc4)), device=f.device)
    return out


def crop_select(reg_boxes, cls, crop_bx, cam_idxs, pre_loc, H1, H2, P1, P2, cs=112, cd_max=50, W=0.5):
    """Everything after the LOCALIZE detector in the tracker's crop path (MC3D_crop_tracker.py:1192-1226), one
    workgroup per object: -> (state [n,6] f32, class [n] i64, confidence [n] f32)."""
    _hip.need_gpu(reg_boxes, cls, crop_bx, cam_idxs, pre_loc, H1, H2, P1, P2)
    n, A, C = cls.shape
    if A > CROP_MAX_A or cd_max > CROP_MAX_K:
        raise RuntimeError("crop_select sorts a crop's anchors in LDS: at most %d anchors and cd_max %d, got %d / %d"
                           % (CROP_MAX_A, CROP_MAX_K, A, cd_max))
    if reg_boxes.shape != (n, A, 20) or crop_bx.shape != (n, 4) or pre_loc.shape != (n, 6) or cam_idxs.shape[0] != n:
        raise RuntimeError("crop_select: reg %s cls %s crops %s priors %s do not line up"
                           % (tuple(reg_boxes.shape), tuple(cls.shape), tuple(crop_bx.shape), tuple(pre_loc.shape)))
    dev = cls.device
    reg_boxes, cls, pre_loc = _hip.f32c(reg_boxes), _hip.f32c(cls), _hip.f32c(pre_loc)
    crop_bx, cam = crop_bx.double().contiguous(), cam_idxs.long().contiguous()
    st = torch.empty((n, 6), dtype=torch.float32, device=dev)
    oc = torch.empty(n, dtype=torch.int64, device=dev)
    of = torch.empty(n, dtype=torch.float32, device=dev)
    if n:
        _hip.call("rn_crop_select", reg_boxes, cls, crop_bx, cam, pre_loc, H1, H2, P1, P2, H1.shape[0], n, A, C, float(cs),
                  int(cd_max), float(W), st, oc, of, device=dev)
    return st, oc, of


# ------------------------------------------------------------------------------------------------ camera calibration
VP_LEVELS = 16
VP_FEW_LINES, VP_BAD_START, VP_LONG_AXIS, VP_BAD_OFFSETS = 1, 2, 4, 8
SZ_MAX_ITERS = 64
SZ_BAD_FIRST_STEP, SZ_NO_WINNER, SZ_TOO_MANY = 1, 2, 4
FIT_FEW_POINTS, FIT_DEGENERATE, FIT_NOT_FINITE, FIT_BAD_OFFSETS = 1, 2, 4, 8


def _csr(offsets, what):
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise RuntimeError("%s: offsets are int64 [sets + 1], got %s %s" % (what, offsets.dtype, tuple(offsets.shape)))
    return offsets.contiguous()


def vanishing_points(lines, offsets):
    """find_vanishing_point (homography.py:96-154) of every line set in one launch, see include/retinanet_mi355x.h.
    lines fp64 [N,4], offsets int64 [S+1] (CSR row ranges; a range outside the N rows sets the VP_BAD_OFFSETS bit) ->
    (out fp64 [S,3] = (px, py, best distance), trace fp64 [S,16,3], status int32 [S]); nothing is synchronised."""
    _hip.need_gpu(lines, offsets)
    if lines.dim() != 2 or lines.shape[1] != 4 or lines.dtype != torch.float64:
        raise RuntimeError("vanishing_points: lines are fp64 [N,4] (x0, y0, x1, y1), got %s %s" % (lines.dtype, tuple(lines.shape)))
    offsets = _csr(offsets, "vanishing_points")
    lines = lines.contiguous()
    S = offsets.shape[0] - 1
    dev = lines.device
    out = torch.empty((S, 3), dtype=torch.float64, device=dev)
    trace = torch.zeros((S, VP_LEVELS, 3), dtype=torch.float64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    _hip.call("rn_vanishing_points", lines, lines.shape[0], offsets, S, out, trace, status, device=dev)
    return out, trace, status


def _calib_inputs(boxes, heights, H, P, what):
    if boxes.dim() != 3 or boxes.shape[1:] != (8, 2) or boxes.shape[0] == 0:
        raise RuntimeError("%s: boxes are [d,8,2] image corners with d >= 1, got %s" % (what, tuple(boxes.shape)))
    if heights.dim() != 1 or heights.shape[0] != boxes.shape[0]:
        raise RuntimeError("%s: one height per box, got %s for %d boxes" % (what, tuple(heights.shape), boxes.shape[0]))
    if tuple(H.shape) != (3, 3) or tuple(P.shape) != (3, 4) or H.dtype != torch.float64 or P.dtype != torch.float64:
        raise RuntimeError("%s: H is fp64 [3,3] and P fp64 [3,4], got %s and %s" % (what, tuple(H.shape), tuple(P.shape)))
    return boxes.double().contiguous(), _hip.f32c(heights), H.contiguous(), P.contiguous()


def hg_reproj_error(boxes, heights, H, P_orig, C):
    """test_transformation's arithmetic (homography.py:581-587) for every scale C [K] of P_orig's third column ->
    fp64 [K,2] = (top, bottom) mean corner distance in pixels."""
    _hip.need_gpu(boxes, heights, H, P_orig, C)
    boxes, heights, H, P_orig = _calib_inputs(boxes, heights, H, P_orig, "hg_reproj_error")
    if C.dim() != 1 or C.shape[0] == 0 or C.dtype != torch.float64:
        raise RuntimeError("hg_reproj_error: C is fp64 [K] with K >= 1, got %s %s" % (C.dtype, tuple(C.shape)))
    C = C.contiguous()
    out = torch.empty((C.shape[0], 2), dtype=torch.float64, device=boxes.device)
    _hip.call("rn_hg_reproj_error", boxes, heights, H, P_orig, C, boxes.shape[0], C.shape[0], out, device=boxes.device)
    return out


def hg_scale_z(boxes, heights, H, P_orig, granularity=1e-06, max_scale=10.0):
    """The search of scale_Z (homography.py:607-666) in one launch -> (trace fp64 [SZ_MAX_ITERS,10,2] = (C, error), zero
    beyond the iterations run (the search shrinks its step 4.5 x per iteration: 10 iterations at the defaults); out fp64 [3] = (last C evaluated, best C, best error of the last iteration);
    info int32 [2] = (iterations, status bits))."""
    _hip.need_gpu(boxes, heights, H, P_orig)
    boxes, heights, H, P_orig = _calib_inputs(boxes, heights, H, P_orig, "hg_scale_z")
    dev = boxes.device
    trace = torch.zeros((SZ_MAX_ITERS, 10, 2), dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    _hip.call("rn_hg_scale_z", boxes, heights, H, P_orig, boxes.shape[0], float(granularity), float(max_scale), SZ_MAX_ITERS, trace,
              out, info, device=dev)
    return trace, out, info


def fit_homography(src, dst, offsets, refine=True):
    """Plane homographies dst ~ H [src; 1], one per CSR row range: src, dst fp64 [N,2], offsets int64 [B+1] ->
    (H fp64 [B,3,3] with H[2,2] = 1, NaN where the status is not 0; status int32 [B]).  Stands in for
    cv2.findHomography(src, dst) at its default method; parity with OpenCV is unpinned (include/retinanet_mi355x.h)."""
    _hip.need_gpu(src, dst, offsets)
    if src.dim() != 2 or src.shape[1] != 2 or src.shape != dst.shape or src.dtype != torch.float64 or dst.dtype != torch.float64:
        raise RuntimeError("fit_homography: src and dst are fp64 [N,2], got %s and %s" % (tuple(src.shape), tuple(dst.shape)))
    offsets = _csr(offsets, "fit_homography")
    src, dst = src.contiguous(), dst.contiguous()
    B = offsets.shape[0] - 1
    H = torch.empty((B, 3, 3), dtype=torch.float64, device=src.device)
    status = torch.empty(B, dtype=torch.int32, device=src.device)
    _hip.call("rn_fit_homography", src, dst, src.shape[0], offsets, B, int(bool(refine)), H, status, device=src.device)
    return H, status


# ------------------------------------------------------------------------------------------------ output frames
RENDER_MAX_DIM = 16384             # RN_RENDER_MAX_DIM
RENDER_BITS = dict(prior=0, crop_edge=1, track=2, det=3, in_crop=4, label=5, label_text=6, banner_edge=7, banner_text=8)
RENDER_RECT_COLS = ("x0", "y0", "x1", "y1", "cam", "mode", "anchor", "bit")
RENDER_RUN_COLS = ("x", "y", "cam", "anchor", "scale", "dilate", "bit", "start", "length")


def render_mask(n_cam, H, W, device):
    """A cleared mask plane uint16 [n_cam,H,W] whose buffer reaches to a multiple of 4 bytes, as the painters' two-pixel
    atomics need it (include/retinanet_mi355x.h)."""
    n = int(n_cam) * int(H) * int(W)
    return torch.zeros(n + (n & 1), dtype=torch.uint16, device=device)[:n].view(int(n_cam), int(H), int(W))


def _render_plane(what, mask):
    if mask.dtype != torch.uint16 or mask.dim() != 3 or not mask.is_contiguous() or min(mask.shape) < 1 \
            or max(mask.shape[1:]) > RENDER_MAX_DIM:
        raise RuntimeError("%s: mask is a contiguous uint16 [n_cam,H,W] plane (H, W <= %d), got %s %s"
                           % (what, RENDER_MAX_DIM, mask.dtype, tuple(mask.shape)))
    room = mask.untyped_storage().nbytes() - 2 * mask.storage_offset()
    if mask.data_ptr() % 4 or room < (2 * mask.numel() + 3) // 4 * 4:
        raise RuntimeError("%s: the mask's buffer must be 4-byte aligned and reach to a multiple of 4 bytes: allocate it with "
                           "ops.render_mask" % what)
    return tuple(int(s) for s in mask.shape)


def _render_boxes(what, name, boxes, dev):
    if boxes is None:
        return 0
    _hip.need_gpu(boxes)
    if boxes.dtype != torch.float64 or boxes.dim() != 3 or tuple(boxes.shape[1:]) != (8, 2) or not boxes.is_contiguous() \
            or boxes.device != dev:
        raise RuntimeError("%s: %s is a contiguous fp64 [n,8,2] tensor on the mask's device, got %s %s"
                           % (what, name, boxes.dtype, tuple(boxes.shape)))
    return boxes.shape[0]


def render_edges(corners, cam, thickness, bit, mask):
    """ORs bit number `bit` into mask along the 14 edges of every box: corners fp64 [n,8,2], cam int32 [n] (rn_render_edges)."""
    _hip.need_gpu(corners, cam, mask)
    n_cam, H, W = _render_plane("render_edges", mask)
    n = _render_boxes("render_edges", "corners", corners, mask.device)
    _typed("render_edges", ("cam", cam, torch.int32))
    if tuple(cam.shape) != (n,) or cam.device != mask.device:
        raise RuntimeError("render_edges: cam is int32 [n] on the mask's device")
    if not (1 <= int(thickness) <= 255 and 0 <= int(bit) <= 15):
        raise RuntimeError("render_edges: 1 <= thickness <= 255 and 0 <= bit <= 15")
    _hip.call("rn_render_edges", corners, cam, n, int(thickness), int(bit), mask, n_cam, H, W, device=mask.device)
    return mask


def _render_records(what, name, rec, cols, dev):
    _hip.need_gpu(rec)
    if rec.dtype != torch.int32 or rec.dim() != 2 or rec.shape[1] != cols or not rec.is_contiguous() or rec.device != dev:
        raise RuntimeError("%s: %s is a contiguous int32 [n,%d] tensor on the mask's device, got %s %s"
                           % (what, name, cols, rec.dtype, tuple(rec.shape)))
    return rec.shape[0]


def render_rects(rects, mask, anchors=None):
    """rects int32 [n,8] (RENDER_RECT_COLS): half-open rectangles, filled (mode 0) or outlined (1), absolute or offset from
    (int(min x), int(max y)) of box `anchor` of anchors fp64 [m,8,2] (rn_render_rects)."""
    _hip.need_gpu(mask)
    n_cam, H, W = _render_plane("render_rects", mask)
    n = _render_records("render_rects", "rects", rects, len(RENDER_RECT_COLS), mask.device)
    m = _render_boxes("render_rects", "anchors", anchors, mask.device)
    _hip.call("rn_render_rects", rects, n, anchors, m, mask, n_cam, H, W, device=mask.device)
    return mask


def render_text(runs, text, font, mask, anchors=None):
    """runs int32 [n,9] (RENDER_RUN_COLS) over the bytes of text uint8 [T]; font uint8 [95,8] (rn_render_text)."""
    _hip.need_gpu(text, font, mask)
    n_cam, H, W = _render_plane("render_text", mask)
    n = _render_records("render_text", "runs", runs, len(RENDER_RUN_COLS), mask.device)
    m = _render_boxes("render_text", "anchors", anchors, mask.device)
    _typed("render_text", ("text", text, torch.uint8), ("font", font, torch.uint8))
    if text.dim() != 1 or tuple(font.shape) != (95, 8) or text.device != mask.device or font.device != mask.device:
        raise RuntimeError("render_text: text is uint8 [T] and font uint8 [95,8], both on the mask's device")
    _hip.call("rn_render_text", runs, n, text, text.numel(), font, anchors, m, mask, n_cam, H, W, device=mask.device)
    return mask


def render_compose(frames, mask, crops_present, cols, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """frames fp32 [n_cam,3,H,W] (normalised RGB) + mask uint16 [n_cam,H,W] -> the uint8 mosaic [R*H, cols*W, 3], camera i in
    tile (i // cols, i % cols), unused tiles zero (rn_render_compose)."""
    _hip.need_gpu(frames, mask, out)
    n_cam, H, W = _render_plane("render_compose", mask)
    if frames.dtype != torch.float32 or tuple(frames.shape) != (n_cam, 3, H, W) or not frames.is_contiguous() \
            or frames.device != mask.device:
        raise RuntimeError("render_compose: frames is a contiguous fp32 [%d,3,%d,%d] tensor on the mask's device, got %s %s"
                           % (n_cam, H, W, frames.dtype, tuple(frames.shape)))
    cols = int(cols)
    if not 1 <= cols <= n_cam:
        raise RuntimeError("render_compose: 1 <= cols <= n_cam")
    rows = -(-n_cam // cols)
    if out is None:
        out = torch.empty((rows * H, cols * W, 3), dtype=torch.uint8, device=mask.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (rows * H, cols * W, 3) or not out.is_contiguous() or out.device != mask.device:
        raise RuntimeError("render_compose: out is a contiguous uint8 [%d,%d,3] tensor on the mask's device" % (rows * H, cols * W))
    _hip.call("rn_render_compose", frames, *[float(m) for m in mean], *[float(s) for s in std], mask, int(bool(crops_present)), out,
              n_cam, H, W, cols, device=mask.device)
    return out


# ------------------------------------------------------------------------------------------------ tracking CSV replay
REPLAY_BITS = dict(primary=0, secondary=1, label=2, label_text=3)         # RN_REPLAY_* of the header, as bit numbers
REPLAY_MAX_CANVAS = 1 << 20        # RN_REPLAY_MAX_CANVAS
REPLAY_ABSDIFF_BLOCKS = 1024       # RN_REPLAY_ABSDIFF_BLOCKS


def replay_layout(n_cam):
    """(rows, cols) of the replay's canvas: rows = round(sqrt(n)), cols = ceil(n / rows); camera i in tile (i % rows, i //
    rows), column-major as datareader.py:364-374 index it."""
    rows = int(np.round(np.sqrt(int(n_cam))))
    return rows, -(-int(n_cam) // rows)


def replay_boxes(state7, dt, P1, P2=None, offset=0, count=None):
    """Rows [offset, offset + count) of state7 fp32 [R,7] = (x, y, l, w, h, direction, v), the objects of one label instant,
    in every camera: dt fp64 [C], P1 / P2 fp64 [C,3,4] -> (views fp32 [C*n,7], image corners fp64 [C*n,8,2], side int32 [C*n],
    camera int32 [C*n]); row c*n + i is object i in camera c (rn_replay_boxes)."""
    _hip.need_gpu(state7, dt, P1, P2)
    _typed("replay_boxes", ("state7", state7, torch.float32), ("dt", dt, torch.float64), ("P1", P1, torch.float64))
    if state7.dim() != 2 or state7.shape[1] != 7 or dt.dim() != 1 or dt.shape[0] < 1:
        raise RuntimeError("replay_boxes: state7 is fp32 [R,7] and dt fp64 [C], C >= 1, got %s and %s" % (tuple(state7.shape), tuple(dt.shape)))
    C, dev = dt.shape[0], state7.device
    for name, P in (("P1", P1), ("P2", P2)):
        if P is not None and (P.dtype != torch.float64 or tuple(P.shape) != (C, 3, 4) or not P.is_contiguous() or P.device != dev):
            raise RuntimeError("replay_boxes: %s is a contiguous fp64 [%d,3,4] tensor on state7's device, got %s %s"
                               % (name, C, P.dtype, tuple(P.shape)))
    if dt.device != dev:
        raise RuntimeError("replay_boxes: dt is on state7's device")
    offset = int(offset)
    n = state7.shape[0] - offset if count is None else int(count)
    if offset < 0 or n < 0 or offset + n > state7.shape[0]:
        raise RuntimeError("replay_boxes: rows [%d, %d) are outside the %d rows of state7" % (offset, offset + n, state7.shape[0]))
    if C > 65535 or C * n > 0x7FFFFFFF:
        raise RuntimeError("replay_boxes: too many cameras or rows")
    views = torch.empty((C * n, 7), dtype=torch.float32, device=dev)
    im = torch.empty((C * n, 8, 2), dtype=torch.float64, device=dev)
    side = torch.empty(C * n, dtype=torch.int32, device=dev)
    cam = torch.empty(C * n, dtype=torch.int32, device=dev)
    if n:
        _hip.call("rn_replay_boxes", state7.data_ptr() + 28 * offset, n, dt, P1, P2, C, views, im, side, cam, device=dev)
    return views, im, side, cam


def replay_compose(frames_u8, mask, size=None, swap_rb=False, out=None):
    """frames uint8 [n_cam,H,W,3] + mask uint16 [n_cam,H,W] (bits REPLAY_BITS) -> the uint8 RGB mosaic [OH,OW,3], tiles as
    ``replay_layout``; size = (OW, OH) or None for the canvas itself (rn_replay_compose)."""
    _hip.need_gpu(frames_u8, mask, out)
    n_cam, H, W = _render_plane("replay_compose", mask)
    if frames_u8.dtype != torch.uint8 or tuple(frames_u8.shape) != (n_cam, H, W, 3) or not frames_u8.is_contiguous() \
            or frames_u8.device != mask.device:
        raise RuntimeError("replay_compose: frames is a contiguous uint8 [%d,%d,%d,3] tensor on the mask's device, got %s %s"
                           % (n_cam, H, W, frames_u8.dtype, tuple(frames_u8.shape)))
    rows, cols = replay_layout(n_cam)
    if n_cam > 65535 or cols * W > REPLAY_MAX_CANVAS or rows * H > REPLAY_MAX_CANVAS:
        raise RuntimeError("replay_compose: the canvas %d x %d is larger than %d" % (cols * W, rows * H, REPLAY_MAX_CANVAS))
    OW, OH = (cols * W, rows * H) if size is None else (int(size[0]), int(size[1]))
    if not (1 <= OW <= RENDER_MAX_DIM and 1 <= OH <= RENDER_MAX_DIM):
        raise RuntimeError("replay_compose: the output size is (width, height), each in [1, %d], got %s" % (RENDER_MAX_DIM, (OW, OH)))
    if out is None:
        out = torch.empty((OH, OW, 3), dtype=torch.uint8, device=mask.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (OH, OW, 3) or not out.is_contiguous() or out.device != mask.device:
        raise RuntimeError("replay_compose: out is a contiguous uint8 [%d,%d,3] tensor on the mask's device" % (OH, OW))
    _hip.call("rn_replay_compose", frames_u8, int(bool(swap_rb)), mask, out, n_cam, H, W, rows, OW, OH, device=mask.device)
    return out


def _u8_frame(what, name, f):
    if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or not f.is_contiguous() or min(f.shape) < 1 \
            or max(f.shape[:2]) > RENDER_MAX_DIM:
        raise RuntimeError("%s: %s is a contiguous uint8 [H,W,3] frame (H, W <= %d), got %s %s"
                           % (what, name, RENDER_MAX_DIM, f.dtype, tuple(f.shape)))


def frame_absdiff(a, b, y0=100, y1=500, x0=100, x1=500):
    """sum |a - b| over a[y0:y1, x0:x1, :] of two uint8 [H,W,3] frames, the window clipped to the frame -> int64 [1] on the
    device, an exact integer (rn_frame_absdiff; datareader.py:617 divides it by the window's size)."""
    _hip.need_gpu(a, b)
    _u8_frame("frame_absdiff", "a", a)
    _u8_frame("frame_absdiff", "b", b)
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError("frame_absdiff: two frames of one size on one device, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    y0, y1, x0, x1 = (int(v) for v in (y0, y1, x0, x1))
    if min(y0, y1, x0, x1) < 0 or max(y0, y1, x0, x1) > 0x7FFFFFFF:
        raise RuntimeError("frame_absdiff: window bounds are non-negative int32")
    partial = torch.empty(REPLAY_ABSDIFF_BLOCKS, dtype=torch.int64, device=a.device)
    out = torch.empty(1, dtype=torch.int64, device=a.device)
    _hip.call("rn_frame_absdiff", a, b, a.shape[0], a.shape[1], y0, y1, x0, x1, partial, out, device=a.device)
    return out


def absdiff_window(H, W, y0=100, y1=500, x0=100, x1=500):
    """The number of bytes ``frame_absdiff`` sums for a frame of H x W: the clipped window's rows x columns x 3."""
    return max(min(int(y1), int(H)) - max(int(y0), 0), 0) * max(min(int(x1), int(W)) - max(int(x0), 0), 0) * 3


def running_frame(running, frame, first=False):
    """running fp64 [H,W,3] <- frame's values (first) or 0.95 * running + 0.05 * frame, one rounding per operation, in place
    (rn_running_frame; datareader.py:74-77).  -> running."""
    _hip.need_gpu(running, frame)
    _u8_frame("running_frame", "frame", frame)
    if running.dtype != torch.float64 or running.shape != frame.shape or not running.is_contiguous() or running.device != frame.device:
        raise RuntimeError("running_frame: running is a contiguous fp64 %s tensor on the frame's device, got %s %s"
                           % (tuple(frame.shape), running.dtype, tuple(running.shape)))
    _hip.call("rn_running_frame", running, frame, frame.numel(), int(bool(first)), device=frame.device)
    return running


# ------------------------------------------------------------------------------------------------ multi-camera label audit
LABEL_POINTS = 5                   # RN_LABEL_POINTS
LABEL_MAX_CAMS = 1024              # RN_LABEL_MAX_CAMS
LABEL_GUARD, LABEL_FOUND_CUR, LABEL_FOUND_PREV = 1, 2, 4
LABEL_BAD_OFFSETS, LABEL_BAD_FRAME, LABEL_BAD_PREFIX = 1, 2, 4
LABEL_BAD_CAMERA, LABEL_BAD_ERROR = 8, 16                      # of label_rebase
LABEL_BAD_TABLE = 32                                           # of the spline kernels
LABEL_BAD_GROUP = 64                                           # of label_group_rmse
_LABEL_BITS = ((LABEL_BAD_OFFSETS, "tracklet offsets out of order or outside the rows"),
               (LABEL_BAD_FRAME, "a frame index outside the frames or not ascending along its tracklet"),
               (LABEL_BAD_PREFIX, "more missing frames than output rows"),
               (LABEL_BAD_CAMERA, "a camera index outside the cameras"),
               (LABEL_BAD_ERROR, "a reprojection error that is not finite at a round's winning candidate"),
               (LABEL_BAD_TABLE, "a spline group, wave, spline index or row range outside its table"),
               (LABEL_BAD_GROUP, "group ids that do not ascend or lie outside the groups"))


def label_status(device, status=None):
    """The status word the three entry points OR their bits into: a zeroed int32 [1] unless one is handed on."""
    return _status_word("label", device, status)


def label_check(status):
    """Raises on a non-zero status word (an int, or the int32 [1] tensor: one element is read back)."""
    _refused("the label kernels refused their input: ", _LABEL_BITS, status)


def label_pair_index(cam, prev):
    """The pair index of (cam, prev < cam) in ``label_pair_samples``' output."""
    return cam * (cam - 1) // 2 + prev


def _label_table(what, offsets, cols, frame=None):
    _typed(what, ("offsets", offsets, torch.int64), ("cols", cols, torch.float64))
    if offsets.dim() != 1 or offsets.numel() < 1 or cols.dim() != 2 or cols.shape[1] != 3:
        raise RuntimeError("%s: offsets is int64 [T+1], cols fp64 [R,3]" % what)
    T, R = offsets.numel() - 1, cols.shape[0]
    if frame is not None:
        _typed(what, ("frame", frame, torch.int32))
        if tuple(frame.shape) != (R,):
            raise RuntimeError("%s: frame is int32 [R]" % what)
    if T >= 2 ** 31 or R >= 2 ** 31:
        raise RuntimeError("%s: more than 2^31 tracklets or rows" % what)
    return T, R


def label_pair_samples(offsets, cols, n_cam, key_col, val0, val1=-1, status=None):
    """seems_to_be_working.py:1889-1916 for every (camera pair, object): offsets int64 [n_ids * n_cam + 1] (tracklet = object *
    n_cam + camera), cols fp64 [R,3] (x, y, timestamp); key_col / val0 / val1 pick the columns (val1 -1: none) -> (flags uint8
    [P, n_ids, 5], values fp64 [P, n_ids, 5, 4] = (cam's val0, prev's val0, cam's val1, prev's val1), status); pair
    ``label_pair_index(cam, prev)``, P = n_cam (n_cam - 1) / 2."""
    _hip.need_gpu(offsets, cols)
    T, R = _label_table("label_pair_samples", offsets, cols)
    n_cam, key_col, val0, val1 = int(n_cam), int(key_col), int(val0), int(val1)
    if not 1 <= n_cam <= LABEL_MAX_CAMS or T % n_cam or key_col not in (0, 1, 2) or val0 not in (0, 1, 2) or val1 not in (-1, 0, 1, 2):
        raise RuntimeError("label_pair_samples: 1 <= n_cam <= %d divides the tracklet count, columns are 0..2 (val1 may be -1)"
                           % LABEL_MAX_CAMS)
    n_ids, P, dev = T // n_cam, n_cam * (n_cam - 1) // 2, cols.device
    status = label_status(dev, status)
    flags = torch.empty((P, n_ids, LABEL_POINTS), dtype=torch.uint8, device=dev)
    values = torch.empty((P, n_ids, LABEL_POINTS, 4), dtype=torch.float64, device=dev)
    _hip.call("rn_label_pair_samples", offsets, cols, R, n_cam, n_ids, key_col, val0, val1, flags, values, status, device=dev)
    return flags, values, status


def label_outliers(offsets, cols, frame, n_frames, n_visit, status=None):
    """seems_to_be_working.py:2195-2231 along every tracklet: frame int32 [R] (ascending inside a tracklet), n_frames =
    len(data), n_visit = the frames the walk reaches before its break -> (delete uint8 [R], status)."""
    _hip.need_gpu(offsets, cols, frame)
    T, R = _label_table("label_outliers", offsets, cols, frame)
    F, n_visit, dev = int(n_frames), int(n_visit), cols.device
    if not 0 <= F < 2 ** 31 or n_visit < 0:
        raise RuntimeError("label_outliers: 0 <= n_frames < 2^31, n_visit >= 0")
    status = label_status(dev, status)
    delete = torch.empty(R, dtype=torch.uint8, device=dev)
    _hip.call("rn_label_outliers", offsets, cols, frame, T, R, F, n_visit, delete, status, device=dev)
    return delete, status


def label_interpolate(offsets, cols, frame, all_ts, rows, status=None):
    """seems_to_be_working.py:800-828 for every missing frame between two present frames of every tracklet: all_ts fp64 [F,
    n_cam]; rows = the size of the output (the host knows it from the frame column) -> (out fp64 [rows,3] = (x, y, timestamp),
    out_src int32 [rows] = the row before the gap, out_frame int32 [rows], total int64 [1], status), in tracklet order, frames
    ascending."""
    lib = _hip.load()
    _hip.need_gpu(offsets, cols, frame, all_ts)
    T, R = _label_table("label_interpolate", offsets, cols, frame)
    _typed("label_interpolate", ("all_ts", all_ts, torch.float64))
    rows, dev = int(rows), cols.device
    if all_ts.dim() != 2 or not 1 <= all_ts.shape[1] <= LABEL_MAX_CAMS or T % all_ts.shape[1] or all_ts.shape[0] >= 2 ** 31 \
            or rows < 0:
        raise RuntimeError("label_interpolate: all_ts is fp64 [F, n_cam], n_cam divides the tracklet count, rows >= 0")
    F, n_cam = all_ts.shape
    status = label_status(dev, status)
    ws = torch.empty(max(16, lib.rn_label_interpolate_workspace_bytes(T, R)), dtype=torch.uint8, device=dev)
    out = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    out_src = torch.empty(rows, dtype=torch.int32, device=dev)
    out_frame = torch.empty(rows, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    _hip.call("rn_label_interpolate", offsets, cols, frame, all_ts, T, R, F, n_cam, rows, ws, out, out_src, out_frame, total, status,
              device=dev)
    return out, out_src, out_frame, total, status


# ------------------------------------------------------------------------------------------------ re-basing labels
LABEL_REBASE_MAX_GRID = 16         # RN_LABEL_REBASE_MAX_GRID
LABEL_REBASE_MAX_ROUNDS = 8        # RN_LABEL_REBASE_MAX_ROUNDS


def label_rebase_radii(search_rad=50, stop=1):
    """The radii of seems_to_be_working.py:1682-1706, by the reference's own ``search_rad /= 5``: [50, 10.0, 2.0]."""
    radii = []
    while search_rad > stop:
        radii.append(search_rad)
        search_rad /= 5
    return radii


def label_rebase(state6, cam, P1_old, P2_old, P1_new, P2_new, radii, grid=11, status=None):
    """seems_to_be_working.py:1677-1709 for every box, one wave each: state6 fp64 [n,6] = (x, y, l, w, h, direction), cam int32
    [n], P1_* fp64 [n_cam,3,4] (or [n_cam,12]), P2_* alike or None (no wrapper switch), radii fp64 [rounds] on the device,
    2 <= grid <= 16 -> (centre fp64 [n,2], err fp64 [n], idx int32 [n, rounds], status).  A box the kernel leaves out (its
    status bit is set) keeps NaN / -1."""
    _hip.need_gpu(state6, cam, P1_old, P2_old, P1_new, P2_new, radii)
    specs = [("state6", state6, torch.float64), ("cam", cam, torch.int32), ("P1_old", P1_old, torch.float64),
             ("P1_new", P1_new, torch.float64), ("radii", radii, torch.float64)]
    specs += [(k, v, torch.float64) for k, v in (("P2_old", P2_old), ("P2_new", P2_new)) if v is not None]
    _typed("label_rebase", *specs)
    n, n_cam, rounds, grid = state6.shape[0], P1_old.shape[0], radii.numel(), int(grid)
    if state6.dim() != 2 or state6.shape[1] != 6 or tuple(cam.shape) != (n,) or radii.dim() != 1 or n >= 2 ** 31:
        raise RuntimeError("label_rebase: state6 is fp64 [n,6], cam int32 [n], radii fp64 [rounds]")
    for k, v in (("P1_old", P1_old), ("P2_old", P2_old), ("P1_new", P1_new), ("P2_new", P2_new)):
        if v is not None and (v.numel() != n_cam * 12 or v.shape[0] != n_cam):
            raise RuntimeError("label_rebase: %s is fp64 [n_cam,3,4] for the %d cameras of P1_old" % (k, n_cam))
    if not 2 <= grid <= LABEL_REBASE_MAX_GRID or not 1 <= rounds <= LABEL_REBASE_MAX_ROUNDS or n_cam > LABEL_MAX_CAMS:
        raise RuntimeError("label_rebase: 2 <= grid <= %d, 1 <= rounds <= %d, at most %d cameras"
                           % (LABEL_REBASE_MAX_GRID, LABEL_REBASE_MAX_ROUNDS, LABEL_MAX_CAMS))
    dev = state6.device
    status = label_status(dev, status)
    centre = torch.empty((n, 2), dtype=torch.float64, device=dev)
    err = torch.empty(n, dtype=torch.float64, device=dev)
    idx = torch.empty((n, rounds), dtype=torch.int32, device=dev)
    _hip.call("rn_label_rebase", state6, cam, n, P1_old, P2_old, P1_new, P2_new, n_cam, radii, rounds, grid, centre, err, idx, status,
              device=dev)
    return centre, err, idx, status


def label_offset_y(xy, coef, y_straight, direction, reverse=False):
    """seems_to_be_working.py:1792-1802 for every box: xy fp64 [n,2], coef fp64 [n,3] = (p2, p1, p0), y_straight fp64 [n]
    (subtracted from the offset where direction is -1), direction int32 [n] -> y fp64 [n], y - offset or, reverse, y + offset."""
    _hip.need_gpu(xy, coef, y_straight, direction)
    _typed("label_offset_y", ("xy", xy, torch.float64), ("coef", coef, torch.float64), ("y_straight", y_straight, torch.float64),
           ("direction", direction, torch.int32))
    n = xy.shape[0]
    if xy.dim() != 2 or xy.shape[1] != 2 or tuple(coef.shape) != (n, 3) or tuple(y_straight.shape) != (n,) or \
            tuple(direction.shape) != (n,):
        raise RuntimeError("label_offset_y: xy is fp64 [n,2], coef fp64 [n,3], y_straight fp64 [n], direction int32 [n]")
    out = torch.empty(n, dtype=torch.float64, device=xy.device)
    _hip.call("rn_label_offset_y", xy, coef, y_straight, direction, n, int(bool(reverse)), out, device=xy.device)
    return out


# ------------------------------------------------------------------------------------------------ detector-assisted labelling
def _label_cameras(what, n, cam, P1, P2):
    specs = [("cam", cam, torch.int32), ("P1", P1, torch.float64)] + ([] if P2 is None else [("P2", P2, torch.float64)])
    _typed(what, *specs)
    n_cam = P1.shape[0] if P1.dim() else -1
    if tuple(cam.shape) != (n,) or n >= 2 ** 31:
        raise RuntimeError("%s: cam is int32 [n] for the n = %d boxes" % (what, n))
    for k, v in (("P1", P1), ("P2", P2)):
        if v is not None and (v.dim() < 2 or v.numel() != n_cam * 12 or v.shape[0] != n_cam):
            raise RuntimeError("%s: %s is fp64 [n_cam,3,4] for the cameras of P1" % (what, k))
    if n_cam > LABEL_MAX_CAMS:
        raise RuntimeError("%s: at most %d cameras" % (what, LABEL_MAX_CAMS))
    return n_cam


def label_crop_windows(state6, cam, P1, P2, ber=1.2, width=1920, height=1080, status=None):
    """manual_annotator_state_v3.py:662-673 and :707-717 for every box, one thread each: state6 fp32 [n,6] = (x, y, l, w, h,
    direction), cam int32 [n], P1 fp64 [n_cam,3,4] (or [n_cam,12]), P2 alike or None (no wrapper switch) -> (crop_box fp32 [n,4],
    rois fp32 [n,5] = (camera, window), win fp32 [n,3] = (minx, miny, scale), skipped uint8 [n], status).  A box whose crop box
    leaves the frame is flagged in ``skipped`` and keeps NaN in rois and win, as the reference returns silently."""
    _hip.need_gpu(state6, cam, P1, P2)
    _typed("label_crop_windows", ("state6", state6, torch.float32))
    if state6.dim() != 2 or state6.shape[1] != 6:
        raise RuntimeError("label_crop_windows: state6 is fp32 [n,6]")
    n = state6.shape[0]
    n_cam = _label_cameras("label_crop_windows", n, cam, P1, P2)
    dev = state6.device
    status = label_status(dev, status)
    crop_box = torch.empty((n, 4), dtype=torch.float32, device=dev)
    rois = torch.empty((n, 5), dtype=torch.float32, device=dev)
    win = torch.empty((n, 3), dtype=torch.float32, device=dev)
    skipped = torch.empty(n, dtype=torch.uint8, device=dev)
    _hip.call("rn_label_crop_windows", state6, cam, n, P1, P2, n_cam, float(ber), float(width), float(height), crop_box, rois, win,
              skipped, status, device=dev)
    return crop_box, rois, win, skipped, status


def label_best_anchor(cls, reg, win, cs=112):
    """manual_annotator_state_v3.py:731-740 for every crop, one wave each: cls fp32 [n,A,C] and reg fp32 [n,A,4] (the 2D
    localiser's LOCALIZE outputs), win fp32 [n,3] = (minx, miny, scale) -> (box fp32 [n,4] in frame coordinates, anchor int32
    [n], confidence fp32 [n], class int32 [n]).  torch.max / torch.argmax: a NaN counts as largest, equal values go to the
    lower index."""
    _hip.need_gpu(cls, reg, win)
    _typed("label_best_anchor", ("cls", cls, torch.float32), ("reg", reg, torch.float32), ("win", win, torch.float32))
    if cls.dim() != 3 or cls.shape[1] < 1 or cls.shape[2] < 1 or tuple(reg.shape) != (cls.shape[0], cls.shape[1], 4) or \
            tuple(win.shape) != (cls.shape[0], 3) or cls.shape[0] >= 2 ** 31 or cls.shape[1] * cls.shape[2] >= 2 ** 31:
        raise RuntimeError("label_best_anchor: cls is fp32 [n,A,C] with A, C >= 1, reg fp32 [n,A,4], win fp32 [n,3]")
    n, A, C = cls.shape
    dev = cls.device
    box = torch.empty((n, 4), dtype=torch.float32, device=dev)
    anchor = torch.empty(n, dtype=torch.int32, device=dev)
    conf = torch.empty(n, dtype=torch.float32, device=dev)
    klass = torch.empty(n, dtype=torch.int32, device=dev)
    _hip.call("rn_label_best_anchor", cls, reg, win, n, A, C, float(cs), box, anchor, conf, klass, device=dev)
    return box, anchor, conf, klass


def label_fit_box2d(tmpl, cam, centre, target, P1, P2, radii, grid=11, skip=None, status=None):
    """manual_annotator_state_v3.py:603-632 for every box, one wave each: tmpl fp32 [n,4] = (l, w, h, direction), cam int32 [n],
    centre fp32 [n,2] (where the search starts), target fp32 [n,4] = (x1, y1, x2, y2), P1 fp64 [n_cam,3,4] (or [n_cam,12]), P2
    alike or None (no wrapper switch), radii fp64 [rounds] on the device (``label_rebase_radii``), 2 <= grid <= 16 -> (centre
    fp32 [n,2], err fp32 [n], idx int32 [n, rounds], status).  A box the kernel leaves out (its status bit is set) keeps
    NaN / -1, and so does, without a status bit, a box whose byte of ``skip`` (uint8 [n], ``label_crop_windows``' skipped) is
    set."""
    _hip.need_gpu(tmpl, cam, centre, target, P1, P2, radii, skip)
    _typed("label_fit_box2d", ("tmpl", tmpl, torch.float32), ("centre", centre, torch.float32),
           ("target", target, torch.float32), ("radii", radii, torch.float64))
    n, rounds, grid = tmpl.shape[0] if tmpl.dim() else -1, radii.numel(), int(grid)
    if tuple(tmpl.shape) != (n, 4) or tuple(centre.shape) != (n, 2) or tuple(target.shape) != (n, 4) or radii.dim() != 1:
        raise RuntimeError("label_fit_box2d: tmpl is fp32 [n,4], centre fp32 [n,2], target fp32 [n,4], radii fp64 [rounds]")
    if skip is not None:
        _typed("label_fit_box2d", ("skip", skip, torch.uint8))
        if tuple(skip.shape) != (n,):
            raise RuntimeError("label_fit_box2d: skip is uint8 [n]")
    n_cam = _label_cameras("label_fit_box2d", n, cam, P1, P2)
    if not 2 <= grid <= LABEL_REBASE_MAX_GRID or not 1 <= rounds <= LABEL_REBASE_MAX_ROUNDS:
        raise RuntimeError("label_fit_box2d: 2 <= grid <= %d, 1 <= rounds <= %d" % (LABEL_REBASE_MAX_GRID, LABEL_REBASE_MAX_ROUNDS))
    dev = tmpl.device
    status = label_status(dev, status)
    out = torch.empty((n, 2), dtype=torch.float32, device=dev)
    err = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty((n, rounds), dtype=torch.int32, device=dev)
    _hip.call("rn_label_fit_box2d", tmpl, cam, centre, target, skip, n, P1, P2, n_cam, radii, rounds, grid, out, err, idx, status,
              device=dev)
    return out, err, idx, status


# ------------------------------------------------------------------------------------------------ spline trajectories
SPLINE_GRP, SPLINE_WS_COLS, SPLINE_FIGS, SPLINE_MAX_NCAP = 8, 19, 5, 4096     # RN_SPLINE_*
SPLINE_UNUSED, SPLINE_STUCK, SPLINE_REJECTED = 97, 98, 99
SPLINE_METRICS = {"ape": 0}                                    # any other metric: the reference's ``else`` branch (1)


def spline_metric(metric):
    return SPLINE_METRICS.get(metric, 1) if isinstance(metric, str) else int(metric)


def spline_waves(grp):
    """Host side of ``spline_fit``: grp int32 [G, 8] (numpy) = (row0, m, k, ncap, cand0, ncand, -, axis) -> waves int32 [NW, 2] =
    (group, first candidate); column 6 of grp is filled with each group's first wave.  The 64 lanes of a wave are consecutive
    candidates of one group."""
    import numpy as np
    waves, w = [], 0
    for g in range(len(grp)):
        grp[g, 6] = w
        for c0 in range(0, int(grp[g, 5]), 64):
            waves.append((g, c0))
            w += 1
    return np.array(waves, np.int32).reshape(-1, 2)


def label_box_weights(state6, cam, P1, P2=None, status=None):
    """seems_to_be_working.py:1186-1196 for every box: state6 fp64 [n,6] = (x, y, l, w, h, direction), cam int32 [n], P1 / P2 fp64
    [n_cam,12] (P2 None: no wrapper switch) -> (out fp64 [n,4] = (x_weight, y_weight, x_diff, y_diff), status)."""
    _hip.need_gpu(state6, cam, P1, P2)
    specs = [("state6", state6, torch.float64), ("cam", cam, torch.int32), ("P1", P1, torch.float64)]
    _typed("label_box_weights", *(specs + ([("P2", P2, torch.float64)] if P2 is not None else [])))
    n, n_cam = state6.shape[0], P1.shape[0]
    if state6.dim() != 2 or state6.shape[1] != 6 or tuple(cam.shape) != (n,) or P1.numel() != n_cam * 12 or n >= 2 ** 31 or \
            not 1 <= n_cam <= LABEL_MAX_CAMS or (P2 is not None and tuple(P2.shape) != tuple(P1.shape)):
        raise RuntimeError("label_box_weights: state6 is fp64 [n,6], cam int32 [n], P1 and P2 fp64 [n_cam,12]")
    dev = state6.device
    status = label_status(dev, status)
    out = torch.empty((n, 4), dtype=torch.float64, device=dev)
    _hip.call("rn_label_box_weights", state6, cam, n, P1, P2, n_cam, out, status, device=dev)
    return out, status


def _spline_rows(what, grp, tx, *cols):
    _typed(what, ("grp", grp, torch.int32), ("tx", tx, torch.float64), *[("column", c, torch.float64) for c in cols])
    if grp.dim() != 2 or grp.shape[1] != SPLINE_GRP or tx.dim() != 1 or any(tuple(c.shape) != tuple(tx.shape) for c in cols) or \
            grp.shape[0] >= 2 ** 31 or tx.numel() >= 2 ** 31:
        raise RuntimeError("%s: grp is int32 [G,%d], tx and the other columns fp64 [R]" % (what, SPLINE_GRP))
    return grp.shape[0], tx.numel()


def _spline_ncap(what, ncap):
    ncap = int(ncap)
    if not 6 <= ncap <= SPLINE_MAX_NCAP:
        raise RuntimeError("%s: 6 <= ncap <= %d" % (what, SPLINE_MAX_NCAP))
    return ncap


def spline_workspace_bytes(n_waves, ncap):
    return int(_hip.load().rn_spline_fit_workspace_bytes(int(n_waves), int(ncap)))


def spline_fit(grp, waves, tx, val, wt, s, ncap, workspace=None, status=None):
    """FITPACK curfit (iopt = 0) for every candidate smoothing factor, one lane each: grp int32 [G,8] and waves int32 [NW,2] from
    ``spline_waves``, tx / val / wt fp64 [R], s fp64 [NC], ncap = the largest knot count any lane may reach -> (workspace fp64
    [19 * ncap, NW * 64] (row 0.. the knots t, row ncap.. the coefficients c of every lane), n int32 [NW * 64], ier int32,
    fp fp64, iterations int32, status).  ``workspace``: a tensor of a former call to reuse (at least as large)."""
    _hip.need_gpu(grp, waves, tx, val, wt, s, workspace)
    G, R = _spline_rows("spline_fit", grp, tx, val, wt)
    _typed("spline_fit", ("waves", waves, torch.int32), ("s", s, torch.float64))
    ncap = _spline_ncap("spline_fit", ncap)
    if waves.dim() != 2 or waves.shape[1] != 2 or s.dim() != 1 or waves.shape[0] >= 2 ** 25 or s.numel() >= 2 ** 31:
        raise RuntimeError("spline_fit: waves is int32 [NW,2], s fp64 [NC]")
    NW, dev = waves.shape[0], tx.device
    NL = NW * 64
    status = label_status(dev, status)
    need = SPLINE_WS_COLS * ncap * NL
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or not workspace.is_contiguous() or workspace.numel() < need:
        raise RuntimeError("spline_fit: the workspace is a contiguous fp64 tensor of at least %d elements" % need)
    n = torch.empty(NL, dtype=torch.int32, device=dev)
    ier = torch.empty(NL, dtype=torch.int32, device=dev)
    fp = torch.empty(NL, dtype=torch.float64, device=dev)
    iters = torch.empty(NL, dtype=torch.int32, device=dev)
    _hip.call("rn_spline_fit", grp, G, waves, NW, tx, val, wt, R, s, s.numel(), ncap, workspace, n, ier, fp, iters, status, device=dev)
    return workspace.reshape(-1)[:need].view(SPLINE_WS_COLS * ncap, NL), n, ier, fp, iters, status


def spline_select(grp, tx, val, wt, wscore, n_cand, ncap, workspace, n, ier, fp, metric="ape", status=None):
    """seems_to_be_working.py:1238-1294 for every group, one workgroup each, on the output of ``spline_fit`` -> (scores fp64 [NC]
    (NaN: skipped), win int32 [G,3] = (candidate or -1, n, ier), figures fp64 [G,5] = (fp, score, sqrt(mean r^2), sqrt(mean (w
    r)^2), sqrt(max (w r)^2)), t fp64 [G, ncap], c fp64 [G, ncap], status)."""
    _hip.need_gpu(grp, tx, val, wt, wscore, workspace, n, ier, fp)
    G, R = _spline_rows("spline_select", grp, tx, val, wt, wscore)
    _typed("spline_select", ("workspace", workspace, torch.float64), ("n", n, torch.int32), ("ier", ier, torch.int32),
           ("fp", fp, torch.float64))
    ncap, NC, NL = _spline_ncap("spline_select", ncap), int(n_cand), n.numel()
    if NL % 64 or tuple(ier.shape) != (NL,) or tuple(fp.shape) != (NL,) or workspace.numel() < SPLINE_WS_COLS * ncap * NL or \
            not 0 <= NC < 2 ** 31:
        raise RuntimeError("spline_select: n, ier, fp are [NW * 64] and the workspace is spline_fit's for the same ncap")
    dev = tx.device
    status = label_status(dev, status)
    scores = torch.empty(NC, dtype=torch.float64, device=dev)
    win = torch.empty((G, 3), dtype=torch.int32, device=dev)
    fig = torch.empty((G, SPLINE_FIGS), dtype=torch.float64, device=dev)
    t = torch.empty((G, ncap), dtype=torch.float64, device=dev)
    c = torch.empty((G, ncap), dtype=torch.float64, device=dev)
    _hip.call("rn_spline_select", grp, G, tx, val, wt, wscore, R, NC, NL // 64, ncap, workspace, n, ier, fp, spline_metric(metric),
              scores, win, fig, t, c, status, device=dev)
    return scores, win, fig, t, c, status


def _spline_pack(what, st, sc, snk):
    _typed(what, ("st", st, torch.float64), ("sc", sc, torch.float64), ("snk", snk, torch.int32))
    if st.dim() != 2 or tuple(sc.shape) != tuple(st.shape) or tuple(snk.shape) != (st.shape[0], 2) or st.shape[0] >= 2 ** 31:
        raise RuntimeError("%s: st and sc are fp64 [S, ncap], snk int32 [S,2] = (n, k)" % what)
    return st.shape[0], _spline_ncap(what, st.shape[1])


def spline_eval(st, sc, snk, qs, qt):
    """FITPACK splev with extrapolation, one thread per query: st / sc fp64 [S, ncap] the knots and coefficients, snk int32 [S,2] =
    (n, k) (n = 0: no spline), qs int32 [Q] the spline of every query, qt fp64 [Q] -> fp64 [Q] (NaN without a spline)."""
    _hip.need_gpu(st, sc, snk, qs, qt)
    S, ncap = _spline_pack("spline_eval", st, sc, snk)
    _typed("spline_eval", ("qs", qs, torch.int32), ("qt", qt, torch.float64))
    if qs.dim() != 1 or tuple(qt.shape) != tuple(qs.shape):
        raise RuntimeError("spline_eval: qs is int32 [Q], qt fp64 [Q]")
    out = torch.empty(qs.numel(), dtype=torch.float64, device=st.device)
    _hip.call("rn_spline_eval", st, sc, snk, S, ncap, qs, qt, qs.numel(), out, device=st.device)
    return out


def label_ts_shift(st, sc, snk, off, rs, rx, base, run, shifts, use_run=True, metric="ape", status=None):
    """seems_to_be_working.py:1416-1442 for every (frame, camera) entry, one wave each: the packed splines of ``spline_eval``, off
    int64 [E+1] the rows of every entry, rs int32 [Rr] / rx fp64 [Rr] the spline and the label x of its kept objects, base / run
    fp64 [E] the camera's time stamp and running error, shifts fp64 [trials < 64] -> (best_t fp64 [E], errs fp64 [E,2] = (best,
    initial), best_i int32 [E], status)."""
    _hip.need_gpu(st, sc, snk, off, rs, rx, base, run, shifts)
    S, ncap = _spline_pack("label_ts_shift", st, sc, snk)
    _typed("label_ts_shift", ("off", off, torch.int64), ("rs", rs, torch.int32), ("rx", rx, torch.float64),
           ("base", base, torch.float64), ("run", run, torch.float64), ("shifts", shifts, torch.float64))
    E, Rr, trials = off.numel() - 1, rs.numel(), shifts.numel()
    if off.dim() != 1 or E < 0 or rs.dim() != 1 or tuple(rx.shape) != (Rr,) or tuple(base.shape) != (E,) or tuple(run.shape) != (E,) \
            or shifts.dim() != 1 or not 1 <= trials < 64 or E >= 2 ** 31 or Rr >= 2 ** 31:
        raise RuntimeError("label_ts_shift: off is int64 [E+1], rs int32 [Rr], rx fp64 [Rr], base and run fp64 [E], 1 <= trials < 64")
    dev = st.device
    status = label_status(dev, status)
    best_t = torch.empty(E, dtype=torch.float64, device=dev)
    errs = torch.empty((E, 2), dtype=torch.float64, device=dev)
    best_i = torch.empty(E, dtype=torch.int32, device=dev)
    _hip.call("rn_label_ts_shift", st, sc, snk, S, ncap, off, rs, rx, E, Rr, base, run, shifts, trials, int(bool(use_run)),
              spline_metric(metric), best_t, errs, best_i, status, device=dev)
    return best_t, errs, best_i, status


# ------------------------------------------------------------------------------------------------ label quality
LABEL_SERIES_PLANES, LABEL_SERIES_MAX_LDS_ROWS = 7, 4096       # RN_LABEL_SERIES_*


def label_series(offsets, cols, n_cam, lane=None, lds_rows=None, status=None):
    """manual_annotator_state_v3.py:3847-3958 for every object, one workgroup each: the audit's table (offsets int64 [n_ids *
    n_cam + 1], cols fp64 [R,3] = (x, y, timestamp)); lane (lo, hi) keeps the rows with lo < y < hi only; lds_rows, a power of
    two in 2 .. 4096 (the default), is the largest object sorted in LDS, a longer one goes through a global workspace with the
    same result -> (order int32 [R], keep uint8 [R], series fp64 [7, R] = t, x, y, v, vy, a, theta, counts int32 [n_ids,3] = (n,
    m, feasible segments), figs fp64 [n_ids,2] = (range, variation), status): include/retinanet_mi355x.h."""
    lib = _hip.load()
    _hip.need_gpu(offsets, cols)
    T, R = _label_table("label_series", offsets, cols)
    n_cam = int(n_cam)
    lds_rows = LABEL_SERIES_MAX_LDS_ROWS if lds_rows is None else int(lds_rows)
    if not 1 <= n_cam <= LABEL_MAX_CAMS or T % n_cam:
        raise RuntimeError("label_series: 1 <= n_cam <= %d divides the tracklet count" % LABEL_MAX_CAMS)
    if not 2 <= lds_rows <= LABEL_SERIES_MAX_LDS_ROWS or lds_rows & (lds_rows - 1):
        raise RuntimeError("label_series: lds_rows is a power of two, 2 .. %d" % LABEL_SERIES_MAX_LDS_ROWS)
    lo, hi = (0.0, 0.0) if lane is None else (float(lane[0]), float(lane[1]))
    n_ids, dev = T // n_cam, cols.device
    status = label_status(dev, status)
    ws = torch.empty(max(16, lib.rn_label_series_workspace_bytes(R)), dtype=torch.uint8, device=dev)
    order = torch.empty(R, dtype=torch.int32, device=dev)
    keep = torch.empty(R, dtype=torch.uint8, device=dev)
    series = torch.empty((LABEL_SERIES_PLANES, R), dtype=torch.float64, device=dev)
    counts = torch.empty((n_ids, 3), dtype=torch.int32, device=dev)
    figs = torch.empty((n_ids, 2), dtype=torch.float64, device=dev)
    _hip.call("rn_label_series", offsets, cols, R, n_cam, n_ids, int(lane is not None), lo, hi, lds_rows, ws, order, keep, series,
              counts, figs, status, device=dev)
    return order, keep, series, counts, figs, status


def label_group_rmse(im, group, n_groups, status=None):
    """manual_annotator_state_v3.py:3997-4000 for every group, one workgroup each: im fp64 [n,8,2] (``hg_to_im``), group int32
    [n], ascending ids in [0, n_groups) -> (rmse fp64 [n_groups], mean fp64 [n_groups,2], count int32 [n_groups], status); an
    empty group gives NaN, NaN, 0."""
    _hip.need_gpu(im, group)
    _typed("label_group_rmse", ("im", im, torch.float64), ("group", group, torch.int32))
    n, G = group.numel(), int(n_groups)
    if group.dim() != 1 or tuple(im.shape) != (n, 8, 2) or n >= 2 ** 31 or not 0 <= G < 2 ** 31:
        raise RuntimeError("label_group_rmse: im is fp64 [n,8,2], group int32 [n], 0 <= n_groups < 2^31")
    dev = im.device
    status = label_status(dev, status)
    rmse = torch.empty(G, dtype=torch.float64, device=dev)
    mean = torch.empty((G, 2), dtype=torch.float64, device=dev)
    count = torch.empty(G, dtype=torch.int32, device=dev)
    _hip.call("rn_label_group_rmse", im, group, n, G, rmse, mean, count, status, device=dev)
    return rmse, mean, count, status

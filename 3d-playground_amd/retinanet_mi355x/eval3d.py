"""Validation of the directional detector in 3D: average precision on the overlap of projected cuboids, and the corner
errors of the matched boxes.  ``retinanet/eval3d.py`` re-exports it.  The reference has no counterpart: its csv_eval.py
scores four columns, here columns 16:20 (csv_eval.evaluate), and says nothing about the sixteen corner coordinates the
loss trains and the tracker consumes.

Detections are what the directional model returns per image: scores [K], labels [K], boxes [K,20], columns 0:16 the
corners fbl fbr bbl bbr ftl ftr btl btr as (x, y).  Ground truth is the trainer's own label layout, [n, >=21] per image
(columns 0:16 the corners, column 20 the class, class -1 padding) or a batched [B,N,21] / [B,N,27] tensor as
corrected_3D_dataset.collate produces it -- a held-out slice of the training loader is a validation set.

The overlap of a detection and an annotation is the IoU of two convex polygons: the hulls of all 8 corners
("silhouette"), of corners 0..3 ("base") or of corners 4..7 ("top"), clipped exactly in fp64 (ops.eval_cuboid_overlap).
Matching is the reference's rule (csv_eval.py:189-213) on that overlap, per threshold; AP per threshold and class comes from
ops.eval_ap.  For the true positives at iou_thresholds[0] the mean IoU, the mean corner error in pixels, the same
relative to the diagonal of the annotation's corner envelope, and the number of boxes that fit better turned by 180
degrees are reported per class.  One packed upload of the annotations, one copy back."""
from __future__ import print_function

import numpy as np
import torch

from . import ops


def _as_numpy(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def split_labels(labels):
    """The ground truth as a list of per-image float64 arrays [n, >=21] without padding rows: a batched [B,N,>=21] tensor
    or array is B images; a sequence holds per-image arrays and / or batched ones."""
    if torch.is_tensor(labels) or isinstance(labels, np.ndarray):
        labels = [labels]
    out = []
    for item in labels:
        a = _as_numpy(item)
        if a.ndim == 3:
            per = list(a)
        elif a.ndim == 2 or a.size == 0:
            per = [a.reshape(-1, a.shape[-1] if a.ndim == 2 and a.size else 21)]
        else:
            raise RuntimeError("eval3d: a label array is [n, >=21] or [B, N, >=21], got %s" % (a.shape,))
        for p in per:
            if p.shape[0] and p.shape[1] < 21:
                raise RuntimeError("eval3d: labels carry the corners in columns 0:16 and the class in column 20, got %s" % (p.shape,))
            out.append(p[p[:, 20] != -1] if p.shape[0] else p)
    return out


def _pack_labels(per_image, num_classes):
    """One host buffer: int32 offsets [I*C+1] | float64 thresholds are appended by the caller | float64 corners [M,16]
    grouped by (image, class), the annotations of a class in label order.  A class outside [0, num_classes) is an error."""
    corners, off = [], [0]
    for a in per_image:
        cls = a[:, 20] if a.shape[0] else np.zeros(0)
        if a.shape[0] and (np.any(cls != np.floor(cls)) or np.any(cls < 0) or np.any(cls >= num_classes)):
            raise RuntimeError("eval3d: an annotation's class is outside [0, %d)" % num_classes)
        for c in range(num_classes):
            mine = a[cls == c][:, :16] if a.shape[0] else np.zeros((0, 16))
            corners.append(mine)
            off.append(off[-1] + mine.shape[0])
    return (np.ascontiguousarray(np.concatenate(corners).reshape(-1, 16)) if corners else np.zeros((0, 16))), np.asarray(off, np.int32)


class _Evaluation3D:
    """The device state of one evaluation: table, corners, annotations, results."""

    def __init__(self, per_image, num_classes, device, rows, overlap, iou_thresholds, max_detections):
        if overlap not in ops.EVAL_CUBOID_OVERLAPS:
            raise RuntimeError("eval3d: overlap is one of %s, got %r" % (sorted(ops.EVAL_CUBOID_OVERLAPS), overlap))
        self.thresholds = [float(t) for t in iou_thresholds]
        if not 1 <= len(self.thresholds) <= ops.EVAL_CUBOID_MAX_THRESHOLDS:
            raise RuntimeError("eval3d: 1 to %d IoU thresholds, got %d" % (ops.EVAL_CUBOID_MAX_THRESHOLDS, len(self.thresholds)))
        self.I, self.C, self.T, self.overlap = len(per_image), int(num_classes), len(self.thresholds), overlap
        corners, off = _pack_labels(per_image, self.C)
        self.M = corners.shape[0]
        head = (off.nbytes + 7) // 8 * 8
        buf = np.zeros(head + 8 * self.T + corners.nbytes, dtype=np.uint8)
        buf[:off.nbytes] = off.view(np.uint8)
        buf[head:head + 8 * self.T] = np.asarray(self.thresholds, np.float64).view(np.uint8)
        buf[head + 8 * self.T:] = corners.reshape(-1).view(np.uint8)
        packed = torch.from_numpy(buf).to(device)                              # the one upload
        self.ann_offsets = packed[:off.nbytes].view(torch.int32)
        self.thr = packed[head:head + 8 * self.T].view(torch.float64)
        self.ann_corners = packed[head + 8 * self.T:].view(torch.float64).view(self.M, 16)
        self.table, self.img_rows, _ = ops.eval_table(rows, self.I, device)
        self.corners = torch.zeros((rows, 16), dtype=torch.float32, device=device)
        # AP [T,C] f64 | sums [C,5] f64 | annotation counts [C] i32 | cursor, status i32: read back in one copy
        T, C = self.T, self.C
        self.result = torch.zeros(8 * T * C + 40 * C + 4 * C + 8, dtype=torch.uint8, device=device)
        self.ap = self.result[:8 * T * C].view(torch.float64).view(T, C)
        self.sums = self.result[8 * T * C:8 * T * C + 40 * C].view(torch.float64).view(C, 5)
        self.counts = self.result[8 * T * C + 40 * C:8 * T * C + 44 * C].view(torch.int32)
        self.state = self.result[8 * T * C + 44 * C:].view(torch.int32)
        self.max_detections = int(max_detections)

    def add(self, image, scores, labels, boxes, score_threshold):
        if boxes.numel() and (boxes.dim() != 2 or boxes.shape[1] != 20):
            raise RuntimeError("eval3d: the directional model's boxes are [K,20], got %s" % (tuple(boxes.shape),))
        ops.eval_select(scores, labels, boxes, self.table, self.img_rows, self.state, image, self.C, score_threshold,
                        self.max_detections, (16, 20) if boxes.numel() else None)
        ops.eval_corners(boxes, self.table, self.img_rows, image, self.corners)

    def finish(self):
        T, C = self.T, self.C
        best_iou, best_ann = ops.eval_cuboid_overlap(self.table, self.img_rows, self.corners, self.ann_corners, self.ann_offsets,
                                                     C, self.overlap)
        tp, _, matched = ops.eval_cuboid_assign(self.table, self.img_rows, best_iou, best_ann, self.ann_offsets, self.M, C,
                                                self.thr, num_annotations=self.counts)
        for t in range(T):
            ops.eval_ap(self.table, self.state, tp[t], self.counts, ap=self.ap[t])
        ops.eval_cuboid_errors(self.table, self.state, self.img_rows, self.corners, self.ann_corners, self.ann_offsets, C, tp[0],
                               matched, best_iou, sums=self.sums)
        host = self.result.cpu().numpy()                                       # the one read
        ap = host[:8 * T * C].view(np.float64).reshape(T, C)
        sums = host[8 * T * C:8 * T * C + 40 * C].view(np.float64).reshape(C, 5)
        counts = host[8 * T * C + 40 * C:8 * T * C + 44 * C].view(np.int32)
        status = int(host[8 * T * C + 44 * C:].view(np.int32)[1])
        if status != ops.EVAL_OK:
            raise RuntimeError("eval3d: " + ops.eval_status_text(status))
        out = {"ap": {}, "mAP": {}, "errors": {}}
        for t, thr in enumerate(self.thresholds):
            out["ap"][thr] = {c: ((float(ap[t, c]), float(counts[c])) if counts[c] else (0, 0)) for c in range(C)}
            have = [float(ap[t, c]) for c in range(C) if counts[c]]
            out["mAP"][thr] = sum(have) / len(have) if have else 0.0
        for c in range(C):
            n = float(sums[c, 0])
            out["errors"][c] = {"tp": int(n), "iou": float(sums[c, 1]) / n if n else 0.0,
                                "corner_px": float(sums[c, 2]) / n if n else 0.0,
                                "corner_rel": float(sums[c, 3]) / n if n else 0.0, "reversed": int(sums[c, 4])}
        return out


def evaluate_cuboids(detections, labels, num_classes, overlap="silhouette", iou_thresholds=(0.5, 0.7), score_threshold=0.05,
                     max_detections=100):
    """detections: per image (scores [K], labels [K], boxes [K,20]) device tensors; labels: the ground truth (split_labels).
    -> {"ap": {t: {label: (ap, n_annotations)}}, "mAP": {t: mean over the classes with annotations},
        "errors": {label: {"tp", "iou", "corner_px", "corner_rel", "reversed"}}} of Python numbers."""
    detections = list(detections)
    per_image = split_labels(labels)
    if len(detections) != len(per_image):
        raise RuntimeError("evaluate_cuboids: %d images of detections, %d of labels" % (len(detections), len(per_image)))
    if not detections:
        raise RuntimeError("evaluate_cuboids: no images")
    device = detections[0][0].device
    rows = sum(min(int(d[0].shape[0]), int(max_detections)) for d in detections)
    ev = _Evaluation3D(per_image, num_classes, device, rows, overlap, iou_thresholds, max_detections)
    for i, (scores, det_labels, boxes) in enumerate(detections):
        ev.add(i, scores, det_labels, boxes, score_threshold)
    return ev.finish()


def evaluate_3d(batches, net, num_classes=None, overlap="silhouette", iou_thresholds=(0.5, 0.7), score_threshold=0.05,
                max_detections=100):
    """Runs ``net`` in eval mode image by image over an iterable of (im [B,3,H,W], label [B,N,>=21]) batches -- what the
    training loader yields -- and scores its boxes against the labels.  num_classes defaults to the model's."""
    batches = list(batches)
    per_image = split_labels([label for _, label in batches])
    if num_classes is None:
        num_classes = net.classificationModel.num_classes
    net.eval()
    device = next(net.parameters()).device
    ev = _Evaluation3D(per_image, num_classes, device, len(per_image) * int(max_detections), overlap, iou_thresholds,
                       max_detections)
    index = 0
    with torch.no_grad():
        for im, _ in batches:
            for b in range(im.shape[0]):
                scores, labels, boxes = net(im[b:b + 1].to(device).float())
                ev.add(index, scores, labels, boxes, score_threshold)
                index += 1
    return ev.finish()


def validator(batches, **kwargs):
    """-> ``validate(net, epoch)`` for trainer.train: evaluate_3d over ``batches`` (an iterable of (im, label) batches, or a
    callable epoch -> such an iterable, like the trainer's own ``batches``) with the keyword arguments given."""
    def validate(net, epoch):
        return evaluate_3d(batches(epoch) if callable(batches) else batches, net, **kwargs)
    return validate

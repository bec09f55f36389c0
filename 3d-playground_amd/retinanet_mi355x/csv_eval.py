"""The reference's retinanet/csv_eval.py (one file for R/ and D/) under its own names: per-class average precision of a
detector over a dataset, computed on the device.  ``retinanet/csv_eval.py`` and ``flat2d/retinanet/csv_eval.py`` re-export it.

The reference copies every image's detections to the host, appends them one at a time to numpy arrays and sorts per
class on the host.  Here the model's outputs go straight into a device table (ops.eval_select, one launch per image),
the annotations are uploaded in ONE packed copy, matching / sort / AP run as kernels (ops.eval_match, ops.eval_ap) and the
host reads ONE buffer at the end: AP, annotation counts and the status word.

Two deliberate differences, see INTEGRATION.md: equal scores keep dataset order (the reference's np.argsort leaves it
open), and ``box_cols`` names the four box columns -- (0, 4) for [K,4] boxes, (16, 20) for the directional model's
[K,20] rows, where the reference would read two corner points as a box.
"""
from __future__ import print_function

import numpy as np
import torch

from . import ops


def compute_overlap(a, b):
    """csv_eval.py:11-35: IoU of a (N, 4) against b (K, 4) -> (N, K), numpy on the host (a helper of the reference's
    public surface; evaluate() does not call it)."""
    a, b = np.asarray(a), np.asarray(b)
    ax1, ay1, ax2, ay2 = (a[:, k][:, None] for k in range(4))
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(ax2, b[:, 2]) - np.maximum(ax1, b[:, 0]), 0)
    ih = np.maximum(np.minimum(ay2, b[:, 3]) - np.maximum(ay1, b[:, 1]), 0)
    union = np.maximum((ax2 - ax1) * (ay2 - ay1) + area_b - iw * ih, np.finfo(float).eps)
    return iw * ih / union


def _compute_ap(recall, precision):
    """csv_eval.py:38-62: area under the precision envelope, numpy on the host (see compute_overlap)."""
    mrec = np.concatenate(([0.], recall, [1.]))
    mpre = np.concatenate(([0.], precision, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def _pack_annotations(annotations, num_classes):
    """One host buffer: int32 offsets [I*C+1] (padded to 8 bytes), then float64 boxes [M,4]."""
    boxes, off = [], [0]
    for per_image in annotations:
        for label in range(num_classes):
            a = np.asarray(per_image[label], dtype=np.float64)
            a = a.reshape(-1, a.shape[-1] if a.ndim == 2 and a.size else 4)[:, :4]
            boxes.append(a)
            off.append(off[-1] + a.shape[0])
    off = np.asarray(off, dtype=np.int32)
    box = np.ascontiguousarray(np.concatenate(boxes).reshape(-1, 4)) if boxes else np.zeros((0, 4))
    head = (off.nbytes + 7) // 8 * 8
    buf = np.zeros(head + box.nbytes, dtype=np.uint8)
    buf[:off.nbytes] = off.view(np.uint8)
    buf[head:] = box.reshape(-1).view(np.uint8)
    return buf, len(off), head, box.shape[0]


class _Evaluation:
    """The device state of one evaluation: table, annotations, results."""

    def __init__(self, annotations, num_classes, device, rows, max_detections):
        self.I, self.C = len(annotations), int(num_classes)
        buf, n_off, head, M = _pack_annotations(annotations, self.C)
        packed = torch.from_numpy(buf).to(device)                              # the one upload
        self.ann_offsets = packed[:4 * n_off].view(torch.int32)
        self.ann_box = packed[head:].view(torch.float64).view(M, 4)
        self.table, self.img_rows, _ = ops.eval_table(rows, self.I, device)
        # AP [C] f64 | annotation counts [C] i32 | cursor, status i32: read back in one copy
        self.result = torch.zeros(12 * self.C + 8, dtype=torch.uint8, device=device)
        self.ap = self.result[:8 * self.C].view(torch.float64)
        self.counts = self.result[8 * self.C:12 * self.C].view(torch.int32)
        self.state = self.result[12 * self.C:].view(torch.int32)
        self.max_detections = int(max_detections)

    def add(self, image, scores, labels, boxes, score_threshold, box_cols):
        ops.eval_select(scores, labels, boxes, self.table, self.img_rows, self.state, image, self.C, score_threshold,
                        self.max_detections, box_cols)

    def finish(self, iou_threshold):
        tp, _ = ops.eval_match(self.table, self.img_rows, self.ann_box, self.ann_offsets, self.C, iou_threshold,
                               num_annotations=self.counts)
        ops.eval_ap(self.table, self.state, tp, self.counts, ap=self.ap)
        host = self.result.cpu().numpy()                                       # the one read
        ap = host[:8 * self.C].view(np.float64)
        counts = host[8 * self.C:12 * self.C].view(np.int32)
        status = int(host[12 * self.C:].view(np.int32)[1])
        if status != ops.EVAL_OK:
            raise RuntimeError("csv_eval: " + ops.eval_status_text(status))
        return {label: ((float(ap[label]), float(counts[label])) if counts[label] else (0, 0)) for label in range(self.C)}


def evaluate_detections(detections, annotations, num_classes, iou_threshold=0.5, score_threshold=0.05, max_detections=100,
                        box_cols=None):
    """detections: per image (scores [K], labels [K], boxes [K,4] or [K,20]) device tensors, as the models return them;
    annotations: per image a sequence indexed by label of arrays [n, >=4] (what load_annotations gives).
    -> {label: (average precision, number of annotations)} as the reference's evaluate returns it."""
    detections = list(detections)
    if len(detections) != len(annotations):
        raise RuntimeError("evaluate_detections: %d images of detections, %d of annotations" % (len(detections), len(annotations)))
    if not detections:
        return {label: (0, 0) for label in range(num_classes)}
    device = detections[0][0].device
    rows = sum(min(int(d[0].shape[0]), int(max_detections)) for d in detections)
    ev = _Evaluation(annotations, num_classes, device, rows, max_detections)
    for i, (scores, labels, boxes) in enumerate(detections):
        ev.add(i, scores, labels, boxes, score_threshold, box_cols)
    return ev.finish(iou_threshold)


def _get_annotations(generator):
    return [generator.load_annotations(i) for i in range(len(generator))]


def evaluate(generator, retinanet, iou_threshold=0.5, score_threshold=0.05, max_detections=100, save_path=None,
             box_cols=None):
    """csv_eval.py:154-242.  Uses the generator as the reference does: len, num_classes(), generator[i][0] (the image,
    CHW), load_annotations(i)[label], label_to_name.  save_path is accepted and unused, as in the reference."""
    num_classes = generator.num_classes()
    annotations = _get_annotations(generator)
    retinanet.eval()
    device = next(retinanet.parameters()).device
    ev = _Evaluation(annotations, num_classes, device, len(generator) * int(max_detections), max_detections)
    with torch.no_grad():
        for index in range(len(generator)):
            data = generator[index]
            scores, labels, boxes = retinanet(data[0].to(device).float().unsqueeze(dim=0))       # :92
            ev.add(index, scores, labels, boxes, score_threshold, box_cols)
            print('{}/{}'.format(index + 1, len(generator)), end='\r')
    average_precisions = ev.finish(iou_threshold)
    print('\nmAP:')
    for label in range(num_classes):
        print('{}: {}'.format(generator.label_to_name(label), average_precisions[label][0]))
    return average_precisions

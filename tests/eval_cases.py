"""Detector validation (csv_eval.evaluate): a plain numpy restatement with its intermediates, the inputs of the golden
cases, and deterministic edge cases with hand-computed expectations.

``restated`` follows the reference operation for operation (retinanet/csv_eval.py: selection :102-123, matching
:189-213 with compute_overlap :21-35, AP :216-235 with _compute_ap :38-62) with two decisions the reference leaves
open or gets wrong, as INTEGRATION.md states them: every sort is STABLE (equal scores keep dataset order: image
ascending, then selected rank; inside an image the lower index first; -0.0 == +0.0), and the box is four named columns
of the detection rows.  It returns what the device path is compared with exactly: the selected rows, the TP flag of
every row, the (class, score descending) order, the annotation counts -- and the AP, summed with np.sum as the
reference does.

The keyword switches of ``restated`` are MUTATIONS, each a plausible misreading of the reference; the host test shows
that each one is caught by a named edge case, so a device kernel with the same misreading cannot pass."""
import numpy as np

EPS = np.finfo(np.float64).eps
MAX_K = 1 << 20                       # ops.EVAL_MAX_K
OK, TOO_MANY, BAD_LABEL, TABLE_FULL = 0, 1, 2, 4


def overlap(d, ann):
    """One detection box d [4] against annotations ann [n,4], fp64, the operations of compute_overlap in its order."""
    d = np.asarray(d, np.float64)
    ann = np.asarray(ann, np.float64)
    area = (ann[:, 2] - ann[:, 0]) * (ann[:, 3] - ann[:, 1])
    iw = np.minimum(d[2], ann[:, 2]) - np.maximum(d[0], ann[:, 0])
    ih = np.minimum(d[3], ann[:, 3]) - np.maximum(d[1], ann[:, 1])
    iw = np.maximum(iw, 0)
    ih = np.maximum(ih, 0)
    ua = (d[2] - d[0]) * (d[3] - d[1]) + area - iw * ih
    ua = np.maximum(ua, EPS)
    return (iw * ih) / ua


def _a4(x):
    """The first four columns of an annotation array [m, >=4] (or an empty one of any shape) as float64 [m,4]."""
    x = np.asarray(x, np.float64)
    return x.reshape(-1, x.shape[-1] if x.ndim == 2 and x.size else 4)[:, :4]


def select(scores, score_threshold=0.05, max_detections=100, score_ge=False, ties="stable"):
    """Indices of the kept detections of one image in selected order."""
    scores = np.asarray(scores, np.float32)
    thr = np.float32(score_threshold)
    with np.errstate(invalid="ignore"):
        keep = np.where(scores >= thr if score_ge else scores > thr)[0]
    s = scores[keep]
    if ties == "higher":                                   # mutation: the higher index first among equal scores
        o = np.argsort(-s[::-1], kind="stable")
        o = (len(s) - 1 - o)
    else:
        o = np.argsort(-s, kind="stable")
    return keep[o[:max_detections]]


def ap_from_flags(tp_sorted, num_annotations, envelope=True):
    """:225-235 and _compute_ap from the TP flags in sorted order."""
    tp_sorted = np.asarray(tp_sorted, np.float64)
    tps = np.cumsum(tp_sorted)
    fps = np.cumsum(1.0 - tp_sorted)
    recall = tps / num_annotations
    precision = tps / np.maximum(tps + fps, EPS)
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([0.0], precision, [0.0]))
    if envelope:
        for i in range(mpre.size - 1, 0, -1):
            mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def restated(dets, anns, num_classes, iou_threshold=0.5, score_threshold=0.05, max_detections=100, box_cols=(0, 4), *,
             table_rows=None, iou_gt=False, score_ge=False, next_best_free=False, argmax_last=False, ties="stable",
             envelope=True, count_detected_only=False):
    """dets: per image (scores [K], labels [K], boxes [K,n]); anns: per image, per class an array [m, >=4].
    -> dict(rows int32 [D,8] as the device table holds them, img_rows [I,2], tp uint8 [D], order int32 [D],
    num_annotations int64 [C], ap float64 [C], tp_count int64 [C], status)."""
    C, I = num_classes, len(dets)
    c0 = box_cols[0]
    f_rows, i_rows, img_rows, status = [], [], np.zeros((I, 2), np.int32), OK
    for im, (scores, labels, boxes) in enumerate(dets):
        scores = np.asarray(scores, np.float32).reshape(-1)
        labels = np.asarray(labels, np.int64).reshape(-1)
        cur = len(f_rows)
        img_rows[im] = (cur, cur)
        if len(scores) > MAX_K:
            status |= TOO_MANY
            continue
        boxes = np.asarray(boxes, np.float32).reshape(len(scores), -1) if len(scores) else np.zeros((0, c0 + 4), np.float32)
        sel = select(scores, score_threshold, max_detections, score_ge, ties)
        if np.any((labels[sel] < 0) | (labels[sel] >= C)):
            status |= BAD_LABEL
            continue
        if table_rows is not None and cur + len(sel) > table_rows:
            status |= TABLE_FULL
            continue
        for k in sel:
            f_rows.append(np.concatenate((boxes[k, c0:c0 + 4], scores[k:k + 1])).astype(np.float32))
            i_rows.append((labels[k], im, k))
        img_rows[im] = (cur, len(f_rows))
    D = len(f_rows)
    fr = np.asarray(f_rows, np.float32).reshape(D, 5)
    ir = np.asarray(i_rows, np.int32).reshape(D, 3)
    rows = np.concatenate((fr.view(np.int32), ir), axis=1)
    tp = np.zeros(D, np.uint8)
    num_ann = np.zeros(C, np.int64)
    for im in range(I):
        b, e = img_rows[im]
        for c in range(C):
            a = _a4(anns[im][c])
            has_det = bool(np.any(ir[b:e, 0] == c))
            if not count_detected_only or has_det:
                num_ann[c] += len(a)
            taken = []
            for r in range(b, e):
                if ir[r, 0] != c or len(a) == 0:
                    continue                                                  # no annotations: a false positive (:198-201)
                with np.errstate(invalid="ignore"):
                    ov = overlap(fr[r, :4], a)
                j = int(np.argmax(ov)) if not argmax_last else len(ov) - 1 - int(np.argmax(ov[::-1]))
                if next_best_free and j in taken:
                    free = [q for q in range(len(a)) if q not in taken]
                    if free:
                        j = free[int(np.argmax(ov[free]))]
                good = ov[j] > iou_threshold if iou_gt else ov[j] >= iou_threshold
                if good and j not in taken:
                    tp[r] = 1
                    taken.append(j)
    order, ap, tp_count = [], np.zeros(C, np.float64), np.zeros(C, np.int64)
    for c in range(C):
        rc = np.where(ir[:, 0] == c)[0]
        s = fr[rc, 4]
        if ties == "higher":
            o = len(s) - 1 - np.argsort(-s[::-1], kind="stable")
        else:
            o = np.argsort(-s, kind="stable")
        order.append(rc[o])
        tp_count[c] = int(tp[rc].sum())
        if num_ann[c] > 0:
            ap[c] = ap_from_flags(tp[rc[o]], float(num_ann[c]), envelope)
    order = np.concatenate(order).astype(np.int32) if order else np.zeros(0, np.int32)
    return dict(rows=rows, img_rows=img_rows, tp=tp, order=order, num_annotations=num_ann, ap=ap, tp_count=tp_count,
                status=status)


def ap_bound(tp_count):
    """The AP tolerance: T * 2^-52 absolute, at least 2^-52 (two summation orders of T identical non-negative terms
    whose sum is <= 1 differ by at most 2 (T - 1) 2^-53)."""
    return np.maximum(np.asarray(tp_count, np.float64), 1.0) * 2.0 ** -52


# ------------------------------------------------------------------------------------------------ golden inputs
GOLDEN = {"a": dict(seed=11, images=40, classes=3, iou=0.5, score=0.05, max_det=100),
          "b": dict(seed=12, images=40, classes=8, iou=0.5, score=0.05, max_det=20),
          "c": dict(seed=13, images=30, classes=5, iou=0.75, score=0.3, max_det=100)}


def golden_inputs(name):
    """-> (dets, anns): per image 20..100 detections -- jittered copies of the annotations plus clutter -- with scores
    UNIQUE over the whole case (a permutation over 4096), so the reference's unstable argsorts have one answer."""
    g = GOLDEN[name]
    rng = np.random.RandomState(g["seed"])
    I, C = g["images"], g["classes"]
    counts = rng.randint(20, 101, size=I)                  # at most 40 x 100 = 4000 < 4095 scores
    perm = rng.permutation(4095)[:int(counts.sum())] + 1
    all_scores = (perm.astype(np.float64) / 4096.0).astype(np.float32)
    dets, anns, at = [], [], 0
    for i in range(I):
        per = []
        for c in range(C):
            n = rng.randint(0, 7)
            xy = rng.uniform(0, 400, size=(n, 2))
            wh = rng.uniform(15, 120, size=(n, 2))
            per.append(np.concatenate((xy, xy + wh), axis=1))
        anns.append(per)
        K = int(counts[i])
        boxes, labels = np.zeros((K, 4), np.float32), np.zeros(K, np.int64)
        for k in range(K):
            c = rng.randint(0, C)
            labels[k] = c
            if len(per[c]) and rng.rand() < 0.7:
                a = per[c][rng.randint(0, len(per[c]))]
                boxes[k] = a + rng.normal(0, 0.12, size=4) * np.tile(a[2:] - a[:2], 2)
            else:
                xy = rng.uniform(0, 400, size=2)
                boxes[k] = np.concatenate((xy, xy + rng.uniform(15, 120, size=2)))
        dets.append((all_scores[at:at + K].copy(), labels, boxes))
        at += K
    return dets, anns


def pack_golden(dets, anns, C):
    """The arrays tests/golden/csv_eval.npz stores per case."""
    off = np.cumsum([0] + [len(d[0]) for d in dets]).astype(np.int32)
    ab, ao = pack_annotations(anns, C)
    return dict(det_scores=np.concatenate([d[0] for d in dets]).astype(np.float32),
                det_labels=np.concatenate([d[1] for d in dets]).astype(np.int64),
                det_boxes=np.concatenate([d[2] for d in dets]).astype(np.float32), det_offsets=off, ann_box=ab, ann_offsets=ao)


def unpack_golden(g, name):
    """(dets, anns, C, params) of a stored case."""
    off, ao, ab = g[name + "_det_offsets"], g[name + "_ann_offsets"], g[name + "_ann_box"]
    I, C = len(off) - 1, len(g[name + "_ap"])
    dets = [(g[name + "_det_scores"][off[i]:off[i + 1]], g[name + "_det_labels"][off[i]:off[i + 1]],
             g[name + "_det_boxes"][off[i]:off[i + 1]]) for i in range(I)]
    anns = [[ab[ao[i * C + c]:ao[i * C + c + 1]] for c in range(C)] for i in range(I)]
    iou, score, max_det = g[name + "_params"]
    return dets, anns, C, dict(iou_threshold=float(iou), score_threshold=float(score), max_detections=int(max_det))


def pack_annotations(anns, C):
    """-> (ann_box float64 [M,4], ann_offsets int32 [I*C+1]) in (image, class) order."""
    boxes, off = [], [0]
    for per in anns:
        for c in range(C):
            a = _a4(per[c])
            boxes.append(a)
            off.append(off[-1] + len(a))
    return (np.concatenate(boxes).reshape(-1, 4) if boxes else np.zeros((0, 4))), np.asarray(off, np.int32)


# ------------------------------------------------------------------------------------------------ edge cases
def _det(rows):
    """rows: (score, label, box) -> (scores, labels, boxes)."""
    if not rows:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 4), np.float32)
    return (np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int64),
            np.array([r[2] for r in rows], np.float32))


def _ann(C, **per_class):
    return [np.array(per_class.get("c%d" % c, []), np.float64).reshape(-1, 4) for c in range(C)]


def _row_annotations(n):
    """n annotations 8 x 8 in a row, 10 apart."""
    j = np.arange(n, dtype=np.float64)
    return np.stack((10 * j, 0 * j, 10 * j + 8, 0 * j + 8), axis=1)


def edge_cases():
    """name -> dict(dets, anns, C, kw (arguments of restated), tp (expected flags in table order), ap, num_annotations),
    every expectation computed by hand in the comments."""
    nan = float("nan")
    s05 = float(np.float32(0.05))
    E = {}
    # [0,0,2,2] against [0,0,2,1]: intersection 2, union 4 + 2 - 2 = 4, IoU exactly 0.5 -> >= holds: a true positive
    E["iou_at_threshold"] = dict(dets=[_det([(0.9, 0, [0, 0, 2, 2])])], anns=[_ann(1, c0=[[0, 0, 2, 1]])], C=1,
                                 tp=[1], ap=[1.0], num_annotations=[1])
    # a score equal to float32(0.05) is not above it: only the 0.5 detection is kept; 1 of 2 annotations found at precision 1
    E["score_at_threshold"] = dict(dets=[_det([(s05, 0, [0, 0, 4, 4]), (0.5, 0, [10, 0, 14, 4])])],
                                   anns=[_ann(1, c0=[[0, 0, 4, 4], [10, 0, 14, 4]])], C=1, tp=[1], ap=[0.5], num_annotations=[2])
    # the second detection's best annotation (0.9 against 0.889) is taken: false positive although the other one is free
    E["best_taken_free_clears"] = dict(dets=[_det([(0.9, 0, [0, 0, 10, 10]), (0.8, 0, [0, 0, 10, 9])])],
                                       anns=[_ann(1, c0=[[0, 0, 10, 10], [0, 0, 10, 8]])], C=1, tp=[1, 0], ap=[0.5], num_annotations=[2])
    # [1,0,5,4] overlaps both annotations by 12 / 20: the first is assigned; [0,0,4,4] then finds the first taken
    E["equal_overlap"] = dict(dets=[_det([(0.9, 0, [1, 0, 5, 4]), (0.8, 0, [0, 0, 4, 4])])],
                              anns=[_ann(1, c0=[[0, 0, 4, 4], [2, 0, 6, 4]])], C=1, tp=[1, 0], ap=[0.5], num_annotations=[2])
    # two detections on one annotation: TP then FP; recall 1 at precision 1
    E["two_on_one"] = dict(dets=[_det([(0.9, 0, [0, 0, 4, 4]), (0.8, 0, [0, 0, 4, 4])])], anns=[_ann(1, c0=[[0, 0, 4, 4]])],
                           C=1, tp=[1, 0], ap=[1.0], num_annotations=[1])
    # zero areas: union 0 is clamped to eps, overlap 0 / eps = 0, never NaN: a false positive
    E["zero_area"] = dict(dets=[_det([(0.9, 0, [1, 1, 1, 1]), (0.8, 0, [0, 0, 4, 4])])], anns=[_ann(1, c0=[[1, 1, 1, 1]])],
                          C=1, tp=[0, 0], ap=[0.0], num_annotations=[1])
    # a NaN coordinate: the overlap is NaN, the detection a false positive that takes nothing; the next one matches.
    # FP, TP with one annotation: recall 0, 1; precision 0, 1/2; envelope 1/2: AP = 1 * 1/2
    E["nan_box"] = dict(dets=[_det([(0.9, 0, [0, nan, 4, 4]), (0.8, 0, [0, 0, 4, 4])])], anns=[_ann(1, c0=[[0, 0, 4, 4]])],
                        C=1, tp=[0, 1], ap=[0.5], num_annotations=[1])
    # FP, TP, TP with two annotations: precision 0, 1/2, 2/3 -> envelope 2/3 everywhere: AP = 1/2 * 2/3 + 1/2 * 2/3
    # (without the envelope: 1/2 * 1/2 + 1/2 * 2/3)
    E["envelope"] = dict(dets=[_det([(0.9, 0, [50, 50, 60, 60]), (0.8, 0, [0, 0, 4, 4]), (0.7, 0, [10, 0, 14, 4])])],
                         anns=[_ann(1, c0=[[0, 0, 4, 4], [10, 0, 14, 4]])], C=1, tp=[0, 1, 1],
                         ap=[0.5 * (2.0 / 3.0) + 0.5 * (2.0 / 3.0)], num_annotations=[2])
    # equal scores everywhere.  Image 0: three detections, max_detections 2 keeps index 0 and 1 (both clutter), the
    # matching index 2 is cut.  Image 1: a match.  Dataset order: FP, FP, TP -> precision 1/3 at recall 1/2 (2 annotations)
    E["ties"] = dict(dets=[_det([(0.5, 0, [50, 50, 60, 60]), (0.5, 0, [70, 50, 80, 60]), (0.5, 0, [0, 0, 4, 4])]),
                           _det([(0.5, 0, [0, 0, 4, 4])])],
                     anns=[_ann(1, c0=[[0, 0, 4, 4]]), _ann(1, c0=[[0, 0, 4, 4]])], C=1, kw=dict(max_detections=2),
                     tp=[0, 0, 1], ap=[0.5 * (1.0 / 3.0)], num_annotations=[2])
    # image 0 has an annotation and no detection: it still counts.  1 of 2 found at precision 1
    E["count_all_images"] = dict(dets=[_det([]), _det([(0.9, 0, [0, 0, 4, 4])])],
                                 anns=[_ann(1, c0=[[0, 0, 4, 4]]), _ann(1, c0=[[0, 0, 4, 4]])], C=1, tp=[1], ap=[0.5], num_annotations=[2])
    # class 0: a match.  class 1: detections and no annotation anywhere -> (0, 0).  class 2: annotations and no detection
    # -> (0.0, 2).  class 0's detection in image 1 meets an image without class-0 annotations: a false positive
    E["empty_classes"] = dict(dets=[_det([(0.9, 0, [0, 0, 4, 4]), (0.8, 1, [0, 0, 4, 4])]), _det([(0.7, 0, [0, 0, 4, 4])])],
                              anns=[_ann(3, c0=[[0, 0, 4, 4]], c2=[[0, 0, 4, 4]]), _ann(3, c2=[[0, 0, 4, 4]])], C=3,
                              tp=[1, 0, 0], ap=[1.0, 0.0, 0.0], num_annotations=[1, 0, 2])
    # signed zeros above a negative threshold are one score: kept in index order, the first three
    E["signed_zeros"] = dict(dets=[_det([(0.0, 0, [50, 50, 60, 60]), (-0.0, 0, [0, 0, 4, 4]), (-0.0, 0, [70, 50, 80, 60]),
                                         (0.0, 0, [10, 0, 14, 4]), (-1.0, 0, [20, 0, 24, 4])])],
                             anns=[_ann(1, c0=[[0, 0, 4, 4], [10, 0, 14, 4]])], C=1, kw=dict(score_threshold=-0.5, max_detections=3),
                             tp=[0, 1, 0], ap=[0.5 * 0.5], num_annotations=[2])
    # groups of 1, 64, 65 and 200 annotations (one image each): the LAST annotation is matched, then matched again, then
    # the first one: TP, FP, TP (for one annotation the third detection repeats the first: TP, FP, FP)
    for n in (1, 64, 65, 200):
        a = _row_annotations(n)
        E["group_%d" % n] = dict(dets=[_det([(0.9, 0, a[-1]), (0.8, 0, a[-1]), (0.7, 0, a[0])])], anns=[[a]], C=1,
                                 tp=[1, 0, 1] if n > 1 else [1, 0, 0],
                                 ap=[1.0 / n * 1.0 + (2.0 / n - 1.0 / n) * (2.0 / 3.0)] if n > 1 else [1.0], num_annotations=[n])
    for c in E.values():
        c.setdefault("kw", {})
    return E


# mutation (a keyword of restated) -> the edge case that catches it
MUTATIONS = {"iou_gt": (dict(iou_gt=True), "iou_at_threshold"),
             "score_ge": (dict(score_ge=True), "score_at_threshold"),
             "next_best_free": (dict(next_best_free=True), "best_taken_free_clears"),
             "argmax_last": (dict(argmax_last=True), "equal_overlap"),
             "ties_higher": (dict(ties="higher"), "ties"),
             "ties_higher_zeros": (dict(ties="higher"), "signed_zeros"),
             "no_envelope": (dict(envelope=False), "envelope"),
             "count_detected_only": (dict(count_detected_only=True), "count_all_images")}

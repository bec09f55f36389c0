"""3D validation (retinanet_mi355x/eval3d.py, csrc/eval_cuboid.hip): a plain Python / numpy restatement with its
intermediates, the same geometry in exact rational arithmetic, closed-form scenes and the fuzz set.

``restated`` follows the definitions operation for operation: Python floats are IEEE doubles with one rounding per
operation, which is what the kernels compute with contraction off.  Selection, table and sorted order come from
eval_cases.restated (the 2D envelope in columns 16:20 is the table's box, as csv_eval uses it); the AP comes from
eval_cases.ap_from_flags.  Per pair: the points sorted by (x, y) (stable), exact duplicates dropped, the monotone chain in
which a cross product <= 0 pops, Sutherland-Hodgman clipping of the detection's hull by the edges of the annotation's (on
the edge is inside, a 17th vertex is dropped), shoelace areas in vertex order, the intersection clipped to
[0, min(area_a, area_b)], iou = inter / max(area_a + area_b - inter, eps).

The keyword switches of ``restated`` are MUTATIONS, each a plausible misreading; tests/test_eval3d_host.py shows that
each one is caught by a named scene.  ``exact_iou`` runs the very same geometry code on fractions.Fraction."""
import math
from fractions import Fraction

import numpy as np

import eval_cases as ec

EPS = float(np.finfo(np.float64).eps)
MAX_VERTS = 16                                            # ops.EVAL_CUBOID_MAX_VERTS
SUBSETS = {"silhouette": (0, 8), "base": (0, 4), "top": (4, 8)}
REVERSED = [3, 2, 1, 0, 7, 6, 5, 4]                       # the detection turned by 180 degrees
TERMS = ("iou", "corner_px", "corner_rel", "corner_px_reversed")
SUMS = ("tp", "iou", "corner_px", "corner_rel", "reversed")

# The largest |restated - exact| overlap over the fuzz set (fuzz_pairs(), 3000 pairs), measured on 2026-10-20 with
#   python -c "import sys; sys.path[:0] = ['tests']; import eval3d_cases as e; print(e.measure_fuzz())"
# (no pair was within it of 0.5 or 0.7).  The tests hold restated to 8 x this: the set is finite and slivers lose more digits.
FUZZ_MAX_ERROR = 6.662430180270501e-15
FUZZ_BOUND = 8.0 * FUZZ_MAX_ERROR


# ------------------------------------------------------------------------------------------------ geometry (float or Fraction)
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(points, keep_collinear=False, keep_interior=False, keep_duplicates=False):
    """points: (x, y) tuples -> the hull's vertices, counter-clockwise for x right, y up; fewer than 3 when degenerate."""
    pts = sorted(points, key=lambda p: (p[0], p[1]))                          # stable; -0.0 == 0.0
    if not keep_duplicates:
        uniq = []
        for p in pts:
            if not uniq or not (p[0] == uniq[-1][0] and p[1] == uniq[-1][1]):
                uniq.append(p)
        pts = uniq
    n = len(pts)
    if n < 3:
        return pts

    def pops(c):
        if keep_interior:
            return False
        return c < 0 if keep_collinear else c <= 0
    h = []
    for p in pts:
        while len(h) >= 2 and pops(_cross(h[-2], h[-1], p)):
            h.pop()
        h.append(p)
    t = len(h) + 1
    for p in pts[-2::-1]:
        while len(h) >= t and pops(_cross(h[-2], h[-1], p)):
            h.pop()
        h.append(p)
    return h[:-1]


def area(poly, zero):
    s = zero
    for i in range(1, len(poly) - 1):                                         # the fan from vertex 0: small differences, not coordinates
        s = s + _cross(poly[0], poly[i], poly[i + 1])
    return s / 2 if isinstance(s, Fraction) else 0.5 * s


def clip(poly, c1, c2):
    out = []

    def emit(p):
        if len(out) < MAX_VERTS:
            out.append(p)
    s = poly[-1]
    ds = _cross(c1, c2, s)
    for e in poly:
        de = _cross(c1, c2, e)
        if (ds < 0) if de >= 0 else (ds >= 0):
            t = ds / (ds - de)
            emit((s[0] + t * (e[0] - s[0]), s[1] + t * (e[1] - s[1])))
        if de >= 0:
            emit(e)
        s, ds = e, de
    return out


def pair_iou(det, ann, exact=False, **hull_kw):
    """det, ann: sequences of (x, y) as floats (numpy scalars are fine).  -> (iou, vertices of det's hull)."""
    det = [(float(x), float(y)) for x, y in det]
    ann = [(float(x), float(y)) for x, y in ann]
    finite = all(math.isfinite(v) for p in det + ann for v in p)
    if not finite:
        return (Fraction(0) if exact else 0.0), 0
    zero, eps = (Fraction(0), Fraction(EPS)) if exact else (0.0, EPS)
    if exact:
        det = [(Fraction(x), Fraction(y)) for x, y in det]
        ann = [(Fraction(x), Fraction(y)) for x, y in ann]
    hb = hull(ann, **hull_kw)
    ha = hull(det, **hull_kw)
    if len(hb) < 3 or len(ha) < 3:
        return zero, len(ha)
    area_b, area_a = area(hb, zero), area(ha, zero)
    poly = ha
    for e in range(len(hb)):
        if not poly:
            break
        poly = clip(poly, hb[e], hb[e + 1] if e + 1 < len(hb) else hb[0])
    inter = area(poly, zero) if len(poly) >= 3 else zero
    lim = area_a if area_a < area_b else area_b
    if not inter >= 0:
        inter = zero
    if inter > lim:
        inter = lim
    ua = (area_a + area_b) - inter
    ua = ua if ua > eps else eps
    iou = inter / ua
    return (iou if iou == iou else zero), len(ha)


def exact_iou(det, ann):
    """The overlap in rational arithmetic on the very same fp32 / fp64 inputs."""
    return pair_iou(det, ann, exact=True)[0]


def _points(row16, overlap):
    a, b = SUBSETS[overlap]
    return [(row16[2 * k], row16[2 * k + 1]) for k in range(a, b)]


def corner_terms(det16, ann, swap_reversed=False, diag_from_box=False):
    """(corner_px, corner_px / diag, corner_px of the turned detection) of a detection's fp32 corners and an annotation row."""
    d = [float(v) for v in det16]
    b = [float(v) for v in ann[:16]]
    fwd = rev = 0.0
    x0 = x1 = b[0]
    y0 = y1 = b[1]
    for k in range(8):
        kr = REVERSED[k]
        dx, dy = d[2 * k] - b[2 * k], d[2 * k + 1] - b[2 * k + 1]
        ex, ey = d[2 * kr] - b[2 * k], d[2 * kr + 1] - b[2 * k + 1]
        fwd += math.sqrt(dx * dx + dy * dy)
        rev += math.sqrt(ex * ex + ey * ey)
        x0, x1 = min(x0, b[2 * k]), max(x1, b[2 * k])
        y0, y1 = min(y0, b[2 * k + 1]), max(y1, b[2 * k + 1])
    if diag_from_box:
        x0, y0, x1, y1 = (float(v) for v in ann[16:20])
    w, h = x1 - x0, y1 - y0
    diag = math.sqrt(w * w + h * h)
    diag = diag if diag > EPS else EPS
    if swap_reversed:
        fwd, rev = rev, fwd
    px = fwd / 8.0
    return px, px / diag, rev / 8.0


# ------------------------------------------------------------------------------------------------ the whole evaluation
def split_by_class(labels, C):
    """labels: per image an array [n, >=21] -> per image, per class the rows of that class in label order (padding dropped)."""
    out = []
    for a in labels:
        a = np.asarray(a, np.float64).reshape(-1, np.asarray(a).shape[-1] if np.asarray(a).size else 21)
        out.append([a[a[:, 20] == c] for c in range(C)])
    return out


def pack_labels(labels, C):
    """-> (ann_corners float64 [M,16], ann_offsets int32 [I*C+1]) in (image, class) order."""
    rows, off = [], [0]
    for per in split_by_class(labels, C):
        for c in range(C):
            rows.append(per[c][:, :16])
            off.append(off[-1] + len(per[c]))
    return (np.ascontiguousarray(np.concatenate(rows).reshape(-1, 16)) if rows else np.zeros((0, 16))), np.asarray(off, np.int32)


def restated(dets, labels, C, overlap="silhouette", iou_thresholds=(0.5, 0.7), score_threshold=0.05, max_detections=100, *,
             table_rows=None, iou_gt=False, argmax_last=False, next_best_free=False, keep_collinear=False, keep_interior=False,
             keep_duplicates=False, swap_reversed=False, diag_from_box=False):
    """dets: per image (scores [K], labels [K], boxes [K,20]); labels: per image an array [n, >=21].
    -> dict(rows, img_rows, status, order (eval_cases.restated's), corners f32 [D,16], best_iou f64 [D], best_ann i32 [D],
    n_hull [D] (vertices of the detection's hull), tp u8 [T,D], matched i32 [D], num_annotations i64 [C], ap f64 [T,C],
    tp_count i64 [T,C], terms f64 [D,4], sums f64 [C,5])."""
    I, T = len(dets), len(iou_thresholds)
    hull_kw = dict(keep_collinear=keep_collinear, keep_interior=keep_interior, keep_duplicates=keep_duplicates)
    base = ec.restated(dets, [[np.zeros((0, 4))] * C] * I, C, score_threshold=score_threshold, max_detections=max_detections,
                       box_cols=(16, 20), table_rows=table_rows)
    rows, img_rows = base["rows"], base["img_rows"]
    D = len(rows)
    corners = np.zeros((D, 16), np.float32)
    for r in range(D):
        corners[r] = np.asarray(dets[rows[r, 6]][2], np.float32).reshape(-1, 20)[rows[r, 7], :16]
    per = split_by_class(labels, C)
    best_iou, best_ann = np.zeros(D, np.float64), np.full(D, -1, np.int32)
    n_hull = np.zeros(D, np.int32)
    tp, matched = np.zeros((T, D), np.uint8), np.full(D, -1, np.int32)
    terms = np.zeros((D, 4), np.float64)
    num_ann = np.zeros(C, np.int64)
    for im in range(I):
        b, e = img_rows[im]
        for c in range(C):
            anns = per[im][c]
            num_ann[c] += len(anns)
            mine = [r for r in range(b, e) if rows[r, 5] == c]
            ovs = {}
            for r in mine:
                if len(anns) == 0:
                    continue
                ov = []
                for a in anns:
                    v, n_hull[r] = pair_iou(_points(corners[r], overlap), _points(a, overlap), **hull_kw)
                    ov.append(v)
                ov = np.asarray(ov, np.float64)
                j = int(np.argmax(ov)) if not argmax_last else len(ov) - 1 - int(np.argmax(ov[::-1]))
                best_iou[r], best_ann[r], ovs[r] = ov[j], j, ov
            for t, thr in enumerate(iou_thresholds):
                taken = []
                for r in mine:
                    if len(anns) == 0:
                        continue
                    j, ov = int(best_ann[r]), ovs[r]
                    if next_best_free and j in taken:
                        free = [q for q in range(len(anns)) if q not in taken]
                        if free:
                            j = free[int(np.argmax(ov[free]))]
                    good = ov[j] > thr if iou_gt else ov[j] >= thr
                    if good and j not in taken:
                        tp[t, r] = 1
                        taken.append(j)
                        if t == 0:
                            matched[r] = j
                            px, rel, rev = corner_terms(corners[r], anns[j], swap_reversed, diag_from_box)
                            terms[r] = (ov[j], px, rel, rev)
    sums = np.zeros((C, 5), np.float64)
    for c in range(C):
        acc = [0.0] * 5
        for r in range(D):                                                    # table order, one addition at a time
            if rows[r, 5] == c and tp[0, r]:
                acc[0] += 1.0
                acc[1] += float(terms[r, 0])
                acc[2] += float(terms[r, 1])
                acc[3] += float(terms[r, 2])
                acc[4] += 1.0 if terms[r, 3] < terms[r, 1] else 0.0
        sums[c] = acc
    order = base["order"]
    ap, tp_count = np.zeros((T, C), np.float64), np.zeros((T, C), np.int64)
    for t in range(T):
        for c in range(C):
            oc = order[rows[order, 5] == c]
            tp_count[t, c] = int(tp[t, oc].sum())
            if num_ann[c] > 0:
                ap[t, c] = ec.ap_from_flags(tp[t, oc], float(num_ann[c]))
    return dict(rows=rows, img_rows=img_rows, status=base["status"], order=order, corners=corners, best_iou=best_iou,
                best_ann=best_ann, n_hull=n_hull, tp=tp, matched=matched, num_annotations=num_ann, ap=ap, tp_count=tp_count,
                terms=terms, sums=sums)


def summary(res, iou_thresholds):
    """What eval3d.evaluate_cuboids returns, from restated's arrays."""
    C = len(res["num_annotations"])
    out = {"ap": {}, "mAP": {}, "errors": {}}
    for t, thr in enumerate(iou_thresholds):
        n = res["num_annotations"]
        out["ap"][float(thr)] = {c: ((float(res["ap"][t, c]), float(n[c])) if n[c] else (0, 0)) for c in range(C)}
        have = [float(res["ap"][t, c]) for c in range(C) if n[c]]
        out["mAP"][float(thr)] = sum(have) / len(have) if have else 0.0
    for c in range(C):
        s = res["sums"][c]
        n = float(s[0])
        out["errors"][c] = {"tp": int(n), "iou": float(s[1]) / n if n else 0.0, "corner_px": float(s[2]) / n if n else 0.0,
                            "corner_rel": float(s[3]) / n if n else 0.0, "reversed": int(s[4])}
    return out


# ------------------------------------------------------------------------------------------------ scenes
def rect(x0, y0, x1, y1):
    """A cuboid whose top equals its base: the rectangle's corners, in label order fbl fbr bbl bbr (twice)."""
    q = [x0, y1, x1, y1, x0, y0, x1, y0]
    return q + q


def points8(pts):
    return [v for p in pts for v in p]


def label(corners16, cls=0, box=None):
    c = np.asarray(corners16, np.float64)
    if box is None:
        box = [c[0::2].min(), c[1::2].min(), c[0::2].max(), c[1::2].max()]
    return np.concatenate((c, np.asarray(box, np.float64), [float(cls)]))


def det_rows(rows):
    """rows: (score, label, corners16) -> (scores, labels, boxes [K,20]) with the corner envelope in columns 16:20."""
    if not rows:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 20), np.float32)
    boxes = np.zeros((len(rows), 20), np.float32)
    for i, r in enumerate(rows):
        c = np.asarray(r[2], np.float32)
        boxes[i, :16] = c
        with np.errstate(invalid="ignore"):
            boxes[i, 16:] = (np.nanmin(c[0::2]), np.nanmin(c[1::2]), np.nanmax(c[0::2]), np.nanmax(c[1::2]))
    return np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int64), boxes


def labels_of(*rows):
    return np.stack(rows) if rows else np.zeros((0, 21))


# fbl fbr bbl bbr ftl ftr btl btr: the base (0,6) (4,6) (2,4) (6,4), the top 4 higher.  The silhouette is the hexagon
# (0,6) (4,6) (6,4) (6,0) (2,0) (0,2) -- the 6 x 6 square less two corner triangles of area 2: 32 -- with bbl (2,4) and
# ftr (4,2) inside it
HEXAGON = points8([(0, 6), (4, 6), (2, 4), (6, 4), (0, 2), (4, 2), (2, 0), (6, 0)])


def scenes():
    """name -> dict(dets, labels, C, kw, best_iou, best_ann, tp (rows of flags per threshold (0.5, 0.7) unless kw says
    otherwise), and optionally n_hull, sums), every expectation computed by hand in the comments."""
    nan, inf = float("nan"), float("inf")
    S = {}
    # two 4 x 4 squares offset by (2, 2): intersection 2 x 2 = 4, union 16 + 16 - 4 = 28
    S["squares_offset"] = dict(dets=[det_rows([(0.9, 0, rect(2, 2, 6, 6))])], labels=[labels_of(label(rect(0, 0, 4, 4)))],
                               best_iou=[4.0 / 28.0], best_ann=[0], tp=[[0], [0]])
    # a square and the diamond through its edge midpoints: the diamond lies inside, 8 / 16 = 0.5 exactly: >= holds at 0.5
    diamond = points8([(2, 0), (4, 2), (2, 4), (0, 2)] * 2)
    S["square_diamond"] = dict(dets=[det_rows([(0.9, 0, diamond)])], labels=[labels_of(label(rect(0, 0, 4, 4)))],
                               best_iou=[0.5], best_ann=[0], tp=[[1], [0]], n_hull=[4])
    S["identical"] = dict(dets=[det_rows([(0.9, 0, HEXAGON)])], labels=[labels_of(label(HEXAGON))], best_iou=[1.0], best_ann=[0],
                          tp=[[1], [1]], n_hull=[6], sums=[[1.0, 1.0, 0.0, 0.0, 0.0]])
    # squares sharing the edge x = 4: the clipped polygon has no area
    S["edge_touching"] = dict(dets=[det_rows([(0.9, 0, rect(4, 0, 8, 4))])], labels=[labels_of(label(rect(0, 0, 4, 4)))],
                              best_iou=[0.0], best_ann=[0], tp=[[0], [0]])
    # [1,3]^2 inside [0,4]^2: 4 / 16; and the other way round
    S["contained"] = dict(dets=[det_rows([(0.9, 0, rect(1, 1, 3, 3)), (0.8, 0, rect(-2, -2, 6, 6))])],
                          labels=[labels_of(label(rect(0, 0, 4, 4)))], best_iou=[0.25, 0.25], best_ann=[0, 0], tp=[[0, 0], [0, 0]])
    # the hexagon inside the 6 x 6 square: 32 / 36; with the interior corners kept the chain is no hexagon
    S["hexagon"] = dict(dets=[det_rows([(0.9, 0, HEXAGON)])], labels=[labels_of(label(rect(0, 0, 6, 6)))], best_iou=[32.0 / 36.0],
                        best_ann=[0], tp=[[1], [1]], n_hull=[6])
    # the square's corners and its edge midpoints: the midpoints are collinear with a hull edge and go
    mids = points8([(0, 0), (2, 0), (4, 0), (4, 4), (2, 4), (0, 4), (0, 2), (4, 2)])
    S["collinear_triples"] = dict(dets=[det_rows([(0.9, 0, mids)])], labels=[labels_of(label(rect(0, 0, 4, 4)))], best_iou=[1.0],
                                  best_ann=[0], tp=[[1], [1]], n_hull=[4])
    S["all_equal"] = dict(dets=[det_rows([(0.9, 0, points8([(3, 3)] * 8))])], labels=[labels_of(label(rect(0, 0, 4, 4)))],
                          best_iou=[0.0], best_ann=[0], tp=[[0], [0]], n_hull=[1])
    S["all_collinear"] = dict(dets=[det_rows([(0.9, 0, points8([(k, 2 * k) for k in range(8)]))])],
                              labels=[labels_of(label(rect(0, 0, 4, 4)))], best_iou=[0.0], best_ann=[0], tp=[[0], [0]], n_hull=[2])
    # a NaN / an infinite corner in the detection (images 0, 1) and in the annotation (images 2, 3): overlap 0
    bad_n, bad_i = rect(0, 0, 4, 4), rect(0, 0, 4, 4)
    bad_n[5], bad_i[8] = nan, inf
    good = rect(0, 0, 4, 4)
    S["non_finite"] = dict(dets=[det_rows([(0.9, 0, bad_n)]), det_rows([(0.9, 0, bad_i)]), det_rows([(0.9, 0, good)]),
                                 det_rows([(0.9, 0, good)])],
                           labels=[labels_of(label(good)), labels_of(label(good)), labels_of(label(bad_n, box=[0, 0, 4, 4])),
                                   labels_of(label(bad_i, box=[0, 0, 4, 4]))],
                           best_iou=[0.0] * 4, best_ann=[0] * 4, tp=[[0] * 4, [0] * 4])
    # two identical annotations: the lower index is the candidate of both detections; the second finds it taken
    S["identical_annotations"] = dict(dets=[det_rows([(0.9, 0, rect(0, 0, 4, 4)), (0.8, 0, rect(0, 0, 4, 4))])],
                                      labels=[labels_of(label(rect(0, 0, 4, 4)), label(rect(0, 0, 4, 4)))], best_iou=[1.0, 1.0],
                                      best_ann=[0, 0], tp=[[1, 0], [1, 0]])
    # the second detection's best annotation (0.9 against 80 / 90) is taken: a false positive though the other is free
    S["best_taken_other_free"] = dict(dets=[det_rows([(0.9, 0, rect(0, 0, 10, 10)), (0.8, 0, rect(0, 0, 10, 9))])],
                                      labels=[labels_of(label(rect(0, 0, 10, 10)), label(rect(0, 0, 10, 8)))], best_iou=[1.0, 0.9],
                                      best_ann=[0, 0], tp=[[1, 0], [1, 0]])
    # the annotation with its corners renamed by the half turn: the same silhouette, every corner far from its namesake
    turned = [HEXAGON[2 * k + d] for k in REVERSED for d in (0, 1)]
    S["reversed"] = dict(dets=[det_rows([(0.9, 0, turned)])], labels=[labels_of(label(HEXAGON))], best_iou=[1.0], best_ann=[0],
                         tp=[[1], [1]], reversed=[1])
    # the hexagon moved by (1, 0): every corner is 1 px off; the envelope of the corners is 6 x 6, columns 16:20 say 3 x 4
    moved = [v + (1 if k % 2 == 0 else 0) for k, v in enumerate(HEXAGON)]
    S["moved"] = dict(dets=[det_rows([(0.9, 0, moved)])], labels=[labels_of(label(HEXAGON, box=[0, 0, 3, 4]))], best_ann=[0],
                      tp=[[1], [0]], corner_px=[1.0], corner_rel=[1.0 / math.sqrt(72.0)], reversed=[0])
    for s in S.values():
        s.setdefault("C", 1)
        s.setdefault("kw", {})
    return S


# mutation (keywords of restated) -> (the scene that catches it, the result it shows in)
MUTATIONS = {"iou_gt": (dict(iou_gt=True), "square_diamond", "tp"),
             "argmax_last": (dict(argmax_last=True), "identical_annotations", "best_ann"),
             "next_best_free": (dict(next_best_free=True), "best_taken_other_free", "tp"),
             "keep_collinear": (dict(keep_collinear=True), "collinear_triples", "n_hull"),
             "keep_interior": (dict(keep_interior=True), "hexagon", "best_iou"),
             "keep_duplicates": (dict(keep_duplicates=True), "all_equal", "n_hull"),
             "swap_reversed": (dict(swap_reversed=True), "reversed", "sums"),
             "diag_from_box": (dict(diag_from_box=True), "moved", "sums")}


# ------------------------------------------------------------------------------------------------ fuzz
def cuboid(x0, y0, w, h):
    """The affine corner pattern of the synthetic labels (synth.labels_dir): the base, and the top half a height above."""
    base = [(x0, y0 + h), (x0 + .6 * w, y0 + .9 * h), (x0 + .4 * w, y0 + .6 * h), (x0 + w, y0 + .5 * h)]
    return points8(base + [(x, y - .5 * h) for x, y in base])


def fuzz_pairs(n=3000, seed=2024, rectangles=False):
    """-> (det float32 [n,16], ann float64 [n,16]): projected cuboids in a 1920 x 1080 frame, the detection jittered by
    0.5, 3, 10 or 40 px per coordinate; one in ten identical up to fp32 rounding, one in seventeen disjoint.
    rectangles: top equals base and the base is an axis-aligned rectangle (the silhouette is the 2D box)."""
    rng = np.random.RandomState(seed)
    det, ann = np.zeros((n, 16), np.float32), np.zeros((n, 16), np.float64)
    for i in range(n):
        w, h = rng.uniform(20, 400), rng.uniform(20, 300)
        x0, y0 = rng.uniform(0, 1920 - w), rng.uniform(0, 1080 - h)
        a = np.asarray(rect(x0, y0, x0 + w, y0 + h) if rectangles else cuboid(x0, y0, w, h), np.float64)
        sigma = (0.5, 3.0, 10.0, 40.0)[i % 4]
        if rectangles:
            j = rng.normal(0, sigma, 4)
            d = np.asarray(rect(x0 + j[0], y0 + j[1], x0 + w + j[2], y0 + h + j[3]), np.float64)
        else:
            d = a + rng.normal(0, sigma, 16)
        if i % 10 == 3:
            d = a.copy()
        if i % 17 == 5:
            d = d + 3000.0
        ann[i], det[i] = a, d.astype(np.float32)
    return det, ann


def measure_fuzz(overlap="silhouette"):
    """(max |restated - exact|, pairs within that of 0.5 or 0.7) over the fuzz set."""
    det, ann = fuzz_pairs()
    worst, vals = 0.0, []
    for d, a in zip(det, ann):
        v = pair_iou(_points(d, overlap), _points(a, overlap))[0]
        x = exact_iou(_points(d, overlap), _points(a, overlap))
        worst = max(worst, abs(float(Fraction(v) - x)))
        vals.append((v, x))
    near = sum(1 for v, x in vals if min(abs(x - Fraction(0.5)), abs(x - Fraction(0.7))) <= worst)
    return worst, near

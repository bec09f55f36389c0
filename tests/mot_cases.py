"""Tracking evaluation (mot_evaluator.MOT_Evaluator.evaluate): a CPU restatement with its intermediates, builders for
CSV rows, the synthetic edge cases and the stability rule of the end-to-end comparison.

``restated`` follows the reference's evaluate (mot_evaluator.py:120-412) step by step on numpy arrays; scipy solves the
assignment, as in the reference.  Arithmetic widths, established against the imported reference (the host test holds the
restatement to the golden bit for bit):
  transforms        as oracle/homography.py: projections fp64, states and space corners fp32
  refined heights   fp64 (height_from_template divides fp64 image heights by the fp32 guess), fed back as fp64
  footprints        fp32 min / max of the four bottom space corners
  IoU               every step fp32 -- ``a`` is a row of an fp32 tensor, ``b`` an fp32 numpy row, Python's max / min pick
                    one operand (``y if y > x else x``: a NaN second operand is dropped), 1e-06 rounds to fp32 in the
                    sum, the quotient is fp32 -- a true division when the intersection is a tensor, reciprocal times
                    numerator (Tensor.__rtruediv__) when it is a numpy scalar, which is when the prediction lies strictly
                    inside the ground truth on both axes -- and the result widens to the fp64 matrix exactly
  state_err         fp32 |pred - gt| clamped to [0, 500], 7 columns
  im_bot / im_top   fp64: mean over 4 corners of sqrt(dx^2 + dy^2), clamped to [0, 500]
  figures           Match / Pre-threshold IOU: population deviation in fp64 (np.mean / np.std); the state columns: sample
                    deviation in fp32 (torch.mean / torch.std of an fp32 stack); the image errors: sample deviation in fp64

``fixed_sums`` is the summation order the device uses for every figure (fp64, two passes), so that the device can be
held to it bit for bit; ``figures`` turns the sums into the (mean, deviation) pairs.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

from oracle import homography as ohg

LANES = 256                                   # partial sums of fixed_sums (the block size of rn_mot_reduce)
MOT_MAX = 512                                 # ops.MOT_MAX / RN_MOT_MAX
CLASS_NAMES = ["sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer"]
CLASS_DICT = {n: i for i, n in enumerate(CLASS_NAMES)}
CLASS_DICT["truck"] = 5
N_CLASSES = len(ohg.CLASS_HEIGHTS)            # the confusion matrix is [10,10] (mot_evaluator.py:50-51)
STATE_COLS = [39, 40, 43, 42, 44, 35, 38]
FIGURES = [("Pre-threshold IOU", "pre"), ("Match IOU", "match"), ("Width precision", 3), ("Height precision", 4),
           ("Length precision", 2), ("Velocity precision", 6), ("X precision", 0), ("Y precision", 1),
           ("Bottom im precision", "bot"), ("Top im precision", "top")]


# ------------------------------------------------------------------------------------------------ rows
def gt_row(frame, obj_id, cls, corners, vel=""):
    """A 45-column ground-truth row: image corners [8,2] in columns 11:27, velocity (may be "") in column 38."""
    r = [""] * 45
    r[0], r[2], r[3] = str(frame), str(obj_id), cls
    r[11:27] = [repr(float(v)) for v in np.asarray(corners, np.float64).reshape(16)]
    r[38] = vel if isinstance(vel, str) else repr(float(vel))
    return r


def pred_row(frame, obj_id, cls, state, with_height=True):
    """A prediction row from state (x, y, l, w, h, direction, velocity); with_height=False gives the 44-column form."""
    r = [""] * 45
    r[0], r[2], r[3] = str(frame), str(obj_id), cls
    for c, v in zip(STATE_COLS, state):
        r[c] = repr(float(v))
    return r if with_height else r[:44]


def box_corners(x, y, l, w, h, direction=1.0):
    """Image corners [8,2] of a state under SYN_H / SYN_P (image = space x, y + z): exact for dyadic values."""
    sp = ohg.state_to_space(np.array([[x, y, l, w, h, direction]], np.float32))[0].astype(np.float64)
    return np.stack((sp[:, 0], sp[:, 1] + sp[:, 2]), 1)


SYN_H = np.eye(3)
SYN_P = np.array([[1.0, 0, 0, 0], [0, 1.0, 1.0, 0], [0, 0, 0, 1.0]])


# ------------------------------------------------------------------------------------------------ pieces
def iou_matrix(first, second):
    """self.iou for every pair (mot_evaluator.py:87-118, 219-222) -> [n,m] fp64 holding fp32 values."""
    a = np.asarray(first, np.float32)[:, None, :]
    b = np.asarray(second, np.float32)[None, :, :]
    one = np.float32(1e-06)
    with np.errstate(all="ignore"):
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        minx = np.where(b[..., 0] > a[..., 0], b[..., 0], a[..., 0])          # max(a, b): b only if b > a
        maxx = np.where(b[..., 2] < a[..., 2], b[..., 2], a[..., 2])          # min(a, b): b only if b < a
        miny = np.where(b[..., 1] > a[..., 1], b[..., 1], a[..., 1])
        maxy = np.where(b[..., 3] < a[..., 3], b[..., 3], a[..., 3])
        dx, dy = maxx - minx, maxy - miny
        inter = np.where(dx > 0, dx, np.float32(0)) * np.where(dy > 0, dy, np.float32(0))
        union = ((area_a + area_b) - inter) + one
        # the quotient: a tensor numerator divides; a numpy one (both extents came from b, the prediction strictly inside the
        # ground truth on both axes) meets Tensor.__rtruediv__, which is reciprocal() * numerator -- two roundings
        inside = (b[..., 0] > a[..., 0]) & (b[..., 2] < a[..., 2]) & (b[..., 1] > a[..., 1]) & (b[..., 3] < a[..., 3])
        out = np.where(inside, (np.float32(1) / union) * inter, inter / union)
    assert out.dtype == np.float32
    return out.astype(np.float64)


def footprint(space):
    s = np.asarray(space, np.float32)
    return np.stack((s[:, 0:4, 0].min(1), s[:, 0:4, 1].min(1), s[:, 0:4, 0].max(1), s[:, 0:4, 1].max(1)), 1)


def prepare_gt(rows, H, P):
    """-> (state7 fp32 [n,7], footprint fp32 [n,4], image corners fp64 [n,8,2], ids, class strings)."""
    im = np.stack([np.array(r[11:27]).astype(float) for r in rows]).reshape(-1, 8, 2)
    classes = [r[3] for r in rows]
    vel = np.array([float(r[38]) if len(r[38]) > 0 else 0 for r in rows], np.float64).astype(np.float32)
    h0 = ohg.guess_heights(classes)
    with np.errstate(all="ignore"):
        st = ohg.im_to_state(im, H, h0)
        repro = ohg.state_to_im(st, P)
        h1 = ohg.height_from_template(repro, h0, im)                          # fp64
        st = ohg.im_to_state(im, H, h1)
    return (np.concatenate((st, vel[:, None]), 1), footprint(ohg.state_to_space(st)), im, [int(r[2]) for r in rows],
            classes)


def prepare_pred(rows, P):
    """-> (state7 fp32 [m,7], footprint fp32 [m,4], image corners fp64 [m,8,2], ids, class strings)."""
    st = []
    for r in rows:
        r = list(r) + [2] if len(r) == 44 else r
        st.append(np.array([r[c] for c in STATE_COLS]).astype(float))
    st = np.stack(st).reshape(-1, 7).astype(np.float32)
    with np.errstate(all="ignore"):
        return st, footprint(ohg.state_to_space(st)), ohg.state_to_im(st, P), [int(r[2]) for r in rows], [r[3] for r in rows]


def clamp500(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, 0, np.where(x > 500, 500, x)).astype(x.dtype)


def corner_err(p, g):
    """mean over 4 corners of the distance, fp64, summed in corner order."""
    d = p - g
    e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return clamp500(np.float64((((e[0] + e[1]) + e[2]) + e[3]) / 4.0))


def confusion_cell(gt_cls, pred_cls):
    """mot_evaluator.py:314-325: an unknown gt class gives row 5 and carries ITS string into the second lookup."""
    if gt_cls not in CLASS_DICT:
        return 5, 5
    return CLASS_DICT[gt_cls], CLASS_DICT.get(pred_cls, 5)


def fixed_sums(values, valid=None):
    """(count, sum, sum of squared deviations from sum / count) of the valid entries, fp64, in the device's order: entry k
    goes to partial k % LANES, each partial accumulates in increasing k, the partials add in increasing order; an
    invalid entry adds +0.0 in both passes."""
    v = np.asarray(values, np.float64)
    ok = np.ones(len(v), bool) if valid is None else np.asarray(valid, bool)
    n = int(ok.sum())
    pad = (-len(v)) % LANES

    def ordered(x):
        x = np.concatenate((x, np.zeros(pad))).reshape(-1, LANES)
        part = np.zeros(LANES)
        for row in x:
            part = part + row
        s = 0.0
        for p in part:
            s = s + p
        return float(s)
    with np.errstate(all="ignore"):
        s1 = ordered(np.where(ok, v, 0.0))
        mean = np.float64(s1) / np.float64(n)
        d = v - mean
        s2 = ordered(np.where(ok, d * d, 0.0))
    return n, s1, s2


def figures(sums):
    """{key: (n, s1, s2)} -> {name: (mean, deviation)} as fp64; population deviation for the two IoU lists, sample
    deviation for the rest."""
    out = {}
    with np.errstate(all="ignore"):
        for name, key in FIGURES:
            n, s1, s2 = sums[key]
            dof = n if key in ("pre", "match") else n - 1
            out[name] = (float(np.float64(s1) / np.float64(n)), float(np.sqrt(np.float64(s2) / np.float64(dof))))
    return out


# ------------------------------------------------------------------------------------------------ the evaluation
def restated(gt, pred, H, P, match_iou=0, cutoff_frame=10000, ious=None):
    """gt / pred: {frame: [row, ...]}.  ious: {frame: matrix} replaces the computed matrices (the staged comparison).
    -> dict: the integer metrics, confusion, the run-length id lists, per assigned pair (frame, gt row, pred column, IoU,
    matched), per match the error vectors, the fixed-order sums and the figures."""
    H, P = np.asarray(H, np.float64), np.asarray(P, np.float64)
    m = dict(TP=0, FP=0, FN=0, edge=0, FP02=0, FN02=0)
    conf = np.zeros((N_CLASSES, N_CLASSES), np.int64)
    ids, gt_ids, pred_ids = {}, [], []
    pairs, state_err, bot_err, top_err, frames_iou = [], [], [], [], {}
    for f in sorted((set(gt) | set(pred))):
        if not (0 <= f < cutoff_frame):
            continue
        if f not in gt:
            m["FP"] += len(pred[f])
            for r in pred[f]:
                if int(r[2]) not in pred_ids:
                    pred_ids.append(int(r[2]))
            continue
        if f not in pred:
            m["FN"] += len(gt[f])
            for r in gt[f]:
                if int(r[2]) not in gt_ids:
                    gt_ids.append(int(r[2]))
            continue
        g_state, g_box, g_im, g_id, g_cls = prepare_gt(gt[f], H, P)
        p_state, p_box, p_im, p_id, p_cls = prepare_pred(pred[f], P)
        mat = iou_matrix(g_box, p_box) if ious is None else np.asarray(ious[f], np.float64)
        frames_iou[f] = mat
        a, b = linear_sum_assignment(mat, maximize=True)
        matches = []
        for i, j in zip(a, b):
            ok = bool(mat[i, j] >= match_iou)
            pairs.append((f, int(i), int(j), mat[i, j], ok))
            if ok:
                matches.append((int(i), int(j)))
        for j in range(len(p_im)):
            if j not in b:
                x0, y0, x2, y2 = p_im[j, 0, 0], p_im[j, 0, 1], p_im[j, 2, 0], p_im[j, 2, 1]
                if x0 < 0 or x2 < 0 or x0 > 1920 or x2 > 1920 or y0 < 0 or y2 < 0 or y0 > 1080 or y2 > 1080:
                    m["edge"] += 1
        m["TP"] += len(matches)
        m["FP"] += max(0, len(p_state) - len(matches))
        m["FN"] += max(0, len(g_state) - len(matches))
        m["FP02"] += max(0, len(p_state) - len(a))
        m["FN02"] += max(0, len(g_state) - len(a))
        for i, j in matches:
            with np.errstate(invalid="ignore"):
                state_err.append(clamp500(np.abs(p_state[j] - g_state[i])))
                bot_err.append(corner_err(p_im[j, 0:4], g_im[i, 0:4]))
                top_err.append(corner_err(p_im[j, 4:8], g_im[i, 4:8]))
            conf[confusion_cell(g_cls[i], p_cls[j])] += 1
            if g_id[i] not in ids:
                ids[g_id[i]] = [p_id[j]]
            elif ids[g_id[i]][-1] != p_id[j]:
                ids[g_id[i]].append(p_id[j])
            if p_id[j] not in pred_ids:
                pred_ids.append(p_id[j])
            if g_id[i] not in gt_ids:
                gt_ids.append(g_id[i])
    frag = sum(len(v) - 1 for v in ids.values())
    switches = 0
    for pid in pred_ids:
        c = sum(1 for v in ids.values() if pid in v)
        switches += max(0, c - 1)
    TP, FP, FN = m["TP"], m["FP"], m["FN"]
    metrics = {"iou_threshold": match_iou, "True unique objects": len(gt_ids), "Predicted unique objects": len(pred_ids),
               "TP": TP, "FP": FP, "FN": FN, "FP edge-case": m["edge"], "FP @ 0.2": m["FP02"], "FN @ 0.2": m["FN02"]}
    metrics["Recall"] = TP / (TP + FN)                                           # ZeroDivisionError as in the reference
    metrics["Precision"] = TP / (TP + FP)
    metrics["False Alarm Rate"] = FP / TP
    metrics["Fragmentations"] = frag
    metrics["ID switches"] = switches
    metrics["MOTA"] = 1 - (FN + frag + switches + FP) / TP
    metrics["MOTA edge-case"] = 1 - (FN + frag + switches + FP - m["edge"]) / TP
    metrics["MOTA @ 0.2"] = 1 - (m["FN02"] + frag + switches + m["FP02"]) / TP
    pre = np.array([p[3] for p in pairs], np.float64)
    ok = np.array([p[4] for p in pairs], bool)
    se = np.stack(state_err).astype(np.float32).reshape(-1, 7)
    bot, top = np.array(bot_err, np.float64), np.array(top_err, np.float64)
    sums = {"pre": fixed_sums(pre), "match": fixed_sums(pre, ok), "bot": fixed_sums(bot), "top": fixed_sums(top)}
    for c in range(7):
        sums[c] = fixed_sums(se[:, c])
    return dict(metrics=metrics, confusion=conf, ids=ids, gt_ids=gt_ids, pred_ids=pred_ids,
                pair_frame=np.array([p[0] for p in pairs], np.int64), pair_gt=np.array([p[1] for p in pairs], np.int64),
                pair_pred=np.array([p[2] for p in pairs], np.int64), pair_iou=pre, pair_ok=ok, state_err=se, bot_err=bot,
                top_err=top, sums=sums, figures=figures(sums), ious=frames_iou)


# ------------------------------------------------------------------------------------------------ stability
def stable_frame(mat, match_iou, eps):
    """True if no perturbation of the entries by up to +-16 eps can change the assignment or a threshold decision.
    Decided from the reference's matrix alone: the assignment a is optimal with value V; any other assignment scores at
    most the second-best value V2, and perturbing moves each of the min(n,m) terms of both by at most d = 16 eps, so a is
    still the unique optimum if V - V2 > 2 min(n,m) d.  V2 is found exactly by forbidding each assigned pair in turn."""
    d = 16.0 * eps
    a, b = linear_sum_assignment(mat, maximize=True)
    if d == 0.0:
        return True                                          # identical matrices: the same solver gives the same answer
    if np.any(np.abs(mat[a, b] - match_iou) <= d):
        return False
    k = len(a)
    if mat.shape[0] == 1 and mat.shape[1] == 1:
        return True
    V = mat[a, b].sum()
    big = -1e6
    for i, j in zip(a, b):
        alt = mat.copy()
        alt[i, j] = big
        a2, b2 = linear_sum_assignment(alt, maximize=True)
        if V - alt[a2, b2].sum() <= 2 * k * d:
            return False
    return True


def unstable_frames(ious, match_iou, eps):
    return sorted(f for f, mat in ious.items() if not stable_frame(mat, match_iou, eps))


# ------------------------------------------------------------------------------------------------ synthetic cases
def _veh(frame, gid, pid, x, y, l=16.0, w=6.0, h=4.0, cls="sedan", pcls=None, vel=8.0, dx=0.0, dy=0.0, pvel=None,
         with_height=True):
    """A ground-truth box and a prediction shifted by (dx, dy): dyadic values only."""
    g = gt_row(frame, gid, cls, box_corners(x, y, l, w, h), vel)
    p = pred_row(frame, pid, cls if pcls is None else pcls, (x + dx, y + dy, l, w, h, 1.0, (8.0 if isinstance(vel, str) else vel) if pvel is None else pvel),
                 with_height)
    return g, p


def _add(d, f, row):
    d.setdefault(f, []).append(row)


def _grid(frame, n_gt, n_pred, gt, pred, seed=0, tie=False):
    """n_gt ground-truth boxes on a grid and n_pred predictions over (some of) them with dyadic offsets, ids permuted."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(max(n_gt, n_pred))
    for i in range(n_gt):
        x, y = 32.0 * (i % 32), 16.0 * (i // 32)
        _add(gt, frame, gt_row(frame, i, CLASS_NAMES[i % 8], box_corners(x, y, 16.0, 6.0, 4.0), float(i % 5)))
    for j in range(n_pred):
        i = int(perm[j])
        x, y = 32.0 * (i % 32), 16.0 * (i // 32)
        dx = 0.0 if tie else float(rng.randint(0, 8)) * 0.5
        _add(pred, frame, pred_row(frame, 1000 + j, CLASS_NAMES[(i + (j % 3 == 0)) % 8],
                                   (x + dx, y + float(rng.randint(0, 4)) * 0.25, 16.0, 6.0, 4.0 + (j % 2), 1.0, float(j % 7))))


def synthetic_cases():
    """name -> (gt, pred, match_iou, cutoff_frame).  SYN_H / SYN_P and dyadic coordinates: no transform rounds."""
    cases = {}
    # frames only in gt / only in pred / in neither, around a 1 x 1 frame
    gt, pred = {}, {}
    g, p = _veh(0, 1, 11, 64.0, 8.0, dx=2.0)
    _add(gt, 0, g), _add(pred, 0, p)
    _add(gt, 1, _veh(1, 2, 0, 0.0, 8.0)[0]), _add(gt, 1, _veh(1, 1, 0, 64.0, 8.0)[0])
    _add(pred, 3, _veh(3, 0, 11, 64.0, 8.0)[1]), _add(pred, 3, _veh(3, 0, 12, 0.0, 8.0)[1])
    cases["missing_frames"] = (gt, pred, 0, 10)
    for name, (n, k) in {"3x5": (3, 5), "5x3": (5, 3), "65x70": (65, 70), "70x65": (70, 65)}.items():
        gt, pred = {}, {}
        _grid(0, n, k, gt, pred, seed=n)
        cases[name] = (gt, pred, 0.51, 10)
    # all-zero IoU: predictions far from every ground truth; every assigned pair is a match at 0 and none at 0.51
    gt, pred = {}, {}
    for i in range(3):
        _add(gt, 0, gt_row(0, i, "van", box_corners(32.0 * i, 8.0, 16.0, 6.0, 4.0), 1.0))
    for j in range(4):
        _add(pred, 0, pred_row(0, 50 + j, "van", (32.0 * j, 256.0, 16.0, 6.0, 4.0, 1.0, 1.0)))
    g, p = _veh(1, 9, 59, 0.0, 8.0)
    _add(gt, 1, g), _add(pred, 1, p)                                  # one true match so that TP > 0 at 0.51
    cases["zero_iou_0"] = (gt, pred, 0, 10)
    cases["zero_iou_51"] = (gt, pred, 0.51, 10)
    # tied IoUs: two identical predictions over each ground truth, and identical ground truths
    gt, pred = {}, {}
    _grid(0, 6, 9, gt, pred, seed=3, tie=True)
    for j in range(4):
        _add(pred, 0, pred_row(0, 2000 + j, "sedan", (0.0, 0.0, 16.0, 6.0, 4.0, 1.0, 0.0)))
    _add(gt, 0, gt_row(0, 77, "sedan", box_corners(0.0, 0.0, 16.0, 6.0, 4.0), 0.0))
    cases["ties"] = (gt, pred, 0, 10)
    # 44-column prediction rows, empty velocity, unknown classes (gt unknown then known; pred unknown)
    gt, pred = {}, {}
    g, p = _veh(0, 1, 11, 0.0, 8.0, h=2.0, cls="spaceship", pcls="van", vel="", with_height=False)
    _add(gt, 0, g), _add(pred, 0, p)
    g, p = _veh(0, 2, 12, 64.0, 8.0, h=2.0, cls="pickup", pcls="hovercraft", with_height=False, dx=1.0, pvel=600.0)
    _add(gt, 0, g), _add(pred, 0, p)
    g, p = _veh(0, 3, 13, 128.0, 8.0, h=2.0, cls="truck", pcls="semi", with_height=False, dy=0.5)
    _add(gt, 0, g), _add(pred, 0, p)
    cases["rows_and_classes"] = (gt, pred, 0.51, 10)
    # ids: pred 11 matched to gt 1 and gt 2 (one switch); gt 3 matched to 21, 22, 21 (two fragmentations)
    gt, pred = {}, {}
    for f, (p1, p3) in enumerate([(11, 21), (12, 22), (12, 22), (12, 21)]):
        for gid, pid, x in ((1, p1, 0.0), (3, p3, 128.0)):
            g, p = _veh(f, gid, pid, x, 8.0, dx=0.5 * f)
            _add(gt, f, g), _add(pred, f, p)
    for f in (4, 5):
        g, p = _veh(f, 2, 11, 64.0, 8.0)
        _add(gt, f, g), _add(pred, f, p)
    g, p = _veh(5, 2, 11, 256.0, 8.0)                                  # the same ids twice in one frame
    _add(gt, 5, g), _add(pred, 5, p)
    cases["ids"] = (gt, pred, 0.51, 10)
    # outside the frame: unassigned (counted), assigned below the threshold (not counted), and the elif branch (y)
    gt, pred = {}, {}
    g, p = _veh(0, 1, 11, 64.0, 64.0)
    _add(gt, 0, g), _add(pred, 0, p)
    _add(gt, 0, gt_row(0, 2, "sedan", box_corners(1800.0, 64.0, 16.0, 6.0, 4.0), 0.0))
    _add(pred, 0, pred_row(0, 12, "sedan", (1912.0, 64.0, 16.0, 6.0, 4.0, 1.0, 0.0)))      # x > 1920, assigned at IoU 0
    _add(pred, 0, pred_row(0, 13, "sedan", (-64.0, 512.0, 16.0, 6.0, 4.0, 1.0, 0.0)))      # x < 0, unassigned
    _add(pred, 0, pred_row(0, 14, "sedan", (512.0, 1100.0, 16.0, 6.0, 4.0, 1.0, 0.0)))     # y > 1080, unassigned
    _add(pred, 0, pred_row(0, 15, "sedan", (-8.0, -8.0, 16.0, 6.0, 4.0, 1.0, 0.0)))        # both: counted once
    _add(pred, 0, pred_row(0, 16, "sedan", (512.0, 512.0, 16.0, 6.0, 4.0, 1.0, 0.0)))      # inside, unassigned
    cases["edge_case"] = (gt, pred, 0.51, 10)
    # one frame at the size limit
    gt, pred = {}, {}
    _grid(0, MOT_MAX, MOT_MAX, gt, pred, seed=9)
    cases["at_limit"] = (gt, pred, 0.51, 10)
    # 300 frames of 2 x 2, ids drifting, a cutoff that drops the tail
    gt, pred = {}, {}
    for f in range(300):
        for k in range(2):
            g, p = _veh(f, k + 2 * (f // 100), 10 + k + (f // 7) % 3, 64.0 * k, 8.0, dx=0.25 * (f % 8), pvel=float(f % 11))
            _add(gt, f, g), _add(pred, f, p)
    cases["frames_300"] = (gt, pred, 0.51, 290)
    return cases


def too_large_case():
    gt, pred = {}, {}
    _grid(0, 2, MOT_MAX + 1, gt, pred, seed=1)
    return gt, pred


def nan_case():
    gt, pred = {}, {}
    g, p = _veh(0, 1, 11, 0.0, 8.0)
    _add(gt, 0, g), _add(pred, 0, p)
    g, p = _veh(1, 1, 11, 0.0, 8.0)
    p[39] = "nan"
    _add(gt, 1, g), _add(pred, 1, p)
    return gt, pred


def no_tp_case():
    gt, pred = {}, {}
    _add(gt, 0, gt_row(0, 1, "sedan", box_corners(0.0, 8.0, 16.0, 6.0, 4.0), 0.0))
    _add(pred, 0, pred_row(0, 2, "sedan", (512.0, 8.0, 16.0, 6.0, 4.0, 1.0, 0.0)))
    return gt, pred, 0.51


def synth_sequence(frames=2000, n=40, seed=0):
    """A seeded sequence for the benchmark: n vehicles per frame moving along x, predictions jittered, ids switching now
    and then.  Same SYN_H / SYN_P."""
    rng = np.random.RandomState(seed)
    gt, pred = {}, {}
    x0 = rng.uniform(0, 1500, n)
    for f in range(frames):
        for k in range(n):
            x, y = x0[k] + 0.5 * f, 12.0 * (k % 8) + 100.0 * (k // 8)
            _add(gt, f, gt_row(f, k, CLASS_NAMES[k % 8], box_corners(x, y, 16.0, 6.0, 4.0), 30.0))
            j = rng.normal(0, 0.7, 4)
            _add(pred, f, pred_row(f, k + 100 * ((f + k) // 500), CLASS_NAMES[(k + (f % 50 == 0)) % 8],
                                   (x + j[0], y + j[1], 16.0 + j[2], 6.0, 4.0 + j[3], 1.0, 30.0 + j[0])))
    return gt, pred

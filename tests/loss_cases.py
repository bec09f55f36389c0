"""Edge cases, a float64 reference and derived error envelopes for the fused loss (focal_kernel and its epilogue in
csrc/focal_loss.hip, reached through ops.focal_loss) and for the matching rule it shares with ops.assign and the need sets
(csrc/anchor_match_dev.h, csrc/anchor_match.hip).  tests/test_loss_cases_host.py proves that the cases reach the code paths
they are named after and pins the reference to oracle/losses.py; tests/test_gpu_loss_edges.py runs the kernels on them,
tests/test_gpu_need_rule.py the need sets.  Nothing here touches a GPU; every input comes from retinanet_mi355x.synth and numpy.

Reference (``reference``): the loss of D/losses.py / R/losses.py with every continuous operation in float64 (torch
autograd on doubles) and every integer decision -- valid rows, IoU bands, first-maximum argmax, ``.long()`` of the class
-- taken by oracle.losses.assign on the float32 inputs, as the kernel and the reference project take them.  The clamp
bounds are the float32 ones widened to double (LO, HI): float32(1e-4) < 1e-4, so a double clamp would zero a gradient
that float32 passes.  The gradient is that of W_LOSS . (cls, reg, vp).

Envelopes
  dcls, per element.  a = p for the positive class of a positive anchor, 1 - p otherwise; the element is
      +-w s h(a),  h(a) = 2 (1-a) ln a - (1-a)^2 / a,  h'(a) = -2 ln a + 4 (1-a)/a + (1-a)^2/a^2.
  Any float32 evaluation rounds a once, which moves the element by the relative amount
      cond = |h'(a)| ulp32(a) / |h(a)|                      (1.2e-3 at p ~ 1e-4 on a negative: h ~ -3 p^2, h' ~ 6 p)
  so the check is |got - ref| <= |ref| (R + cond) where ref != 0 and got == 0 exactly where ref == 0.  R is measured, per
  case, as the float32 oracle's worst excess of relative error over cond (``dcls_excess``); the kernel is allowed
  DCLS_M = 8 times that: v_log_f32 and v_rcp_f32 (~1 ulp each), the ln 2 factor, the gradient scale folded in float32
  and grad_losses are about twice the oracle's roundings, doubled for headroom.
  dreg.  Rows of non-positives are exactly zero.  Per positive row and column group (0:2, 2:8, 8:12 directional; 0:4 2D)
  max|err| / max|ref|; the kernel is allowed DREG_M = 4 times the float32 oracle's worst row of the same case.
  Loss scalars: relative error within LOSS_M = 4 times the float32 oracle's on that case, floor 2^-22.
A case family with several shapes (tail_sizes, many_labels, ...) is one case per variant: its oracle figures are the worst
over its shapes of that variant (``family_figures``), so that a shape with three elements does not set a bound from a
sample of three.  A result that holds a NaN or an infinity fails every comparison (``within``).
"""
import numpy as np
import torch

import golden_cases as gc
from oracle import anchors as oanchors
from oracle import losses as olosses
from retinanet_mi355x import synth

F32, F64 = np.float32, np.float64
LO32, HI32 = F32(1e-4), F32(1.0) - F32(1e-4)           # the kernel's fmed3 bounds: 1e-4f and 1.0f - 1e-4f
LO, HI = float(LO32), float(HI32)
W_LOSS = (1.25, 2.0, 3.0)                               # d total / d (cls, reg, vp): grad_losses of the backward
DCLS_M, DREG_M, LOSS_M, LOSS_FLOOR = 8.0, 4.0, 4.0, 2.0 ** -22
REG_GAP = 1e-4                                          # every positive's distance from e == 0 and from d == 1/9
CENTRE_MIN = 0.025                                      # ... and the least size of its centre gradient / scale (directional)

# geometry of focal_kernel (csrc/focal_loss.hip)
UNIT, NWAVES, QCAP, NTHR, RESIDENT, MAX_GT, MAX_B = 128, 4, 256, 256, 768, 256, 1024

_SL = (-1, -1, +1, +1, -1, -1, +1, +1)                  # corner j = c + sl l + sw w + sh h (D/losses.py:310-327)
_SW = (-1, +1, -1, +1, -1, +1, -1, +1)
_SH = (+1, +1, +1, +1, -1, -1, -1, -1)
_VP_GROUPS = (((2, 3, 6, 7), (0, 1, 4, 5)), ((1, 3, 5, 7), (0, 2, 4, 6)), ((0, 1, 2, 3), (4, 5, 6, 7)))


# ------------------------------------------------------------------------------------------------ kernel geometry
def focal_groups(B, A, resident=RESIDENT):
    """Workgroups per image: focal_groups() of csrc/focal_loss.hip."""
    units = (A + UNIT - 1) // UNIT
    G = (resident // B) & ~7
    if G < 8:
        G = 8
    need = (units + NWAVES - 1) // NWAVES
    if G > need:
        G = ((need + 7) & ~7) if need >= 8 else need
    return max(G, 1)


def wave_units(B, A):
    """{(g, wave): [units it walks, in order]} of one image."""
    G, units = focal_groups(B, A), (A + UNIT - 1) // UNIT
    return {(g, w): list(range(g * NWAVES + w, units, G * NWAVES)) for g in range(G) for w in range(NWAVES)}


def queue_trace(B, A, state):
    """The wave loop of focal_kernel on one image's states [A]: -> (largest queue length reached, number of times a wave
    broke out with the queue past QCAP - UNIT and units left, i.e. drained and re-issued without a primed buffer)."""
    pos = (np.asarray(state) == 1)
    plain = (np.asarray(state) == 0)
    peak = reissues = 0
    for us in wave_units(B, A).values():
        qn = 0
        for k, u in enumerate(us):
            sl = slice(u * UNIT, min((u + 1) * UNIT, A))
            if not plain[sl].all():                     # a plain unit takes the fast path and queues nothing
                qn += int(pos[sl].sum())
            peak = max(peak, qn)
            if qn > QCAP - UNIT:
                reissues += k + 1 < len(us)
                qn = 0
    return peak, reissues


# ------------------------------------------------------------------------------------------------ cases
class Case(object):
    """cls [B,A,C], reg [B,A,12|4], anchors [1,A,4], ann [B,N,27|5]: float32 CPU tensors."""

    def __init__(self, name, directional, cls, reg, anchors, ann, **extra):
        self.name, self.directional = name, bool(directional)
        self.cls, self.reg, self.anchors, self.ann = cls.contiguous(), reg.contiguous(), anchors.contiguous(), ann.contiguous()
        self.__dict__.update(extra)
        self.memo = {}
        B, A, C = self.cls.shape
        assert self.anchors.shape == (1, A, 4) and self.reg.shape == (B, A, 12 if directional else 4)
        assert self.ann.shape[0] == B and self.ann.shape[2] == (27 if directional else 5)

    @property
    def B(self):
        return self.cls.shape[0]

    @property
    def A(self):
        return self.cls.shape[1]

    @property
    def C(self):
        return self.cls.shape[2]

    @property
    def N(self):
        return self.ann.shape[1]

    def __repr__(self):
        return self.name


def _memo(fn):
    def wrapped(case):
        if fn.__name__ not in case.memo:
            case.memo[fn.__name__] = fn(case)
        return case.memo[fn.__name__]
    wrapped.__name__ = fn.__name__
    return wrapped


def anchor_table(hw):
    return torch.from_numpy(oanchors.anchors_for_image(*hw))[0]


def dir_rows(boxes, classes):
    """[n,27] directional label rows whose corner envelope is exactly ``boxes`` [n,4] (the four box edges appear among the
    corners as given; every other corner coordinate lies strictly inside), laid out as synth.labels_dir."""
    b = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    w, h = x1 - x0, y1 - y0
    xs = (x0, x0 + F32(.6) * w, x0 + F32(.4) * w, x1)
    yb = (y1, y0 + F32(.9) * h, y0 + F32(.6) * h, y0 + F32(.5) * h)
    yt = (y0 + F32(.5) * h, y0 + F32(.4) * h, y0 + F32(.1) * h, y0)
    out = np.zeros((b.shape[0], 27), dtype=F32)
    for k in range(4):
        out[:, 2 * k], out[:, 2 * k + 1] = xs[k], yb[k]
        out[:, 8 + 2 * k], out[:, 9 + 2 * k] = xs[k], yt[k]
    out[:, 16:20] = b
    out[:, 20] = np.asarray(classes, dtype=F32)
    return out


def box_rows(boxes, classes):
    b = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    return np.concatenate((b, np.asarray(classes, dtype=F32).reshape(-1, 1)), 1)


def label_rows(directional, boxes, classes):
    return dir_rows(boxes, classes) if directional else box_rows(boxes, classes)


def cls_col(directional):
    return 20 if directional else 4


def _ann(directional, per_image, N=None):
    """Stack per-image row arrays (or None for an image without labels) into [B,N,cols], padding with invalid rows."""
    cols = 27 if directional else 5
    N = max([0 if r is None else len(r) for r in per_image] + [1]) if N is None else N
    out = -np.ones((len(per_image), N, cols), dtype=F32)
    for j, r in enumerate(per_image):
        if r is not None and len(r):
            out[j, :len(r)] = r
    return torch.from_numpy(out)


def _heads(B, A, C, n_reg, seed, reg_std=0.2):
    """cls = u^6 (reaches below 1e-4 and close to 1: both clamp edges), reg ~ N(0, reg_std)."""
    return synth.scores_portable(B, A, C, seed, power=6), torch.from_numpy(synth.normal((B, A, n_reg), seed + 1, reg_std))


def _finish(case, seed=977):
    """Redraw the regression rows of positives that sit within 2 REG_GAP of e == 0 or of the smooth-L1 kink, or whose
    centre gradient nearly cancels (below 2 CENTRE_MIN)."""
    for it in range(40):
        bad = [(j, idx[(gap < 2 * REG_GAP) | (centre < 2 * CENTRE_MIN)]) for j, idx, gap, centre in positive_gaps(case)]
        n = sum(len(i) for _, i in bad)
        if n == 0:
            return case
        fresh = synth.normal((n, case.reg.shape[2]), seed + 4 * it, 0.2)
        k = 0
        for j, idx in bad:
            case.reg[j, idx] = torch.from_numpy(fresh[k:k + len(idx)])
            k += len(idx)
        case.memo.clear()
    raise AssertionError("regression rows of %s do not settle" % case.name)


# ---- queue_full
QF_X, QF_Y = (100.0, 100.0, 200.0, 180.0), (400.0, 300.0, 520.0, 400.0)
QF_A = 69 * UNIT - 37
QF_SPLIT = 32 * UNIT                                    # anchors below are jittered copies of QF_X, the rest of QF_Y


def _queue_full(directional, B, C):
    A = QF_A
    base = np.where(np.arange(A)[:, None] < QF_SPLIT, np.array(QF_X, F32)[None], np.array(QF_Y, F32)[None])
    anc = (base + synth.uniform((A, 4), 501, -4.0, 4.0)).astype(F32)
    tiny = ((140, 130, 150, 140), (450, 340, 460, 352))
    per = []
    for j in range(B):
        if j == 0:
            rows = label_rows(directional, (QF_X, QF_Y), (1, 2))
        elif j == 1:                                    # the same, behind an invalid row and in the other order
            rows = np.concatenate((-np.ones((1, 27 if directional else 5), F32), label_rows(directional, (QF_Y, QF_X), (0, 3))))
        elif j == 2:
            rows = label_rows(directional, (QF_X,), (2,))          # positives in units 0..31 only
        elif j == 3:
            rows = None                                 # no labels: the raw sum
        elif j == 4:
            rows = label_rows(directional, tiny, (1, 0))            # labels, no positive: npos == 0, clamp(min=1)
        else:                                           # ordinary sparse images: a shifted box, IoU 0.44 .. 0.48 before the jitter
            s = 35.0 + (j % 5)
            bx = (QF_X[0] + s, QF_X[1], QF_X[2] + s, QF_X[3]) if j % 2 else (QF_Y[0], QF_Y[1] + s, QF_Y[2], QF_Y[3] + s)
            rows = label_rows(directional, (bx, tiny[j % 2]), (j % C, (j + 1) % C))
        per.append(rows)
    cls, reg = _heads(B, A, C, 12 if directional else 4, 511 if directional else 521)
    return _finish(Case("queue_full" if directional else "queue_full_2d", directional, cls, reg,
                        torch.from_numpy(anc)[None], _ann(directional, per)))


# ---- tail_sizes
TAIL_A = (1, 63, 64, 65, 127, 128, 129, 511, 513, 3969)
TAIL_HW = {True: (96, 128), False: (136, 168)}         # the 96x128 table has 2313 rows; 3969 = 31*128 + 1 needs the larger one
TAIL_C3 = (1, 129, 3969)


def _tail(A, directional, C):
    table = anchor_table(TAIL_HW[A <= 2313])
    anc = table[:A]
    i0 = 40 if A > 40 else 0

    def shrunk(i, f):                                   # concentric with anchor i, width scaled by f: IoU with it == f
        a = table[i].numpy().astype(F64)
        cx, hw = 0.5 * (a[0] + a[2]), 0.5 * f * (a[2] - a[0])
        return (cx - hw, a[1], cx + hw, a[3])
    boxes0 = [tuple(table[i0].numpy())]
    if i0:
        boxes0.append(shrunk(0, 0.45))                  # anchor 0: IoU 0.45 -> ignored
    boxes0.append(tuple(table[A - 1].numpy()))          # the last anchor (alone in its unit at A = 3969) is positive
    boxes1 = [tuple(table[min(A - 1, 100)].numpy()), shrunk(min(A - 1, 9), 0.47), tuple(table[A // 2].numpy())][::-1]
    per = [label_rows(directional, boxes0, [k % C for k in range(len(boxes0))]),
           label_rows(directional, boxes1, [(k + 1) % C for k in range(len(boxes1))])]
    cls, reg = _heads(2, A, C, 12 if directional else 4, 600 + A + 7 * C + directional)
    return _finish(Case("tail_A%d_%s_C%d" % (A, "dir" if directional else "2d", C), directional, cls, reg, anc[None],
                        _ann(directional, per, N=4)))


# ---- many_labels
ML_N = (1, 63, 64, 65, 128, 256)
ML_HW = (96, 128)


def ml_tie_anchor():
    """A 64x64 anchor of the 96x128 table near the middle of the image: the box of rows 63 and 64."""
    t = anchor_table(ML_HW).numpy()
    ok = np.nonzero((np.abs(t[:, 2] - t[:, 0] - 64) < 0.01) & (np.abs(t[:, 3] - t[:, 1] - 64) < 0.01))[0]
    return int(ok[len(ok) // 2])


def _many_labels(N, directional, C):
    table = anchor_table(ML_HW)
    big = tuple(table[ml_tie_anchor()].numpy())
    seed = 700 + N
    x0, y0 = synth.uniform((N,), seed, 0.0, 100.0), synth.uniform((N,), seed + 1, 0.0, 70.0)
    w, h = synth.uniform((N,), seed + 2, 10.0, 30.0), synth.uniform((N,), seed + 3, 10.0, 30.0)
    boxes = np.stack((x0, y0, x0 + w, y0 + h), 1).astype(F32)
    klass = synth.randint((N,), seed + 4, C).astype(F32)
    r = min(63, N - 1)
    boxes[r] = big
    klass[r] = 2.7                                      # .long() truncates to 2
    if N > 64:                                          # the same box on either side of the register / LDS boundary
        boxes[64] = big
        klass[64] = 3.0
    img0 = label_rows(directional, boxes, klass)
    img1 = label_rows(directional, boxes, klass)
    img1[:N - 1] = -1.0                                 # only row N-1 is valid ...
    img1[N - 1] = label_rows(directional, (big,), (1,))[0]      # ... and it has positives
    out = boxes.copy()
    out[:, 0::2] += 4000.0                              # every row valid, all outside the anchors' window: no positive
    img2 = label_rows(directional, out, klass)
    cls, reg = _heads(3, table.shape[0], C, 12 if directional else 4, 710 + N + directional)
    return _finish(Case("labels_N%d_%s" % (N, "dir" if directional else "2d"), directional, cls, reg, table[None],
                        _ann(directional, (img0, img1, img2), N=N)))


# ---- thresholds
TH_REPS = 60                                            # 60 positives per image: the oracle's worst row is a fair sample
TH_KINDS = ("half", "below_half", "two_fifths", "below_two_fifths")
TH_STATE = {"half": 1, "below_half": -1, "two_fifths": -1, "below_two_fifths": 0}
TH_FILL = 100                                           # ordinary anchors (far away) before and after the special ones


def th_expected_iou(kind):
    half, tf = F32(0.5), F32(2.0) / F32(5.0)
    return {"half": half, "below_half": np.nextafter(half, F32(0)), "two_fifths": tf,
            "below_two_fifths": np.nextafter(tf, F32(0))}[kind]


def _thresholds(directional, C):
    two_minus = np.nextafter(F32(2), F32(0))            # one edge scaled by (1 - 2^-24)
    anc, boxes, kinds = [], [], []
    for rep in range(TH_REPS):
        for k, kind in enumerate(TH_KINDS):
            x = F32(16 * (4 * rep + k))
            anc.append((x, 0, x + 4, 4 if k < 2 else 5))            # area 16 or 20
            boxes.append((x, 0, x + 4, F32(2) if k % 2 == 0 else two_minus))
            kinds.append(kind)
    fill = anchor_table((96, 128))[:2 * TH_FILL].numpy() + np.array([0, 1000, 0, 1000], F32)
    anchors = np.concatenate((fill[:TH_FILL], np.array(anc, F32), fill[TH_FILL:]))
    klass = [i % C for i in range(len(boxes))]
    rows = label_rows(directional, boxes, klass)
    per = [rows, rows[::-1].copy()]
    cls, reg = _heads(2, anchors.shape[0], C, 12 if directional else 4, 800 + directional)
    return _with(_finish(Case("thresholds_%s" % ("dir" if directional else "2d"), directional, cls, reg,
                              torch.from_numpy(anchors)[None], _ann(directional, per))), kinds=kinds, first=TH_FILL)


def _with(case, **extra):
    case.__dict__.update(extra)
    return case


# ---- clamp_edges
def clamp_values():
    z, o = F32(0), F32(1)
    return np.array([LO32, np.nextafter(LO32, z), np.nextafter(LO32, o), HI32, np.nextafter(HI32, z), np.nextafter(HI32, o),
                     z, o], dtype=F32)


CLAMP_WHERE = ("negative", "positive_class", "positive_other", "fast_path")


def _clamp_edges(directional, C):
    H, W = 96, 128
    table = anchor_table((H, W))
    make = synth.labels_dir if directional else synth.labels_2d
    ann = make(2, 6, H, W, num_classes=C, seed=21, size_px=(28, 70))
    cls, reg = _heads(2, table.shape[0], C, 12 if directional else 4, 900 + directional)
    case = Case("clamp_%s" % ("dir" if directional else "2d"), directional, cls, reg, table[None], ann)
    vals, plan = clamp_values(), []
    for j, asg in enumerate(assignment(case)):
        state, cidx = asg[2].numpy(), asg[3].numpy()
        A = len(state)
        unit_plain = np.array([(state[u * UNIT:(u + 1) * UNIT] == 0).all() for u in range((A + UNIT - 1) // UNIT)])
        in_plain = unit_plain[np.arange(A) // UNIT]
        slots = {"negative": [(a, c) for a in np.nonzero((state == 0) & ~in_plain)[0][:4] for c in range(C)],
                 "positive_class": [(a, cidx[a]) for a in np.nonzero(state == 1)[0]],
                 "positive_other": [(a, c) for a in np.nonzero(state == 1)[0] for c in range(C) if c != cidx[a]],
                 "fast_path": [(a, c) for a in np.nonzero(in_plain)[0][5:9] for c in range(C)]}
        for where in CLAMP_WHERE:
            for i, (a, c) in enumerate(slots[where][:2 * len(vals)]):
                case.cls[j, a, c] = float(vals[i % len(vals)])
                plan.append((where, j, int(a), int(c), i % len(vals)))
    case.memo.clear()
    return _with(_finish(case), plan=plan)


# ---- the rest
def _one_image_full_size():
    H, W = 1080, 1920
    A = oanchors.num_anchors(H, W)
    cls, reg = synth.head_outputs(1, A, 8, 12, seed=5)
    return _finish(Case("one_image_1080p", True, cls, reg, anchor_table((H, W))[None], synth.labels_dir(1, 10, H, W, 8, seed=2)))


def _big_batch(directional, B, A, C, hw):
    table = anchor_table(hw)
    per = []
    for j in range(B):
        if j % 3 == 0:
            per.append(None)                            # empty images: vp_images < B
        else:
            i, k = (7 * j) % A, (31 * j + 5) % A
            a = table[k].numpy().astype(F64)
            per.append(label_rows(directional, (tuple(table[i].numpy()), (a[0], a[1], a[0] + 0.46 * (a[2] - a[0]), a[3])),
                                  (j % C, (j + 3) % C)))
    cls, reg = _heads(B, A, C, 12 if directional else 4, 1000 + B + directional)
    return _finish(Case("batch_B%d_A%d_%s" % (B, A, "dir" if directional else "2d"), directional, cls, reg, table[:A][None],
                        _ann(directional, per)))


def _golden(directional):
    ann = gc.loss_labels_dir() if directional else gc.loss_labels_2d()
    cls, reg = gc.loss_heads(12 if directional else 4, 21 if directional else 31)
    return Case("golden_%s" % ("dir" if directional else "2d"), directional, cls, reg, anchor_table(gc.LOSS_HW)[None], ann)


QF2D_B = 49                                             # smallest B with (768 // B) & ~7 <= 8


def _build(name):
    if name == "queue_full":
        return [_queue_full(True, 96, 8)]
    if name == "queue_full_2d":
        return [_queue_full(False, QF2D_B, 4)]
    if name == "tail_sizes":
        out = []
        for A in TAIL_A:
            for directional, C in ((True, 8), (False, 4)):
                out.append(_tail(A, directional, C))
            if A in TAIL_C3:
                out += [_tail(A, True, 3), _tail(A, True, 4), _tail(A, False, 3), _tail(A, False, 8)]
        return out
    if name == "many_labels":
        return [_many_labels(N, d, C) for N in ML_N for d, C in ((True, 8), (False, 4))]
    if name == "thresholds":
        return [_thresholds(True, 8), _thresholds(False, 4)]
    if name == "clamp_edges":
        return [_clamp_edges(True, 8), _clamp_edges(False, 4)]
    if name == "one_image_full_size":
        return [_one_image_full_size()]
    if name == "big_batch":
        return [_big_batch(True, 300, 128, 8, (96, 128)), _big_batch(False, 300, 128, 8, (96, 128)),
                _big_batch(True, 97, 3969, 8, (136, 168))]
    if name == "fast_path_values":
        return [_golden(True), _golden(False)]
    raise KeyError(name)


FAMILIES = ("queue_full", "queue_full_2d", "tail_sizes", "many_labels", "thresholds", "clamp_edges", "one_image_full_size",
            "big_batch", "fast_path_values")
_FAMILY, _FIGURES = {}, {}


def family(name):
    if name not in _FAMILY:
        _FAMILY[name] = _build(name)
    return _FAMILY[name]


def names(name):
    """Case names of a family without building it (parametrize ids)."""
    if name == "tail_sizes":
        out = []
        for A in TAIL_A:
            out += ["tail_A%d_dir_C8" % A, "tail_A%d_2d_C4" % A]
            if A in TAIL_C3:
                out += ["tail_A%d_dir_C3" % A, "tail_A%d_dir_C4" % A, "tail_A%d_2d_C3" % A, "tail_A%d_2d_C8" % A]
        return out
    if name == "many_labels":
        return ["labels_N%d_%s" % (N, v) for N in ML_N for v in ("dir", "2d")]
    return {"queue_full": ["queue_full"], "queue_full_2d": ["queue_full_2d"], "thresholds": ["thresholds_dir", "thresholds_2d"],
            "clamp_edges": ["clamp_dir", "clamp_2d"], "one_image_full_size": ["one_image_1080p"],
            "big_batch": ["batch_B300_A128_dir", "batch_B300_A128_2d", "batch_B97_A3969_dir"],
            "fast_path_values": ["golden_dir", "golden_2d"]}[name]


def get(fam, name):
    return [c for c in family(fam) if c.name == name][0]


def workspace_pair():
    """Two cases of one shape for the shared-workspace test: the golden case, and the same with its images rolled by one
    (image 2 is the empty one) and the regression negated."""
    x = _golden(True)
    y = Case("golden_dir_rolled", True, x.cls.roll(1, 0), -x.reg.roll(2, 0), x.anchors, x.ann.roll(1, 0))
    return x, y


# ------------------------------------------------------------------------------------------------ reference
def assign_images(case, ann=None, dtype=torch.float32):
    """Per image None (no valid row) or (iou_max [A], original row of the argmax [A], state [A], class [A] int64, argmax
    among the valid rows [A]), from oracle.losses.assign on the inputs as ``dtype``."""
    cc = cls_col(case.directional)
    ann = case.ann if ann is None else ann
    out = []
    for j in range(case.B):
        rows = torch.nonzero(ann[j][:, cc] != -1).reshape(-1)
        if rows.numel() == 0:
            out.append(None)
            continue
        lab = ann[j][rows].to(dtype)
        gt = olosses.envelope_boxes(lab[:, :16]) if case.directional else lab[:, :4]
        iou, arg, state = olosses.assign(case.anchors[0].to(dtype), gt)
        out.append((iou, rows[arg], state, lab[arg, cc].long(), arg))
    return out


@_memo
def assignment(case):
    """The integer decisions of the case: float32, as the kernel and the reference project take them."""
    return assign_images(case)


def plain_units(state):
    """[A] bool: the anchor lies in a 128-anchor unit of plain negatives (the packed fast path of focal_kernel)."""
    A = state.shape[0]
    pad = torch.zeros(((A + UNIT - 1) // UNIT) * UNIT, dtype=torch.bool)
    pad[:A] = state != 0
    return (~pad.reshape(-1, UNIT).any(1)).repeat_interleave(UNIT)[:A]


def _sl1(d):
    return torch.where(d <= 1.0 / 9.0, 4.5 * d * d, d - 0.5 / 9.0)


def _residuals(case, j, pos, row, r, anc):
    """-> (e [P,20|4] target - prediction, wt [20|4] weights on |e|, t raw label rows [P,:]) of image j's positives, float64."""
    aw, ah = (anc[:, 2] - anc[:, 0])[pos, None], (anc[:, 3] - anc[:, 1])[pos, None]
    acx, acy = anc[pos, 0:1] + 0.5 * aw, anc[pos, 1:2] + 0.5 * ah
    g = case.ann[j].double()[row[pos]]
    if case.directional:
        sl, sw, sh = (torch.tensor(s, dtype=torch.float64) for s in (_SL, _SW, _SH))
        px = r[:, 0:1] + sl * r[:, 2:3] + sw * r[:, 4:5] + sh * r[:, 6:7]
        py = r[:, 1:2] + sl * r[:, 3:4] + sw * r[:, 5:6] + sh * r[:, 7:8]
        ex = (g[:, 0:16:2] - acx) / aw - px
        ey = (g[:, 1:16:2] - acy) / ah - py
        eb = torch.cat(((g[:, 16:17] - acx) / aw, (g[:, 17:18] - acy) / ah, (g[:, 18:19] - acx) / aw, (g[:, 19:20] - acy) / ah), 1) - r[:, 8:12]
        wt = torch.tensor([1.0] * 4 + [0.5] * 4 + [1.0] * 4 + [0.5] * 4 + [1.0] * 4, dtype=torch.float64)
        return torch.cat((ex, ey, eb), 1), wt, g
    gw, gh = g[:, 2:3] - g[:, 0:1], g[:, 3:4] - g[:, 1:2]
    gcx, gcy = g[:, 0:1] + 0.5 * gw, g[:, 1:2] + 0.5 * gh
    gw, gh = gw.clamp(min=1.0), gh.clamp(min=1.0)
    t = torch.cat(((gcx - acx) / aw / 0.1, (gcy - acy) / ah / 0.1, torch.log(gw / aw) / 0.2, torch.log(gh / ah) / 0.2), 1)
    return t - r, torch.ones(4, dtype=torch.float64), g


def positive_gaps(case):
    """[(image, positive anchor indices, per row min(|e|, |d - 1/9|), per row the smaller of the centre's two gradients in units
    of the row's scale)].  The directional centre (columns 0:2) collects one +-w sl1'(d) term per corner; where they
    cancel, max|ref| of the group is a rounding residue and no relative measure of it means anything."""
    out = []
    anc = case.anchors[0].double()
    for j, asg in enumerate(assignment(case)):
        if asg is None or not bool((asg[2] == 1).any()):
            continue
        pos = asg[2] == 1
        e, wt, _ = _residuals(case, j, pos, asg[1], case.reg[j].double()[pos], anc)
        d = e.abs() * wt
        gap = torch.minimum(e.abs(), (d - 1.0 / 9.0).abs()).min(1).values
        centre = torch.full_like(gap, np.inf)
        if case.directional:
            g = torch.sign(e) * wt * torch.where(d <= 1.0 / 9.0, 9.0 * d, torch.ones_like(d))
            centre = torch.minimum(g[:, 0:8].sum(1).abs(), g[:, 8:16].sum(1).abs())
        out.append((j, torch.nonzero(pos).reshape(-1), gap.numpy(), centre.numpy()))
    return out


class Result(object):
    def __init__(self, losses, dcls, dreg, **extra):
        self.losses, self.dcls, self.dreg = losses, dcls, dreg
        self.__dict__.update(extra)


@_memo
def reference(case):
    """float64 losses [3|2], dcls, dreg (numpy) and ``a`` [B,A,C], the argument of h per element."""
    return reference_with(case, assignment(case))


def reference_with(case, assigned):
    """The reference on the integer decisions ``assigned`` (as ``assign_images`` returns them)."""
    cls = case.cls.double().requires_grad_(True)
    reg = case.reg.double().requires_grad_(True)
    anc = case.anchors[0].double()
    zero = torch.zeros((), dtype=torch.float64)
    terms = ([], [], [])
    a_all = np.empty(tuple(case.cls.shape), dtype=F64)
    for j, asg in enumerate(assigned):
        p = cls[j].clamp(LO, HI)
        if asg is None:                                                     # raw sum, D/losses.py:58-87
            terms[0].append((0.75 * p * p * -torch.log(1.0 - p)).sum())
            terms[1].append(zero)
            a_all[j] = (1.0 - p).detach().numpy()
            continue
        row, state, cidx = asg[1], asg[2], asg[3]
        pos = state == 1
        hot = torch.zeros(p.shape, dtype=torch.bool)
        hot[pos, cidx[pos]] = True
        a = torch.where(hot, p, 1.0 - p)
        w = torch.where(hot, 0.25, 0.75) * (state >= 0)[:, None].double()
        npos = int(pos.sum())
        terms[0].append((w * (1.0 - a) ** 2 * -torch.log(a)).sum() / max(npos, 1))
        a_all[j] = a.detach().numpy()
        if npos == 0:
            terms[1].append(zero)
            terms[2].append(zero)
            continue
        r = reg[j][pos]
        e, wt, g = _residuals(case, j, pos, row, r, anc)
        terms[1].append(_sl1(e.abs() * wt).mean())
        if case.directional:
            vp = 0.0
            for k, (plus, minus) in enumerate(_VP_GROUPS):
                tx = (sum(g[:, 2 * i] for i in plus) - sum(g[:, 2 * i] for i in minus)) / 4.0
                ty = (sum(g[:, 2 * i + 1] for i in plus) - sum(g[:, 2 * i + 1] for i in minus)) / 4.0
                vx, vy = r[:, 2 + 2 * k], r[:, 3 + 2 * k]
                vp = vp + (1.0 - (vx * tx + vy * ty) / (torch.sqrt(vx * vx + vy * vy) * torch.sqrt(tx * tx + ty * ty)))
            terms[2].append((vp / 3.0).mean())
    losses = [torch.stack(terms[0]).mean(), torch.stack(terms[1]).mean()]
    if case.directional:
        losses.append(torch.stack(terms[2]).mean())                        # over the images that have labels
    sum(w * l for w, l in zip(W_LOSS, losses)).backward()
    dreg = reg.grad.numpy() if reg.grad is not None else np.zeros(tuple(case.reg.shape), F64)
    return Result(np.array([float(l.detach()) for l in losses]), cls.grad.numpy(), dreg, a=a_all)


@_memo
def oracle32(case):
    """oracle.losses in float32 with its own autograd: what the golden vectors hold."""
    c, r = case.cls.clone().requires_grad_(True), case.reg.clone().requires_grad_(True)
    fn = olosses.focal_loss_dir if case.directional else olosses.focal_loss_2d
    out = fn(c, r, case.anchors, case.ann)
    sum(w * o for w, o in zip(W_LOSS, out)).sum().backward()
    dreg = r.grad.numpy() if r.grad is not None else np.zeros(tuple(case.reg.shape), F32)
    return Result(np.array([float(o.detach()) for o in out]), c.grad.numpy(), dreg)


# ------------------------------------------------------------------------------------------------ envelopes
def dcls_cond(a):
    """|h'(a)| ulp32(a) / |h(a)|, float64."""
    a = np.asarray(a, dtype=F64)
    m, ln = 1.0 - a, np.log(a)
    h = 2.0 * m * ln - m * m / a
    hp = -2.0 * ln + 4.0 * m / a + m * m / (a * a)
    return np.abs(hp) * np.spacing(a.astype(F32)).astype(F64) / np.abs(h)


@_memo
def cond_of(case):
    return dcls_cond(reference(case).a)


def dcls_excess(got, case):
    """-> (worst relative error in excess of cond over the elements with ref != 0, got == 0 exactly wherever ref == 0)."""
    ref, cond = reference(case).dcls, cond_of(case)
    got = np.asarray(got, dtype=F64)
    nz = ref != 0
    exact = bool(np.all(got[~nz] == 0))
    if not nz.any():
        return -np.inf, exact
    return float((np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]) - cond[nz]).max()), exact


def dreg_groups(directional):
    return ((0, 2), (2, 8), (8, 12)) if directional else ((0, 4),)


def dreg_metrics(got, case):
    """-> (per column group the worst positive row's max|err| / max|ref|, rows of non-positives exactly zero)."""
    ref = reference(case).dreg.reshape(-1, case.reg.shape[2])
    got = np.asarray(got, dtype=F64).reshape(ref.shape)
    rows = np.zeros(ref.shape[0], dtype=bool)
    for j, asg in enumerate(assignment(case)):
        if asg is not None:
            rows[j * case.A:(j + 1) * case.A] = (asg[2] == 1).numpy()
    exact = bool(np.all(got[~rows] == 0))
    out = []
    for lo, hi in dreg_groups(case.directional):
        if not rows.any():
            out.append(0.0)
            continue
        den = np.abs(ref[rows, lo:hi]).max(1)                  # 0 where a centre's +-scale terms cancel: then err must be 0 too
        err = np.abs(got[rows, lo:hi] - ref[rows, lo:hi]).max(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(float(np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf)).max()))
    return np.array(out), exact


def loss_rel(got, case):
    """Relative error per loss scalar; a reference of exactly 0 (no positive anywhere) must be met exactly."""
    ref = reference(case).losses
    got = np.asarray(got, dtype=F64)[:len(ref)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.where(got == 0, 0.0, np.inf))


@_memo
def oracle_figures(case):
    o = oracle32(case)
    R, exact_c = dcls_excess(o.dcls, case)
    rows, exact_r = dreg_metrics(o.dreg, case)
    return {"R": R, "dreg": rows, "loss": loss_rel(o.losses, case), "exact": exact_c and exact_r}


def family_figures(fam):
    """The float32 oracle's figures of a case family, per variant: {("R" | "dreg" | "loss", directional): worst over the
    family's shapes of that variant}."""
    if fam not in _FIGURES:
        out = {}
        for d in (True, False):
            sel = [oracle_figures(c) for c in family(fam) if c.directional == d]
            if sel:
                out["R", d] = max(f["R"] for f in sel)
                out["dreg", d] = np.max([f["dreg"] for f in sel], axis=0)
                out["loss", d] = np.max([f["loss"] for f in sel], axis=0)
        _FIGURES[fam] = out
    return _FIGURES[fam]


def within(got, case, R, dreg_rows, loss_err):
    """``got`` (losses, dcls, dreg) against the float64 reference of ``case`` inside the envelopes scaled from the float32
    oracle's figures given.  -> (list of failures, dict of the measured figures).  Every bound is written so that a
    measure that is not a number fails it."""
    got = [np.asarray(g, dtype=F64) for g in got]
    bad = ["%s holds values that are not finite" % n for n, g in zip(("losses", "dcls", "dreg"), got) if not np.isfinite(g).all()]
    meas, exact_c = dcls_excess(got[1], case)
    rows, exact_r = dreg_metrics(got[2], case)
    rel = loss_rel(got[0], case)
    if not exact_c:
        bad.append("dcls is not exactly 0 where the reference is")
    if not exact_r:
        bad.append("dreg is not exactly 0 off the positives")
    if not meas <= DCLS_M * R:
        bad.append("dcls excess %.3g > %g x %.3g" % (meas, DCLS_M, R))
    if not np.all(rows <= DREG_M * dreg_rows):
        bad.append("dreg rows %s > %g x %s" % (rows, DREG_M, dreg_rows))
    if not np.all(rel <= np.maximum(LOSS_M * loss_err, LOSS_FLOOR)):
        bad.append("losses rel %s > max(%g x %s, 2^-22)" % (rel, LOSS_M, loss_err))
    return bad, {"R": meas, "dreg": rows, "loss": rel}


def check(got, case, fam):
    """The comparison of the GPU tests: ``within`` the oracle's figures of the case's family and variant."""
    fig, d = family_figures(fam), case.directional
    return within(got, case, fig["R", d], fig["dreg", d], fig["loss", d])

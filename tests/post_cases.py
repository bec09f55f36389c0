"""Edge cases and plain references for the detector's eval tail: rn_rowmax, rn_threshold_select, rn_decode_dir_select and
rn_nms (csrc/boxes.hip, reached again from csrc/tracker_post.hip).  tests/test_post_cases_host.py proves that the cases
are what they claim and that the references agree among themselves; tests/test_gpu_post_edges.py runs the kernels on them.

References
  select_ref    the loop of oracle.boxes.adaptive_threshold with ``keep`` as a parameter: comparison in fp32, ``t`` advancing
                in double by 10**.2; with ``fixed`` it is s > float32(fixed).
  nms_int_ref   greedy NMS in exact integer arithmetic for boxes with integer coordinates: box j is suppressed by a kept box
                i of higher rank iff inter/union > num/den as rationals.  For a positive union that is
                den*inter > num*union in int64; a union of 0 gives what IEEE division gives (0/0 compares false, x/0 with
                x > 0 is +inf and compares true) and a negative union (inverted boxes) a quotient <= 0, never above a
                positive threshold.  Per category when ``cats`` is given, so the fp32 offset trick plays no part.  Rank is
                score descending, ties by lower index, +0.0 and -0.0 equal.
  nms_f64_ref   the same greedy rule with the IoU evaluated in fp64 on the unshifted boxes (for the non-integer family).

Integer NMS cases keep every coordinate an integer below 2048 in magnitude and every side at most 128, so that each
difference, area, sum and union is exact in fp32 and only the division rounds; category offsets up to 17 * 2049 stay exact
integers too.  With unions below 2**20 a quotient that differs from num/den as a rational differs from it by more than an
fp32 ulp, so the fp32 decision ``inter / union > float32(num / den)`` equals the rational one for 1/2 and for 3/10.

Everything is deterministic (numpy.random.default_rng(seed)); nothing here touches a GPU.
"""
import numpy as np

F32 = np.float32
STEP = 10 ** .2                     # D/model.py:326, :372


# ------------------------------------------------------------------------------------------------ references
def thr_table(start, kmax=400):
    """float32(t_k) of the reference's loop, up to and including the first +inf."""
    out, t = [], float(start)
    with np.errstate(over="ignore"):
        for _ in range(kmax):
            out.append(F32(t))
            if np.isinf(out[-1]):
                break
            t *= STEP
    return np.array(out, dtype=F32)


def select_ref_k(scores_f32, start, keep, fixed=None):
    """-> (ascending int32 indices, k of the chosen threshold; 0 for a fixed threshold)."""
    s = np.asarray(scores_f32, dtype=F32)
    if fixed is not None:
        return np.flatnonzero(s > F32(fixed)).astype(np.int32), 0
    t, k = float(start), 0
    with np.errstate(over="ignore", invalid="ignore"):
        while True:
            mask = s > F32(t)
            n = int(mask.sum())
            t *= STEP
            if n <= keep:
                return np.flatnonzero(mask).astype(np.int32), k
            k += 1


def select_ref(scores_f32, start, keep, fixed=None):
    return select_ref_k(scores_f32, start, keep, fixed)[0]


def score_order(scores):
    """Rank of the contract: score descending, ties by lower index, both zeros equal."""
    return np.argsort(-(np.asarray(scores, dtype=np.float64) + 0.0), kind="stable")


def nms_int_ref(boxes_int, scores, cats, num, den):
    """-> int64 kept indices in rank order.  See the module docstring."""
    b = np.asarray(boxes_int)
    assert np.array_equal(b, np.round(b)), "integer coordinates only"
    b = b.astype(np.int64)
    n = b.shape[0]
    order = score_order(scores)
    b = b[order]
    c = None if cats is None else np.asarray(cats, dtype=np.int64)[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        r = b[i + 1:]
        iw = np.maximum(np.minimum(r[:, 2], b[i, 2]) - np.maximum(r[:, 0], b[i, 0]), 0)
        ih = np.maximum(np.minimum(r[:, 3], b[i, 3]) - np.maximum(r[:, 1], b[i, 1]), 0)
        inter = iw * ih
        union = area[i] + area[i + 1:] - inter
        sup = ((union > 0) & (den * inter > num * union)) | ((union == 0) & (inter > 0))
        if c is not None:
            sup &= c[i + 1:] == c[i]
        dead[i + 1:] |= sup
    return order[np.array(keep, dtype=np.int64)]


def nms_f64_ref(boxes, scores, cats, thr, margin=False):
    """Greedy NMS with the IoU in fp64 on the boxes as given (no offsets; other categories never suppress).
    With ``margin`` also returns min |IoU - thr| over every pair the greedy rule evaluates."""
    b = np.asarray(boxes, dtype=np.float64)
    n = b.shape[0]
    order = score_order(scores)
    b = b[order]
    c = None if cats is None else np.asarray(cats, dtype=np.int64)[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(n, dtype=bool)
    keep, closest = [], np.inf
    for i in range(n - 1):
        if dead[i]:
            continue
        keep.append(i)
        r = b[i + 1:]
        iw = np.maximum(np.minimum(r[:, 2], b[i, 2]) - np.maximum(r[:, 0], b[i, 0]), 0)
        ih = np.maximum(np.minimum(r[:, 3], b[i, 3]) - np.maximum(r[:, 1], b[i, 1]), 0)
        inter = iw * ih
        iou = inter / (area[i] + area[i + 1:] - inter)
        if c is not None:
            iou = np.where(c[i + 1:] == c[i], iou, 0.0)
        closest = min(closest, float(np.abs(iou - thr).min()))
        dead[i + 1:] |= iou > thr
    if n and not dead[n - 1]:
        keep.append(n - 1)
    kept = order[np.array(keep, dtype=np.int64)]
    return (kept, closest) if margin else kept


def iou_fraction(a, b):
    """(inter, union) of two integer boxes, as integers."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0)
    inter = iw * ih
    return inter, (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter


# ------------------------------------------------------------------------------------------------ NMS cases
class NmsCase:
    """One rn_nms problem.  ``boxes`` [rows, box_stride] fp32 with the box in columns box_col:box_col+4, ``scores`` a flat
    fp32 buffer read at src * score_stride, ``cand_idx`` [n] the source row of each candidate, ``cats`` [n] per candidate
    or None.  The threshold is num/den (``thr`` is the float handed to the kernel).  ``ref_cats`` is what nms_int_ref
    gets: ``cats``, except where the offset trick collapses (see degenerate_negative_collapsed)."""

    def __init__(self, name, boxes, scores, cats=None, num=1, den=2, box_col=0, score_stride=1, cand_idx=None, integer=True,
                 ref_cats="same"):
        self.name = name
        self.boxes = np.ascontiguousarray(boxes, dtype=F32)
        self.scores = np.ascontiguousarray(scores, dtype=F32)
        self.box_stride, self.box_col, self.score_stride = self.boxes.shape[1], box_col, score_stride
        self.cand_idx = np.arange(self.boxes.shape[0], dtype=np.int32) if cand_idx is None else np.asarray(cand_idx, np.int32)
        self.n = self.cand_idx.shape[0]
        self.cats = None if cats is None else np.asarray(cats, dtype=np.int32)
        self.ref_cats = self.cats if isinstance(ref_cats, str) else ref_cats
        self.num, self.den, self.thr = num, den, num / den
        self.integer = integer

    def cand_boxes(self):
        return self.boxes[self.cand_idx.astype(np.int64), self.box_col:self.box_col + 4]

    def cand_scores(self):
        return self.scores[self.cand_idx.astype(np.int64) * self.score_stride]

    def __repr__(self):
        return self.name


_EXPECTED = {}


def nms_expected(case):
    """Kept candidate positions in rank order, computed once per case: nms_int_ref for integer cases, the oracle
    (fp32, the reference's operation order) for the non-integer family."""
    if case.name not in _EXPECTED:
        if case.integer:
            want = nms_int_ref(case.cand_boxes(), case.cand_scores(), case.ref_cats, case.num, case.den)
        else:
            want = nms_oracle(case)
        want.setflags(write=False)
        _EXPECTED[case.name] = want
    return _EXPECTED[case.name]


def nms_oracle(case):
    import torch
    from oracle import boxes as oboxes
    b, s = torch.from_numpy(case.cand_boxes().copy()), torch.from_numpy(case.cand_scores().copy())
    if case.cats is None:
        return oboxes.greedy_nms(b, s, case.thr).numpy()
    return oboxes.batched_nms(b, s, torch.from_numpy(case.cats.astype(np.int64)), case.thr).numpy()


GRID, CELL = 92, 22                 # cluster origins: 92 x 92 cells of 22 px; (92 - 1) * 22 + 5 + 20 = 2027 < 2048


def clustered_boxes(n, seed, clusters=None):
    """n integer boxes in max(1, n // 2) clusters (sides 16..20 per cluster, jitter 0..5 per box): inside a cluster some
    pairs overlap above 1/2 and some do not, neighbouring clusters overlap a little, and roughly half of the boxes
    survive NMS at 1/2."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 2) if clusters is None else clusters
    assert k <= GRID * GRID
    cells = rng.permutation(GRID * GRID)[:k]
    side = rng.integers(16, 21, size=(k, 2))
    which = rng.integers(0, k, size=n)
    jit = rng.integers(0, 6, size=(n, 2))
    x1 = (cells[which] % GRID) * CELL + jit[:, 0]
    y1 = (cells[which] // GRID) * CELL + jit[:, 1]
    return np.stack((x1, y1, x1 + side[which, 0], y1 + side[which, 1]), axis=1).astype(F32)


def distinct_scores(n, seed):
    """n distinct fp32 scores in (0, 1) in a seeded random order."""
    rng = np.random.default_rng(seed)
    return ((rng.permutation(n) + 1) / F32(n + 1)).astype(F32)


NMS_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 10000, 16383, 16384)


def nms_size_case(n):
    boxes = clustered_boxes(n, seed=1000 + n)
    scores = distinct_scores(n, seed=2000 + n)
    if n >= 130:                    # chunk 0 suppresses into the last word: the last-ranked box copies the first-ranked
        boxes[int(np.argmin(scores))] = boxes[int(np.argmax(scores))]
    return NmsCase("size_%d" % n, boxes, scores)


CHAIN_N, CHAIN_W, CHAIN_STEP = 200, 32, 8     # IoU with the neighbour 24/40, with the second neighbour 16/48


def chain_boxes():
    x1 = np.arange(CHAIN_N) * CHAIN_STEP
    return np.stack((x1, np.full(CHAIN_N, 100), x1 + CHAIN_W, np.full(CHAIN_N, 100 + CHAIN_W)), axis=1).astype(F32)


def chain_case():
    """Box of rank r sits at x = 8 r: it overlaps rank r +- 1 above 1/2 and rank r +- 2 below.  Greedy NMS keeps the even
    ranks; "suppressed by anything" would keep rank 0 alone.  Ranks are scattered over the candidate positions."""
    rank_of_pos = np.random.default_rng(7).permutation(CHAIN_N)
    boxes = chain_boxes()[rank_of_pos]
    scores = (1.0 - rank_of_pos / F32(CHAIN_N + 1)).astype(F32)
    return NmsCase("chain", boxes, scores)


def tie_cases():
    out = []
    n = 150
    out.append(NmsCase("ties_all_equal", clustered_boxes(n, 31, clusters=40), np.full(n, 0.5, dtype=F32)))
    n = 300
    rng = np.random.default_rng(32)
    blocks = (rng.permutation(n) // 37).astype(F32)                     # 8 blocks of 37 equal scores and one of 4
    out.append(NmsCase("ties_blocks", clustered_boxes(n, 33, clusters=60), (blocks + 1) / 16))
    n = 130
    rng = np.random.default_rng(34)
    z = np.where(rng.integers(0, 2, size=n) == 1, F32(0.0), F32(-0.0)).astype(F32)
    z[:8] = [-0.0, 0.0, -0.0, -0.0, 0.0, 0.0, -0.0, 0.0]
    boxes = clustered_boxes(n, 35, clusters=30)
    boxes[0] = boxes[1] = (2028, 0, 2046, 18)                           # a -0.0 box right before its +0.0 copy, twice,
    boxes[3] = boxes[4] = (2028, 30, 2046, 48)                          # clear of every cluster (those end at x = 2027)
    out.append(NmsCase("ties_signed_zeros", boxes, z))
    n = 140
    rng = np.random.default_rng(36)
    z = np.where(rng.integers(0, 2, size=n) == 1, F32(0.0), F32(-0.0)).astype(F32)
    z[rng.permutation(n)[:40]] = np.linspace(-1.0, 1.0, 40, dtype=F32)   # zeros of both signs between other scores
    out.append(NmsCase("ties_zeros_among_others", clustered_boxes(n, 37, clusters=30), z))
    n = 100
    rng = np.random.default_rng(38)
    neg = -(rng.integers(1, 30, size=n) / F32(8))                       # negative, with ties
    out.append(NmsCase("ties_negative", clustered_boxes(n, 39, clusters=25), neg))
    return out


# (name, box A, box B, num, den, inter, union, B survives): A has the higher score
THRESHOLD_PAIRS = (
    ("iou_1_2_at_0.5", (0, 0, 30, 8), (10, 0, 40, 8), 1, 2, 160, 320, True),
    ("iou_51_100_at_0.5", (0, 0, 20, 5), (1, 1, 18, 4), 1, 2, 51, 100, False),
    ("iou_3_10_at_0.3", (0, 0, 10, 10), (0, 0, 6, 5), 3, 10, 30, 100, True),
    ("iou_31_100_at_0.3", (0, 0, 50, 2), (0, 0, 31, 1), 3, 10, 31, 100, False),
)


def threshold_cases():
    out = []
    for name, a, b, num, den, _, _, _ in THRESHOLD_PAIRS:
        shift = np.array([700, 900, 700, 900])
        out.append(NmsCase("thr_" + name, np.array([b, a]) + shift, np.array([0.25, 0.75]), num=num, den=den))
    return out


def degenerate_cases():
    out = []
    out.append(NmsCase("degenerate_zero_area_identical", np.array([[5, 5, 5, 5]] * 3), np.array([0.3, 0.9, 0.6])))
    out.append(NmsCase("degenerate_zero_width", np.array([[3, 0, 3, 10], [0, 0, 10, 10], [3, 0, 3, 10], [0, 0, 10, 10]]),
                       np.array([0.9, 0.8, 0.7, 0.6])))
    inv = np.array([[0, 0, 10, 10],        # normal
                    [8, 8, 2, 2],          # both axes inverted: area +36, never intersects
                    [8, 0, 2, 10],         # x inverted: area -60
                    [8, 0, 2, 10],         # its copy: union -120
                    [10, 10, 0, 0],        # the normal box with its corners swapped
                    [0, 0, 2, 2],          # small box inside the normal one (IoU 4/100) and against area -60: union -56
                    [0, 0, 10, 10]])       # a copy of the normal box: the only one suppressed
    out.append(NmsCase("degenerate_inverted", inv, np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3])))
    # all coordinates negative: batched_nms offsets by idxs * (max + 1) with max + 1 <= 0.  Every coordinate lies in
    # [-160, -106], a span of 54, and max + 1 <= -105: the categories still move apart, towards minus infinity
    n = 120
    rng = np.random.default_rng(41)
    x1, y1 = rng.integers(-160, -130, size=n), rng.integers(-160, -130, size=n)
    b = np.stack((x1, y1, x1 + rng.integers(10, 26, size=n), y1 + 18), axis=1)
    out.append(NmsCase("degenerate_negative_batched", b, distinct_scores(n, 43), cats=rng.integers(0, 18, size=n)))
    # max = -1: the offset is 0 for every category, so categories DO suppress each other (reference behaviour, kept);
    # the integer reference is therefore asked without categories
    out.append(NmsCase("degenerate_negative_collapsed", b - (b.max() + 1), distinct_scores(n, 44),
                       cats=rng.integers(0, 18, size=n), ref_cats=None))
    return out


BATCHED_BASE, BATCHED_DUPS = 20, 40


def batched_case():
    """Categories 0..17, the same 20 disjoint boxes in each (all 360 kept), then 40 in-category duplicates with lower
    scores (suppressed); the maximum coordinate, 2047, belongs to the last candidate."""
    rng = np.random.default_rng(51)
    cells = rng.permutation(GRID * GRID)[:BATCHED_BASE]
    cx, cy = (cells % GRID) * CELL, (cells // GRID) * CELL
    base = np.stack((cx, cy, cx + 20, cy + 20), axis=1).astype(F32)     # one box per cell, side 20 < 22: disjoint
    boxes = np.tile(base, (18, 1))
    cats = np.repeat(np.arange(18), BATCHED_BASE)
    perm = rng.permutation(boxes.shape[0])
    boxes, cats = boxes[perm], cats[perm]
    dup = rng.integers(0, boxes.shape[0], size=BATCHED_DUPS)
    boxes = np.concatenate((boxes, boxes[dup], np.array([[2030, 2030, 2047, 2047]], dtype=F32)))
    cats = np.concatenate((cats, cats[dup], [9]))
    n = boxes.shape[0]
    scores = np.concatenate((0.5 + distinct_scores(18 * BATCHED_BASE, 53) / 2, distinct_scores(BATCHED_DUPS, 54) / 4, [0.3]))
    assert scores.shape[0] == n
    return NmsCase("batched_18", boxes, scores, cats=cats)


def indirection_case():
    """rn_nms the way postprocess_single calls it: boxes in columns 16:20 of 20, scores with stride 3, and a candidate
    list that is neither the identity nor monotonic over a larger array.  ``keep`` holds candidate positions."""
    rows, n = 500, 200
    rng = np.random.default_rng(61)
    boxes = rng.integers(0, 2000, size=(rows, 20)).astype(F32)          # other columns: unrelated numbers
    boxes[:, 16:20] = clustered_boxes(rows, 62, clusters=120)
    scores = rng.random(rows * 3).astype(F32)
    scores[0::3] = distinct_scores(rows, 63)
    cand = rng.permutation(rows)[:n]
    assert np.any(np.diff(cand) < 0) and np.any(np.diff(cand) > 0)
    return NmsCase("indirection", boxes, scores, box_col=16, score_stride=3, cand_idx=cand)


FLOAT_N, FLOAT_SEED = 3000, 71


def float_cases():
    """The one non-integer family: compared with the oracle only (fp32, the reference's operation order)."""
    rng = np.random.default_rng(FLOAT_SEED)
    n = FLOAT_N
    centre = rng.random((n // 3, 2)) * 900 + 50
    which = rng.integers(0, n // 3, size=n)
    c = centre[which] + rng.normal(0, 4.0, size=(n, 2))
    wh = rng.random((n, 2)) * 40 + 20
    boxes = np.concatenate((c - wh / 2, c + wh / 2), axis=1).astype(F32)
    scores = rng.random(n).astype(F32)
    cats = rng.integers(0, 18, size=n)
    return [NmsCase("float_plain", boxes, scores, integer=False),
            NmsCase("float_batched", boxes, scores, cats=cats, integer=False)]


_NMS_CACHE = {}


def _cached(key, fn):
    if key not in _NMS_CACHE:
        _NMS_CACHE[key] = fn()
    return _NMS_CACHE[key]


def nms_small_cases():
    """Every integer family except the sizes."""
    return _cached("small", lambda: [chain_case()] + tie_cases() + threshold_cases() + degenerate_cases() +
                   [batched_case(), indirection_case()])


def nms_case_names():
    return ["size_%d" % n for n in NMS_SIZES] + [c.name for c in nms_small_cases()] + ["float_plain", "float_batched"]


def nms_case(name):
    def make():
        if name.startswith("size_"):
            return nms_size_case(int(name[5:]))
        for c in nms_small_cases() + float_cases():
            if c.name == name:
                return c
        raise KeyError(name)
    return _cached(name, make)


# ------------------------------------------------------------------------------------------------ select cases
class SelectCase:
    """One rn_threshold_select problem: ``buf`` is the flat fp32 buffer, the scores are buf[offset + i * stride], i < n."""

    def __init__(self, name, scores, start, keep, fixed=None, stride=1, offset=0, buf=None, want_k=None, want_count=None):
        self.name, self.start, self.keep, self.fixed, self.stride, self.offset = name, start, keep, fixed, stride, offset
        scores = np.ascontiguousarray(scores, dtype=F32)
        self.n = scores.shape[0]
        if buf is None:
            assert stride == 1 and offset == 0
            buf = scores
        self.buf = buf
        assert np.array_equal(self.scores(), scores, equal_nan=True)
        self.want_k, self.want_count = want_k, want_count            # what the case was designed to give

    def scores(self):
        return self.buf[self.offset::self.stride][:self.n]

    def __repr__(self):
        return self.name


_SEL_EXPECTED = {}


def select_expected(case):
    """(indices, k) from select_ref_k, computed once per case."""
    if case.name not in _SEL_EXPECTED:
        idx, k = select_ref_k(case.scores(), case.start, case.keep, case.fixed)
        idx.setflags(write=False)
        _SEL_EXPECTED[case.name] = (idx, k)
    return _SEL_EXPECTED[case.name]


SELECT_SIZES = (1, 255, 256, 1023, 1024, 1025, 4097, 1048577, 2097152 + 5)
SEL_BLOCK = 1024


def select_size_case(n):
    """keep = 100, start = 1e-7.  Background 1e-9 (never selected); 150 scores of 1e-5 that the loop has to climb past
    (k >= 1 wherever they exceed keep together with the survivors); the survivors (0.25 .. 0.75) sit in the first and the
    last 1024-block and, where they exist, in blocks 1023, 1024 and 2048: at the first, last and middle position of each
    and at five more.  2 and 3 passes of the block scan at the two largest sizes, the carry used once and twice."""
    rng = np.random.default_rng(3000 + n % 9973)
    s = np.full(n, 1e-9, dtype=F32)
    nblocks = (n + SEL_BLOCK - 1) // SEL_BLOCK
    mid = rng.permutation(n)[:min(150, n)]
    s[mid] = 1e-5
    hot = []
    for blk in sorted({0, nblocks - 1} | {b for b in (1023, 1024, 2048) if b < nblocks}):
        lo, hi = blk * SEL_BLOCK, min(n, (blk + 1) * SEL_BLOCK)
        hot += [lo, hi - 1, (lo + hi) // 2] + list(lo + rng.permutation(hi - lo)[:5])
    hot = np.unique(hot)
    s[hot] = (0.25 + 0.5 * rng.random(hot.shape[0])).astype(F32)
    return SelectCase("size_%d" % n, s, 1e-7, 100, want_count=int(hot.shape[0]))


PATTERN_BLOCKS = ("all", "none", "alternating", "lane0", "lane63", "all", "last_valid")
PATTERN_N = 6 * SEL_BLOCK + 333     # the seventh block is partial


def pattern_scores():
    s = np.full(PATTERN_N, 0.01, dtype=F32)
    i = np.arange(PATTERN_N)
    blk, lane = i // SEL_BLOCK, i % 64
    hot = np.zeros(PATTERN_N, dtype=bool)
    for b, p in enumerate(PATTERN_BLOCKS):
        m = blk == b
        hot |= m & {"all": True, "none": False, "alternating": i % 2 == 1, "lane0": lane == 0, "lane63": lane == 63,
                    "last_valid": i == PATTERN_N - 1}[p]
    s[hot] = 0.5 + (i[hot] % 251) / F32(1024)
    return s, int(hot.sum())


def keep_boundary_cases():
    """start = 1e-7, keep = 64, around t_3 and t_4 of the table (n = 1500, several 1024-blocks' worth is not needed)."""
    T = thr_table(1e-7)
    up = lambda v: np.nextafter(F32(v), F32(np.inf))
    n = 1500
    out = []
    for name, above3, above4, want_k, want_count in (("keep_exactly_full", 64, 10, 3, 64), ("keep_plus_one", 65, 30, 4, 30)):
        rng = np.random.default_rng(81 + above3)
        s = np.zeros(n, dtype=F32)
        pos = rng.permutation(n)
        hi4, hi3, eq3, mid = pos[:above4], pos[above4:above3], pos[above3:above3 + 20], pos[above3 + 20:above3 + 120]
        s[hi4] = np.linspace(up(T[4]), 0.9, above4, dtype=F32)          # > t_4 (the smallest is the next float after it)
        s[hi3] = np.linspace(up(T[3]), T[4], above3 - above4, dtype=F32)  # in (t_3, t_4]: the largest equals t_4
        s[eq3] = T[3]                                                   # equal to float32(t_3): not above it
        s[mid] = np.linspace(up(T[2]), T[3], 100, dtype=F32)             # in (t_2, t_3]
        out.append(SelectCase(name, s, 1e-7, 64, want_k=want_k, want_count=want_count))
    return out


def select_small_cases():
    out = []
    s, cnt = pattern_scores()
    out.append(SelectCase("patterns_adaptive", s, 1e-1, 4000, want_k=0, want_count=cnt))   # background 0.01 < start
    out.append(SelectCase("patterns_fixed", s, 0.0, 64, fixed=0.05, want_count=cnt))
    out += keep_boundary_cases()
    n = 3000
    rng = np.random.default_rng(91)
    out.append(SelectCase("all_below_start", (rng.random(n) * 1e-8).astype(F32), 1e-7, 100, want_k=0, want_count=0))
    s = (rng.random(n) * 1e-3).astype(F32)
    s[rng.permutation(n)[:200]] = 0.9
    out.append(SelectCase("too_many_equal", s, 1e-7, 100, want_count=0))
    T25 = thr_table(1e-25)
    s = (rng.random(n) * 1e-3).astype(F32)
    pos = rng.permutation(n)
    s[pos[:150]] = 3e38
    s[pos[150:170]] = np.inf
    out.append(SelectCase("huge_and_inf_none", s, 1e-25, 100, want_k=len(T25) - 1, want_count=0))
    s = s.copy()
    s[pos[:150]] = 2e38
    out.append(SelectCase("inf_above_last_finite", s, 1e-25, 100, want_k=len(T25) - 2, want_count=20))
    s = (rng.random(n)).astype(F32) * F32(1e-3)
    s[pos[:50]] = 0.5
    s[pos[50:60]] = np.nan
    s[[0, n - 1]] = np.nan
    out.append(SelectCase("nan_never_selected", s, 1e-7, 100, want_count=50))
    # column 1 of an [n, 3] matrix through an offset base pointer, as postprocess_single calls it
    n = 2500
    m = (rng.random((n, 3)) * 1e-3).astype(F32)
    m[rng.permutation(n)[:300], 0] = 0.9                                 # the neighbouring columns would change the count
    m[rng.permutation(n)[:300], 2] = 0.9
    m[rng.permutation(n)[:77], 1] = 0.7
    out.append(SelectCase("strided_column", m[:, 1].copy(), 1e-7, 100, stride=3, offset=1, buf=m.reshape(-1), want_count=77))
    n = 2077
    s = (rng.random(n) * 0.1).astype(F32)                               # about half above 0.05: more than keep
    s[5] = 0.05                                                          # equal to float32(0.05): not selected
    out.append(SelectCase("fixed_over_keep", s, 0.0, 64, fixed=0.05))
    out.append(SelectCase("fixed_everything", (0.06 + rng.random(n) * 0.9).astype(F32), 0.0, 64, fixed=0.05, want_count=n))
    return out


_SEL_CACHE = {}


def select_case_names():
    return ["size_%d" % n for n in SELECT_SIZES] + [c.name for c in _sel_small()]


def _sel_small():
    if "small" not in _SEL_CACHE:
        _SEL_CACHE["small"] = select_small_cases()
    return _SEL_CACHE["small"]


def select_case(name):
    if name not in _SEL_CACHE:
        if name.startswith("size_"):
            _SEL_CACHE[name] = select_size_case(int(name[5:]))
        else:
            _SEL_CACHE[name] = [c for c in _sel_small() if c.name == name][0]
    return _SEL_CACHE[name]


# ------------------------------------------------------------------------------------------------ rowmax, decode_dir_select
def rowmax_cases():
    """(name, cls [n, C] fp32).  The reference is numpy's max / argmax (first maximum)."""
    rng = np.random.default_rng(101)
    ties = rng.integers(0, 3, size=(257, 8)).astype(F32) / 4             # many equal maxima per row: first index wins
    last = rng.random((257, 8)).astype(F32) * F32(0.5)
    last[:, 7] = 0.75
    ninf = rng.random((5, 4)).astype(F32)
    ninf[2] = -np.inf
    ninf[3, 1:] = -np.inf
    return [("ties", ties), ("one_class", rng.random((257, 1)).astype(F32)), ("max_in_last_column", last),
            ("one_row", np.array([[0.1, 0.7, 0.7, 0.2]], dtype=F32)), ("row_of_minus_inf", ninf)]


def rowmax_ref(cls):
    return cls.max(axis=1), cls.argmax(axis=1).astype(np.int64)


DDS_MAX = 300                       # max_candidates of the decode_dir_select cases
DDS_COUNTS = (0, 1, 257, DDS_MAX)


def decode_select_inputs(B=3, A=700, C=4, seed=111):
    """anchors [1,A,4], reg [B,A,12], cls [B,A,C] for rn_decode_dir_select; scores are read through stride C."""
    rng = np.random.default_rng(seed)
    x1 = rng.integers(0, 1800, size=A)
    y1 = rng.integers(0, 1000, size=A)
    anchors = np.stack((x1, y1, x1 + rng.integers(8, 200, size=A), y1 + rng.integers(8, 200, size=A)), axis=1).astype(F32)[None]
    reg = rng.normal(0, 0.3, size=(B, A, 12)).astype(F32)
    cls = rng.random((B, A, C)).astype(F32)
    return anchors, reg, cls


def decode_select_sel(count, total, seed=112):
    """``count`` ascending flat anchor indices of [B*A], first and last anchor included when there is room."""
    rng = np.random.default_rng(seed + count)
    if count < 2:
        return rng.permutation(total)[:count].astype(np.int32)
    inner = 1 + rng.permutation(total - 2)[:count - 2]
    return np.sort(np.concatenate(([0, total - 1], inner))).astype(np.int32)


# ------------------------------------------------------------------------------------------------ wrapper inputs
def p2d_inputs(above, A, C=2, seed=121):
    """postprocess_2d: ``above`` scores above 0.05 in class 0 (a handful in class 1), clustered integer boxes [1,A,4]."""
    rng = np.random.default_rng(seed)
    cls = (rng.random((1, A, C)) * 0.04).astype(F32)
    pos = rng.permutation(A)
    cls[0, pos[:above], 0] = 0.06 + distinct_scores(above, seed + 1) * F32(0.9)
    cls[0, pos[:37], C - 1] = 0.06 + distinct_scores(37, seed + 2) * F32(0.9)
    return cls, clustered_boxes(A, seed + 3, clusters=min(A // 2, GRID * GRID))[None]


def psingle_inputs(C, A=300, seed=131, empty_class=None):
    """postprocess_single: cls [1,A,C], boxes [1,A,20] with clustered integer boxes in columns 16:20."""
    rng = np.random.default_rng(seed)
    cls = rng.random((1, A, C)).astype(F32)
    if empty_class is not None:
        cls[0, :, empty_class] = 0.0                                    # nothing above 1e-25
    boxes = rng.integers(0, 2000, size=(1, A, 20)).astype(F32)
    boxes[0, :, 16:20] = clustered_boxes(A, seed + 1, clusters=80)
    return cls, boxes


DETECT_B, DETECT_A, DETECT_C, DETECT_COUNT = 2, 6000, 3, 10000


def detect_inputs(seed=141):
    """detect_multi with exactly 10000 row maxima above 1e-7 (the rest at 1e-9): the candidate list is exactly full."""
    rng = np.random.default_rng(seed)
    A = DETECT_A
    cells = rng.integers(0, GRID * GRID, size=A)
    x1, y1 = (cells % GRID) * CELL + rng.integers(0, 6, size=A), (cells // GRID) * CELL + rng.integers(0, 6, size=A)
    anchors = np.stack((x1, y1, x1 + 20, y1 + 20), axis=1).astype(F32)[None]
    reg = rng.normal(0, 0.05, size=(DETECT_B, A, 12)).astype(F32)
    reg[:, :, 8:10] -= 0.5                                              # 2D box: about the anchor itself
    reg[:, :, 10:12] += 0.5
    cls = np.full((DETECT_B * A, DETECT_C), 1e-9, dtype=F32)
    pos = rng.permutation(DETECT_B * A)[:DETECT_COUNT]
    cls[pos, rng.integers(0, DETECT_C, size=DETECT_COUNT)] = 0.05 + distinct_scores(DETECT_COUNT, seed + 1) * F32(0.9)
    return anchors, reg, cls.reshape(DETECT_B, A, DETECT_C)


# ------------------------------------------------------------------------------------------------ tracker inputs
def corners_from_boxes(boxes):
    """[d,4] integer boxes -> [d,8,2] integer image corners whose envelope is the box (im_nms takes min / max over the
    eight): the four corners twice, in two different orders."""
    b = np.asarray(boxes, dtype=F32)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    pts = [(x2, y1), (x1, y1), (x2, y2), (x1, y2), (x1, y2), (x2, y2), (x1, y1), (x2, y1)]
    return np.stack([np.stack(p, axis=1) for p in pts], axis=1).astype(F32)


def states_from_boxes(boxes, seed=151):
    """[d,4] integer boxes with even heights -> [d,6] states (x_rear, y_ctr, l, w, h, dir) whose road-plane footprint is
    the box exactly: x from x_rear to x_rear + dir * l, y = y_ctr -+ w / 2."""
    b = np.asarray(boxes, dtype=F32)
    d = b.shape[0]
    direction = np.where(np.random.default_rng(seed).integers(0, 2, size=d) == 1, 1.0, -1.0).astype(F32)
    w = b[:, 3] - b[:, 1]
    assert np.all(w % 2 == 0)
    x_rear = np.where(direction > 0, b[:, 0], b[:, 2])
    return np.stack((x_rear, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], w, np.full(d, 5.0), direction), axis=1).astype(F32)


def tracker_cases():
    """(name, boxes [d,4], scores, num, den): one tie case and one chain case for im_nms / space_nms."""
    n = 150
    tb = clustered_boxes(n, 161, clusters=40)
    tb[:, 3] = tb[:, 1] + 18                                            # even height for states_from_boxes
    ts = (np.random.default_rng(162).permutation(n) // 30 + 1).astype(F32) / 8     # five blocks of 30 equal scores
    c = chain_case()
    return [("ties", tb, ts, 1, 2), ("chain", c.cand_boxes(), c.cand_scores(), 1, 2)]

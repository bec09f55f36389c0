"""The cases of tests/post_cases.py are what they claim, and its references agree among themselves (no GPU): the integer
NMS reference against the oracle's fp32 greedy_nms / batched_nms on every integer case with no exception -- which is what
pins oracle/boxes.py's NMS --, the fp64 evaluation against the oracle on the non-integer family, select_ref against
oracle.boxes.adaptive_threshold, and each family's own property.  The conditions here are conditions, not tolerances."""
import numpy as np
import pytest
import torch

import post_cases as pc
from oracle import boxes as oboxes

INT_NAMES = [n for n in pc.nms_case_names() if not n.startswith("float_")]


# ------------------------------------------------------------------------------------------------ NMS references
@pytest.mark.parametrize("name", INT_NAMES)
def test_integer_reference_equals_oracle(name):
    case = pc.nms_case(name)
    b = case.cand_boxes()
    assert np.array_equal(b, np.round(b)) and np.abs(b).max() < 2048
    assert np.abs(b[:, 2:] - b[:, :2]).max() <= 128
    assert np.array_equal(pc.nms_expected(case), pc.nms_oracle(case))


@pytest.mark.parametrize("name", ["float_plain", "float_batched"])
def test_float_family_fp64_equals_oracle_with_margin(name):
    case = pc.nms_case(name)
    assert case.n == pc.FLOAT_N and not np.array_equal(case.cand_boxes(), np.round(case.cand_boxes()))
    want64, closest = pc.nms_f64_ref(case.cand_boxes(), case.cand_scores(), case.cats, case.thr, margin=True)
    assert closest > 1e-5, closest                       # no evaluated pair within 1e-5 of the threshold in fp64
    assert np.array_equal(want64, pc.nms_expected(case))  # zero disagreements with the fp32 oracle
    assert 0.3 * case.n < len(want64) < case.n


def test_threshold_float_identities():
    assert np.float32(3) / np.float32(10) == np.float32(0.3)
    assert np.float32(30) / np.float32(100) == np.float32(0.3)
    assert np.float32(31) / np.float32(100) > np.float32(0.3)
    assert np.float32(160) / np.float32(320) == np.float32(0.5) and np.float32(51) / np.float32(100) > np.float32(0.5)


# ------------------------------------------------------------------------------------------------ NMS families
@pytest.mark.parametrize("n", pc.NMS_SIZES)
def test_size_family(n):
    case = pc.nms_case("size_%d" % n)
    kept = pc.nms_expected(case)
    s = case.cand_scores()
    assert case.n == n and len(np.unique(s)) == n
    if n >= 63:
        assert 0.4 * n <= len(kept) <= 0.6 * n           # roughly half survive
    if n >= 130:
        order = pc.score_order(s)
        assert np.array_equal(case.cand_boxes()[order[0]], case.cand_boxes()[order[-1]])
        assert kept[0] == order[0] and order[-1] not in kept   # chunk 0 suppresses into the last word


def test_chain_family():
    case = pc.nms_case("chain")
    b = pc.chain_boxes()
    assert pc.iou_fraction(b[0], b[1]) == (24 * 32, 40 * 32) and pc.iou_fraction(b[0], b[2]) == (16 * 32, 48 * 32)
    order = pc.score_order(case.cand_scores())
    assert np.array_equal(case.cand_boxes()[order], b) and not np.array_equal(order, np.arange(pc.CHAIN_N))
    assert np.array_equal(pc.nms_expected(case), order[0::2])    # alternating survivors
    assert pc.CHAIN_N > 3 * 64                           # crosses three 64-chunks


def test_tie_families():
    s = pc.nms_case("ties_all_equal").cand_scores()
    assert len(np.unique(s)) == 1 and len(s) == 150
    _, counts = np.unique(pc.nms_case("ties_blocks").cand_scores(), return_counts=True)
    assert sorted(counts.tolist()) == [4] + [37] * 8
    for name in ("ties_signed_zeros", "ties_zeros_among_others"):
        z = pc.nms_case(name).cand_scores()
        zero = z == 0
        assert np.signbit(z[zero]).sum() >= 20 and (~np.signbit(z[zero])).sum() >= 20
    case = pc.nms_case("ties_signed_zeros")
    z, b, kept = case.cand_scores(), case.cand_boxes(), pc.nms_expected(case)
    assert np.all(z == 0)
    for lo, hi in ((0, 1), (3, 4)):                      # -0.0 at the lower index, +0.0 copy right after: the lower one wins
        assert np.signbit(z[lo]) and not np.signbit(z[hi]) and np.array_equal(b[lo], b[hi])
        assert lo in kept and hi not in kept
    assert np.array_equal(kept, np.sort(kept))           # all equal: rank is the candidate position
    z = pc.nms_case("ties_zeros_among_others").cand_scores()
    assert (z > 0).sum() >= 10 and (z < 0).sum() >= 10
    neg = pc.nms_case("ties_negative").cand_scores()
    assert np.all(neg < 0) and len(np.unique(neg)) < len(neg)


@pytest.mark.parametrize("row", pc.THRESHOLD_PAIRS, ids=[r[0] for r in pc.THRESHOLD_PAIRS])
def test_threshold_pairs(row):
    name, a, b, num, den, inter, union, survives = row
    assert pc.iou_fraction(a, b) == (inter, union)
    assert (den * inter > num * union) != survives
    case = pc.nms_case("thr_" + name)
    assert case.thr == num / den and pc.iou_fraction(*case.cand_boxes()) == (inter, union)
    assert pc.nms_expected(case).tolist() == ([1, 0] if survives else [1])


def test_degenerate_families():
    assert pc.nms_expected(pc.nms_case("degenerate_zero_area_identical")).tolist() == [1, 2, 0]      # 0/0: all kept
    assert pc.nms_expected(pc.nms_case("degenerate_zero_width")).tolist() == [0, 1, 2]
    case = pc.nms_case("degenerate_inverted")
    b = case.cand_boxes()
    assert ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) < 0).sum() == 2
    assert pc.nms_expected(case).tolist() == [0, 1, 2, 3, 4, 5]
    case = pc.nms_case("degenerate_negative_batched")
    b = case.cand_boxes()
    assert b.max() + 1 <= 0 and b.max() - b.min() < -(b.max() + 1)         # the categories still move apart
    assert len(pc.nms_expected(case)) < case.n
    case = pc.nms_case("degenerate_negative_collapsed")
    assert case.cand_boxes().max() == -1 and case.ref_cats is None and len(np.unique(case.cats)) == 18
    per_cat = pc.nms_int_ref(case.cand_boxes(), case.cand_scores(), case.cats, 1, 2)
    assert len(pc.nms_expected(case)) < len(per_cat)      # the zero offset lets categories suppress each other


def test_batched_and_indirection_families():
    case = pc.nms_case("batched_18")
    kept = pc.nms_expected(case)
    n_base = 18 * pc.BATCHED_BASE
    assert np.array_equal(np.unique(case.cats), np.arange(18))
    assert np.array_equal(np.sort(kept), np.r_[np.arange(n_base), case.n - 1])       # the duplicates go, all else stays
    b = case.cand_boxes()
    assert b[-1].max() == b.max() == 2047 and b[:-1].max() < 2047                    # the maximum sits in the last candidate
    case = pc.nms_case("indirection")
    assert (case.box_stride, case.box_col, case.score_stride) == (20, 16, 3)
    assert case.boxes.shape[0] > case.n and len(np.unique(case.cand_idx)) == case.n
    kept = pc.nms_expected(case)
    assert kept.max() < case.n and not np.array_equal(case.cand_idx[kept], kept)     # positions, not source rows


# ------------------------------------------------------------------------------------------------ select
@pytest.mark.parametrize("name", pc.select_case_names())
def test_select_cases(name):
    case = pc.select_case(name)
    idx, k = pc.select_expected(case)
    assert np.array_equal(idx, np.sort(idx))
    if case.want_k is not None:
        assert k == case.want_k
    if case.want_count is not None:
        assert len(idx) == case.want_count
    if case.fixed is None:
        assert len(idx) <= case.keep


@pytest.mark.parametrize("n", pc.SELECT_SIZES)
def test_select_size_family(n):
    case = pc.select_case("size_%d" % n)
    idx, k = pc.select_expected(case)
    assert case.n == n and (k >= 1 or n == 1)
    nblocks = (n + pc.SEL_BLOCK - 1) // pc.SEL_BLOCK
    blocks = set((idx // pc.SEL_BLOCK).tolist())
    assert blocks == {0, nblocks - 1} | {b for b in (1023, 1024, 2048) if b < nblocks}
    assert idx[0] == 0 and idx[-1] == n - 1
    assert (nblocks + 1023) // 1024 == {1048577: 2, 2097157: 3}.get(n, 1)            # passes of the block scan


def test_select_pattern_family():
    s, cnt = pc.pattern_scores()
    idx, _ = pc.select_expected(pc.select_case("patterns_adaptive"))
    assert np.array_equal(idx, pc.select_expected(pc.select_case("patterns_fixed"))[0])
    per_block = np.bincount(idx // pc.SEL_BLOCK, minlength=7).tolist()
    assert per_block == [1024, 0, 512, 16, 16, 1024, 1] and cnt == sum(per_block)
    assert np.all(idx[idx // pc.SEL_BLOCK == 3] % 64 == 0) and np.all(idx[idx // pc.SEL_BLOCK == 4] % 64 == 63)
    assert idx[-1] == pc.PATTERN_N - 1 and pc.PATTERN_N % pc.SEL_BLOCK != 0


def test_select_keep_boundary_family():
    T = pc.thr_table(1e-7)
    full, plus = pc.select_case("keep_exactly_full"), pc.select_case("keep_plus_one")
    for case, above3 in ((full, 64), (plus, 65)):
        s = case.scores()
        assert case.keep == 64 and (s > T[3]).sum() == above3 and (s > T[2]).sum() > 64
        assert (s == T[3]).sum() >= 20 and (s == T[4]).sum() >= 1                # equal to a threshold: not above it
    assert pc.select_expected(full) [1] == 3 and len(pc.select_expected(full)[0]) == 64
    assert pc.select_expected(plus)[1] == 4 and len(pc.select_expected(plus)[0]) == 30
    assert not np.any(full.scores()[pc.select_expected(full)[0]] == T[3])


def test_select_edge_families():
    T = pc.thr_table(1e-25)
    assert np.isinf(T[-1]) and np.isfinite(T[-2]) and len(T) == 319 and T[-2] < 3e38
    case = pc.select_case("too_many_equal")
    assert (case.scores() == np.float32(0.9)).sum() > case.keep and len(pc.select_expected(case)[0]) == 0
    case = pc.select_case("inf_above_last_finite")
    assert np.all(np.isinf(case.scores()[pc.select_expected(case)[0]]))
    case = pc.select_case("nan_never_selected")
    s = case.scores()
    assert np.isnan(s).sum() >= 10 and not np.isnan(s[pc.select_expected(case)[0]]).any()
    case = pc.select_case("strided_column")
    assert (case.stride, case.offset) == (3, 1) and np.shares_memory(case.scores(), case.buf)
    for col in (0, 2):
        assert len(pc.select_ref(case.buf[col::3], case.start, case.keep)) != 77
    case = pc.select_case("fixed_over_keep")
    assert len(pc.select_expected(case)[0]) > case.keep and 5 not in pc.select_expected(case)[0]
    assert case.scores()[5] == np.float32(0.05)


@pytest.mark.parametrize("name", ["size_4097", "nan_never_selected"])
def test_select_ref_is_the_oracle_loop(name):
    """At keep = 10000, the reference's constant, select_ref is oracle.boxes.adaptive_threshold."""
    case = pc.select_case(name)
    s = np.concatenate([case.scores(), np.random.default_rng(5).random(30000).astype(np.float32)])   # > 10000 above t_0
    mask = oboxes.adaptive_threshold(torch.from_numpy(s), case.start).numpy()
    idx, k = pc.select_ref_k(s, case.start, 10000)
    assert k >= 1 and np.array_equal(idx, np.flatnonzero(mask))


# ------------------------------------------------------------------------------------------------ the other families
def test_rowmax_and_decode_select_inputs():
    cases = dict(pc.rowmax_cases())
    v, a = pc.rowmax_ref(cases["ties"])
    assert (np.sum(cases["ties"] == v[:, None], axis=1) > 1).sum() > 100            # rows with several maxima
    t = torch.from_numpy(cases["ties"]).max(dim=1)
    assert np.array_equal(a, t.indices.numpy())                                      # the reference's max(dim=1): first index
    assert cases["one_class"].shape == (257, 1) and np.all(pc.rowmax_ref(cases["max_in_last_column"])[1] == 7)
    assert cases["one_row"].shape[0] == 1 and pc.rowmax_ref(cases["one_row"])[1][0] == 1
    v, a = pc.rowmax_ref(cases["row_of_minus_inf"])
    assert v[2] == -np.inf and a[2] == 0 and a[3] == 0
    anchors, reg, cls = pc.decode_select_inputs()
    total = reg.shape[0] * reg.shape[1]
    for count in pc.DDS_COUNTS:
        sel = pc.decode_select_sel(count, total)
        assert len(sel) == count and np.all(np.diff(sel) > 0)
    assert pc.decode_select_sel(257, total)[[0, -1]].tolist() == [0, total - 1]
    assert pc.DDS_COUNTS == (0, 1, 257, pc.DDS_MAX) and pc.DDS_MAX % 256 != 0 and pc.DDS_MAX > 256


def test_wrapper_inputs():
    cls, boxes = pc.p2d_inputs(12000, 13000)
    assert (cls[0, :, 0] > np.float32(0.05)).sum() == 12000 and 0 < (cls[0, :, 1] > np.float32(0.05)).sum() < 100
    cls, _ = pc.p2d_inputs(16385, 17000)
    assert (cls[0, :, 0] > np.float32(0.05)).sum() == 16385
    cls, _ = pc.psingle_inputs(3, empty_class=1)
    assert not np.any(cls[0, :, 1] > np.float32(1e-25)) and np.all(cls[0, :, 0] > 0)
    anchors, reg, cls = pc.detect_inputs()
    idx, k = pc.select_ref_k(cls.reshape(-1, pc.DETECT_C).max(axis=1), 1e-7, 10000)
    assert k == 0 and len(idx) == pc.DETECT_COUNT == 10000 and idx[-1] >= pc.DETECT_A      # exactly full, both images


def test_tracker_inputs():
    for name, boxes, scores, num, den in pc.tracker_cases():
        det = pc.corners_from_boxes(boxes)
        env = np.stack((det[:, :, 0].min(1), det[:, :, 1].min(1), det[:, :, 0].max(1), det[:, :, 1].max(1)), axis=1)
        assert det.shape == (len(boxes), 8, 2) and np.array_equal(env, boxes) and np.array_equal(det, np.round(det))
        from oracle import tracker_post as otp
        st = pc.states_from_boxes(boxes)
        assert np.array_equal(otp.space_boxes(st).numpy(), boxes) and len(np.unique(st[:, 5])) == 2
        want = pc.nms_int_ref(boxes, scores, None, num, den)
        assert np.array_equal(otp.im_nms(torch.from_numpy(det), torch.from_numpy(scores), num / den,
                                         groups=torch.zeros(len(boxes))).numpy(), want)
        assert np.array_equal(otp.space_nms(st, torch.from_numpy(scores), num / den).numpy(), want)
    assert len(np.unique(pc.tracker_cases()[0][2])) == 5

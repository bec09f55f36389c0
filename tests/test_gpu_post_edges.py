"""The eval tail's kernels (rn_rowmax, rn_threshold_select, rn_decode_dir_select, rn_nms of csrc/boxes.hip) at their
edges against the plain references of tests/post_cases.py, through the C ABI and through ops.nms / postprocess_* /
detect_* / mc3d_post.  tests/test_post_cases_host.py proves the cases and the references.  Everything is integer- or
bit-exact: this file has no tolerances."""
import types

import numpy as np
import pytest
import torch

import post_cases as pc
from oracle import boxes as oboxes
from oracle import tracker_post as otp

pytestmark = pytest.mark.gpu

GUARD = 256                          # bytes of 0xA5 after the workspace the library asked for


@pytest.fixture(scope="module")
def lib(dev):
    from retinanet_mi355x import _hip
    lib = _hip.load()
    assert lib.rn_check_device() == 0
    return lib


@pytest.fixture(scope="module")
def ops(lib):
    from retinanet_mi355x import ops as _ops
    return _ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _workspace(lib, n_scores, max_cand, dev, fill):
    nbytes = int(lib.rn_post_workspace_bytes(n_scores, max_cand))
    ws = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device=dev)
    ws[nbytes:] = 0xA5
    return ws, nbytes


def _guard_intact(ws, nbytes):
    return bool((ws[nbytes:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ select
def run_select(lib, case, ws, dev):
    """-> (count, sel_idx as it is left on the device).  sel_idx is pre-filled with -1."""
    buf = torch.from_numpy(case.buf).to(dev)
    assert case.offset + (case.n - 1) * case.stride < buf.numel()
    room = (case.n if case.fixed is not None else case.keep) + 64
    sel = torch.full((room,), -1, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = lib.rn_threshold_select(buf.data_ptr() + 4 * case.offset, case.n, case.stride, float(case.start), case.keep,
                                 -1.0 if case.fixed is None else float(case.fixed), ws.data_ptr(), count.data_ptr(),
                                 sel.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return int(count.item()), sel.cpu().numpy()


def check_select(lib, case, ws, dev):
    want, _ = pc.select_expected(case)
    count, sel = run_select(lib, case, ws, dev)
    assert count == len(want), (case.name, count, len(want))
    assert np.array_equal(sel[:count], want)
    assert np.all(sel[count:] == -1)


@pytest.mark.parametrize("name", pc.select_case_names())
def test_threshold_select(lib, dev, name):
    case, again = pc.select_case(name), pc.select_case("keep_exactly_full")
    ws, nbytes = _workspace(lib, max(case.n, again.n), 1, dev, 0xFF)
    check_select(lib, case, ws, dev)
    assert _guard_intact(ws, nbytes)
    check_select(lib, again, ws, dev)                    # same workspace, other scores: the histogram starts from zero
    check_select(lib, case, ws, dev)
    assert _guard_intact(ws, nbytes)


# ------------------------------------------------------------------------------------------------ NMS
def run_nms(lib, case, max_cand, ws, dev):
    """rn_nms with the candidate count in device memory, as the post-process functions call it.
    -> (keep_count, keep as it is left on the device).  keep is pre-filled with -1."""
    assert case.n <= max_cand <= 16384
    boxes = torch.from_numpy(case.boxes).to(dev)
    scores = torch.from_numpy(case.scores).to(dev)
    cand = torch.from_numpy(case.cand_idx).to(dev)
    assert int(case.cand_idx.max()) < case.boxes.shape[0] and int(case.cand_idx.max()) * case.score_stride < case.scores.shape[0]
    cats = None if case.cats is None else torch.from_numpy(case.cats).to(dev)
    count = torch.tensor([case.n, -7], dtype=torch.int32, device=dev)
    keep = torch.full((max_cand,), -1, dtype=torch.int32, device=dev)
    rc = lib.rn_nms(boxes.data_ptr(), case.box_stride, case.box_col, scores.data_ptr(), case.score_stride, cand.data_ptr(),
                    None if cats is None else cats.data_ptr(), count[0:1].data_ptr(), max_cand, float(case.thr),
                    ws.data_ptr(), keep.data_ptr(), count[1:2].data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return int(count[1].item()), keep.cpu().numpy()


def check_nms(lib, case, max_cand, ws, dev, what):
    want = pc.nms_expected(case)
    kc, keep = run_nms(lib, case, max_cand, ws, dev)
    assert kc == len(want), (case.name, what, kc, len(want))
    assert np.array_equal(keep[:kc], want), (case.name, what)
    assert np.all(keep[kc:] == -1), (case.name, what)


@pytest.mark.parametrize("name", pc.nms_case_names())
def test_nms(lib, dev, name):
    case = pc.nms_case(name)
    # max_candidates = n, workspace full of 0xFF: the scan reads mask words no kernel wrote
    ws, nbytes = _workspace(lib, 1, case.n, dev, 0xFF)
    check_nms(lib, case, case.n, ws, dev, "max_candidates = n")
    assert _guard_intact(ws, nbytes)
    if case.n == 16384:
        return
    # max_candidates > n, the way the post-process functions call it
    big = 10000 if case.n < 10000 else 16384
    ws, nbytes = _workspace(lib, 1, big, dev, 0xFF)
    check_nms(lib, case, big, ws, dev, "max_candidates = %d" % big)
    # ... and straight after a larger problem on the same workspace
    larger = pc.nms_case("size_4097" if case.n < 4097 else "size_16384")
    if larger.n <= big:
        check_nms(lib, larger, big, ws, dev, "the larger problem")
        check_nms(lib, case, big, ws, dev, "after a larger problem")
    assert _guard_intact(ws, nbytes)


def test_ops_nms(ops, dev):
    assert ops.nms(torch.zeros((0, 4), device=dev), torch.zeros(0, device=dev), 0.5).shape == (0,)
    with pytest.raises(RuntimeError, match="at most"):                   # refused on the host, nothing is launched
        ops.nms(torch.zeros((16385, 4), device=dev), torch.zeros(16385, device=dev), 0.5)
    names = ["size_16384", "batched_18", "degenerate_negative_batched", "ties_signed_zeros", "chain"]
    for case in [pc.nms_case(n) for n in names + ["thr_" + r[0] for r in pc.THRESHOLD_PAIRS]]:
        idxs = None if case.cats is None else torch.from_numpy(case.cats.astype(np.int64)).to(dev)
        got = ops.nms(torch.from_numpy(case.cand_boxes().copy()).to(dev), torch.from_numpy(case.cand_scores().copy()).to(dev),
                      case.thr, idxs)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), pc.nms_expected(case)), case.name
    case = pc.nms_case("batched_18")                                      # without idxs the categories suppress each other
    got = ops.nms(torch.from_numpy(case.cand_boxes().copy()).to(dev), torch.from_numpy(case.cand_scores().copy()).to(dev), 0.5)
    assert np.array_equal(got.cpu().numpy(), pc.nms_int_ref(case.cand_boxes(), case.cand_scores(), None, 1, 2))
    assert got.numel() == pc.BATCHED_BASE + 1


# ------------------------------------------------------------------------------------------------ wrappers
def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w.numpy())


def test_postprocess_2d_between_keep_and_nms_max(ops, dev):
    cls, boxes = pc.p2d_inputs(12000, 13000)
    cls, boxes = torch.from_numpy(cls), torch.from_numpy(boxes)
    want = oboxes.postprocess_2d(cls, boxes)
    assert 10000 < int((cls[0, :, 0] > 0.05).sum()) < 16384 and want[0].numel() > 5000
    _same(ops.postprocess_2d(cls.to(dev), boxes.to(dev)), want)


def test_postprocess_2d_over_nms_max_raises(ops, dev):
    cls, boxes = pc.p2d_inputs(16385, 17000)
    with pytest.raises(RuntimeError, match="more than 16384"):           # read back and refused before any NMS launch
        ops.postprocess_2d(torch.from_numpy(cls).to(dev), torch.from_numpy(boxes).to(dev))


@pytest.mark.parametrize("C,empty", [(1, None), (3, 1)])
def test_postprocess_single_class_edges(ops, dev, C, empty):
    cls, boxes = pc.psingle_inputs(C, empty_class=empty)
    cls, boxes = torch.from_numpy(cls), torch.from_numpy(boxes)
    want = oboxes.postprocess_single(cls, boxes)
    assert sorted(set(want[1].tolist())) == [c for c in range(C) if c != empty]
    _same(ops.postprocess_single(cls.to(dev), boxes.to(dev)), want)


def test_detect_multi_with_the_candidate_list_exactly_full(ops, dev):
    anchors, reg, cls = [torch.from_numpy(a).to(dev) for a in pc.detect_inputs()]
    got = ops.detect_multi(cls, reg, anchors)
    want = ops.postprocess_multi(cls, ops.decode_dir(anchors, reg))
    assert 1000 < got[0].numel() < pc.DETECT_COUNT and set(got[3].tolist()) == {0, 1}
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.cpu().numpy(), w.cpu().numpy())


# ------------------------------------------------------------------------------------------------ rowmax, decode_dir_select
@pytest.mark.parametrize("name,cls", pc.rowmax_cases(), ids=[c[0] for c in pc.rowmax_cases()])
def test_rowmax(lib, dev, name, cls):
    n, C = cls.shape
    x = torch.from_numpy(cls).to(dev)
    scores = torch.full((n + 8,), -5.0, device=dev)
    classes = torch.full((n + 8,), -5, dtype=torch.int64, device=dev)
    assert lib.rn_rowmax(x.data_ptr(), n, C, scores.data_ptr(), classes.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    v, a = pc.rowmax_ref(cls)
    assert np.array_equal(scores.cpu().numpy()[:n], v) and np.array_equal(classes.cpu().numpy()[:n], a)
    assert bool((scores[n:] == -5).all()) and bool((classes[n:] == -5).all())


DDS_MAX = pc.DDS_MAX


@pytest.mark.parametrize("count", pc.DDS_COUNTS)
def test_decode_dir_select(lib, ops, dev, count):
    anchors, reg, cls = pc.decode_select_inputs()
    B, A, C = cls.shape
    sel = pc.decode_select_sel(count, B * A)
    c = 2                                                                # scores: class 2, read through stride C
    anc_d, reg_d, cls_d = [torch.from_numpy(a).to(dev) for a in (anchors, reg, cls)]
    sel_d = torch.full((DDS_MAX,), B * A - 1, dtype=torch.int32, device=dev)
    sel_d[:count] = torch.from_numpy(sel).to(dev)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    boxes = torch.full((DDS_MAX, 20), -1.0, device=dev)
    cscore = torch.full((DDS_MAX,), -1.0, device=dev)
    cimage = torch.full((DDS_MAX,), -1, dtype=torch.int32, device=dev)
    rc = lib.rn_decode_dir_select(anc_d.data_ptr(), reg_d.data_ptr(), A, cls_d.data_ptr() + 4 * c, C, sel_d.data_ptr(),
                                  cnt.data_ptr(), DDS_MAX, boxes.data_ptr(), cscore.data_ptr(), cimage.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    full = ops.decode_dir(anc_d, reg_d).reshape(B * A, 20).cpu().numpy()
    assert np.array_equal(boxes.cpu().numpy()[:count].view(np.uint32), full[sel].view(np.uint32))     # bit for bit
    assert np.array_equal(cscore.cpu().numpy()[:count], cls.reshape(B * A, C)[sel, c])
    assert np.array_equal(cimage.cpu().numpy()[:count], sel // A)
    assert bool((boxes[count:] == -1).all()) and bool((cscore[count:] == -1).all()) and bool((cimage[count:] == -1).all())


# ------------------------------------------------------------------------------------------------ tracker
@pytest.mark.parametrize("which", [0, 1], ids=["ties", "chain"])
def test_tracker_im_nms_and_space_nms(ops, dev, which):
    """mc3d_post.im_nms (envelopes shifted by 10 000) and space_nms (road-plane footprints) run the same kernel; integer
    corners keep both exact."""
    import mc3d_post
    name, boxes, scores, num, den = pc.tracker_cases()[which]
    me = types.SimpleNamespace()
    det, sc = torch.from_numpy(pc.corners_from_boxes(boxes)), torch.from_numpy(scores)
    groups = torch.zeros(len(boxes), dtype=torch.int64)
    want = pc.nms_int_ref(boxes, scores, None, num, den)
    for g in (groups, None):
        ref = otp.im_nms(det, sc, threshold=num / den, groups=g)
        got = mc3d_post.im_nms(me, det.to(dev), sc.to(dev), threshold=num / den, groups=None if g is None else g.to(dev))
        assert np.array_equal(got.cpu().numpy(), ref.numpy()) and np.array_equal(ref.numpy(), want)
    st = torch.from_numpy(pc.states_from_boxes(boxes))
    ref = otp.space_nms(st, sc, threshold=num / den)
    got = mc3d_post.space_nms(me, st.to(dev), sc.to(dev), threshold=num / den)
    assert np.array_equal(got.cpu().numpy(), ref.numpy()) and np.array_equal(ref.numpy(), want)

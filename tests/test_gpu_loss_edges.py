"""The fused loss (focal_kernel and its epilogue, csrc/focal_loss.hip) per element against the float64 reference of
tests/loss_cases.py, at the shapes where the kernel takes another path: a full queue of positives, waves that walk three
units, G > 512 and B > 256 in the epilogue, label rows past the 64 held in registers, small and ragged A, IoU exactly on
the 0.4 / 0.5 thresholds, values exactly on the clamp bounds; then that two runs agree bit for bit and that a workspace
can be used again.  tests/test_loss_cases_host.py proves the cases and that the comparison rejects wrong kernels.

dcls is held per element to |ref| (8 R + cond) with R the float32 oracle's own excess on the case, dreg per positive row
and column group to 4 times the oracle's worst row, the losses to 4 times the oracle's error (floor 2^-22); exact zeros
and the integer outputs of ops.assign are exact.  The figures are printed before they are asserted."""
import os

import numpy as np
import pytest
import torch

import loss_cases as lc

# the cases derive G from the kernel's own RN_FOCAL_RESIDENT; a tuning sweep that overrides it reaches other paths
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("RN_FOCAL_RESIDENT" in os.environ, reason="the cases assume the built-in RN_FOCAL_RESIDENT")]


@pytest.fixture(scope="module")
def ops(dev):
    from retinanet_mi355x import ops as _ops, _hip
    assert _hip.load().rn_check_device() == 0
    return _ops


def run(ops, dev, case):
    """-> (losses, dcls, dreg) as numpy, gradient of W_LOSS . losses, through ops.focal_loss and its autograd node."""
    c = case.cls.to(dev).requires_grad_(True)
    r = case.reg.to(dev).requires_grad_(True)
    out = ops.focal_loss(c, r, case.anchors.to(dev), case.ann.to(dev), case.directional)
    sum(w * o for w, o in zip(lc.W_LOSS, out)).sum().backward()
    return np.array([float(o.detach()) for o in out]), c.grad.cpu().numpy(), r.grad.cpu().numpy()


def check(ops, dev, fam, name):
    """The fused loss inside the envelopes of the case's family and ops.assign bit-exact, on one case."""
    case = lc.get(fam, name)
    got = run(ops, dev, case)
    bad, fig = lc.check(got, case, fam)
    ofig = lc.family_figures(fam)
    print("%s: dcls excess R %.3g (oracle32 of the case %.3g) | dreg rows %s (oracle32 %s) | losses rel %s (oracle32 %s)"
          % (name, fig["R"], ofig["R", case.directional], np.array2string(fig["dreg"], precision=3),
             np.array2string(ofig["dreg", case.directional], precision=3), np.array2string(fig["loss"], precision=3),
             np.array2string(ofig["loss", case.directional], precision=3)))
    assert not bad, (name, bad)
    check_assign(ops, dev, case)
    return case, got


def check_assign(ops, dev, case):
    iou, arg, st = [t.cpu() for t in ops.assign(case.anchors.to(dev), case.ann.to(dev), case.directional)]
    for j, a in enumerate(lc.assignment(case)):
        if a is None:
            assert int(st[j].abs().sum()) == 0 and int((arg[j] != -1).sum()) == 0 and float(iou[j].abs().max()) == 0
            continue
        assert torch.equal(iou[j], a[0]) and torch.equal(arg[j].long(), a[4]) and torch.equal(st[j].long(), a[2]), (case.name, j)


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("fam", ["queue_full", "queue_full_2d"])
def test_queue_full(ops, dev, fam):
    """Images whose every anchor is positive: each wave queues QCAP positives in two units, breaks out of the pipelined
    loop, drains and re-issues its third unit unprimed."""
    check(ops, dev, fam, fam)


@pytest.mark.parametrize("name", lc.names("tail_sizes"))
def test_tail_sizes(ops, dev, name):
    check(ops, dev, "tail_sizes", name)


@pytest.mark.parametrize("name", lc.names("many_labels"))
def test_many_labels(ops, dev, name):
    check(ops, dev, "many_labels", name)


def test_too_many_labels_raise(ops, dev):
    case = lc.get("many_labels", "labels_N256_dir")
    for directional, c in ((True, case), (False, lc.get("many_labels", "labels_N256_2d"))):
        ann = torch.cat((c.ann, c.ann[:, :1]), 1).to(dev)
        assert ann.shape[1] == lc.MAX_GT + 1
        with pytest.raises(RuntimeError, match="RN_ETOOMANY"):
            ops.focal_loss(c.cls.to(dev), c.reg.to(dev), c.anchors.to(dev), ann, directional)
        with pytest.raises(RuntimeError, match="RN_ETOOMANY"):
            ops.assign(c.anchors.to(dev), ann, directional)


def test_no_label_rows_2d(ops, dev):
    """ann of shape [B,0,5]: every image is empty, the classification loss is the raw sum and nothing else moves."""
    src = lc.get("many_labels", "labels_N1_2d")
    case = lc.Case("labels_N0_2d", False, src.cls, src.reg, src.anchors, src.ann[:, :0])
    assert case.N == 0 and all(a is None for a in lc.assignment(case))
    got = run(ops, dev, case)
    ref, orc = lc.reference(case), lc.oracle_figures(case)
    bad, fig = lc.within(got, case, orc["R"], orc["dreg"], orc["loss"])
    print("labels_N0_2d: dcls excess R %.3g (oracle32 %.3g) | losses rel %s (oracle32 %s)" % (fig["R"], orc["R"], fig["loss"], orc["loss"]))
    assert not bad, bad
    assert got[0][1] == 0 and not got[2].any() and ref.losses[1] == 0
    check_assign(ops, dev, case)


@pytest.mark.parametrize("name", lc.names("thresholds"))
def test_thresholds(ops, dev, name):
    """IoU exactly 1/2 is positive, one ulp below it and exactly 0.4f are ignored, one ulp below 0.4f is negative: in
    rn_assign and in the fused kernel, whose ignored anchors leave dcls exactly 0."""
    case, got = check(ops, dev, "thresholds", name)
    for j in range(case.B):
        for i, kind in enumerate(case.kinds):
            row = got[1][j, case.first + i]
            assert bool((row == 0).all()) == (lc.TH_STATE[kind] == -1), (kind, row)
            assert bool(got[2][j, case.first + i].any()) == (lc.TH_STATE[kind] == 1), kind


@pytest.mark.parametrize("name", lc.names("clamp_edges"))
def test_clamp_edges(ops, dev, name):
    """x on a clamp bound or one ulp inside passes gradient, one ulp outside, 0 and 1 do not -- on negatives, on the
    positive class, beside it and in the packed fast path: the zero mask is the float32 oracle's, bit for bit."""
    case, got = check(ops, dev, "clamp_edges", name)
    assert np.array_equal(got[1] != 0, lc.oracle32(case).dcls != 0)
    for where, j, a, col, v in case.plan:
        assert (got[1][j, a, col] != 0) == (v in (0, 2, 3, 4)), (where, v)


def test_one_image_full_size(ops, dev):
    """B = 1 at 1080p: G = 768, the second round of focal_finalize_image's loop over the partials."""
    check(ops, dev, "one_image_full_size", "one_image_1080p")


@pytest.mark.parametrize("name", lc.names("big_batch"))
def test_big_batch(ops, dev, name):
    """B > 256: the strided loops of focal_finalize_batch; B > 96: the G >= 8 floor of focal_groups."""
    check(ops, dev, "big_batch", name)


def test_batch_past_the_limit_raises(ops, dev):
    src = lc.get("big_batch", "batch_B300_A128_2d")
    B = lc.MAX_B + 1
    rep = lambda t: t.repeat(4, 1, 1)[:B].to(dev)
    with pytest.raises(RuntimeError, match="RN_EINVAL"):
        ops.focal_loss(rep(src.cls), rep(src.reg), src.anchors.to(dev), rep(src.ann), False)


@pytest.mark.parametrize("name", lc.names("fast_path_values"))
def test_fast_path_values(ops, dev, name):
    """The golden case of test_gpu_ops.py under the per-element envelope: the packed fast path's values count."""
    check(ops, dev, "fast_path_values", name)


# ------------------------------------------------------------------------------------------------ runs and workspaces
def test_runs_are_bit_reproducible(ops, dev):
    case = lc.get("queue_full", "queue_full")
    a, b = run(ops, dev, case), run(ops, dev, case)
    assert not lc.check(a, case, "queue_full")[0]                                  # finite and right, not merely the same
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def _raw(ops, dev, case, ws):
    """rn_focal_loss_fwd / _bwd on the workspace given, the way modules._NetFn calls them."""
    from retinanet_mi355x import _hip
    lib = _hip.load()
    cls, reg, anc, ann = (t.to(dev).contiguous() for t in (case.cls, case.reg, case.anchors[0], case.ann))
    B, A, C = cls.shape
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    _hip.check(lib.rn_focal_loss_fwd(cls.data_ptr(), reg.data_ptr(), anc.data_ptr(), _hip.ptr(ann), B, A, C, ann.shape[1],
                                     int(case.directional), ws.data_ptr(), losses.data_ptr(), _hip.stream()), "rn_focal_loss_fwd")
    torch.cuda.synchronize()
    head = ws[:lib.rn_focal_workspace_zero_bytes(B)].cpu()
    g = torch.tensor(lc.W_LOSS, dtype=torch.float32, device=dev)
    dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)
    _hip.check(lib.rn_focal_loss_bwd(cls.data_ptr(), reg.data_ptr(), anc.data_ptr(), _hip.ptr(ann), B, A, C, ann.shape[1],
                                     int(case.directional), ws.data_ptr(), g.data_ptr(), dcls.data_ptr(), dreg.data_ptr(),
                                     _hip.stream()), "rn_focal_loss_bwd")
    torch.cuda.synchronize()
    return (losses.cpu(), dcls.cpu(), dreg.cpu()), head


def test_workspace_is_left_ready_for_the_next_forward(ops, dev):
    """Two forwards on one workspace: the counters are zero after each, and the second call's losses and gradients are
    those of a fresh workspace, bit for bit."""
    x, y = lc.workspace_pair()
    assert (x.B, x.A, x.C, x.N) == (y.B, y.A, y.C, y.N) and not torch.equal(x.cls, y.cls)
    ws = ops.focal_workspace(x.B, x.A, dev)
    got_x, head_x = _raw(ops, dev, x, ws)
    got_y, head_y = _raw(ops, dev, y, ws)
    fresh_y, _ = _raw(ops, dev, y, ops.focal_workspace(y.B, y.A, dev))
    fresh_x, _ = _raw(ops, dev, x, ops.focal_workspace(x.B, x.A, dev))
    assert head_x.numel() == 64 + 64 and int(head_x.abs().sum()) == 0 and int(head_y.abs().sum()) == 0
    for a, b in zip(got_y, fresh_y):
        assert torch.equal(a, b)
    for a, b in zip(got_x, fresh_x):
        assert torch.equal(a, b)
    assert not torch.equal(got_x[0], got_y[0])
    bad, _ = lc.check([t.numpy() for t in got_x], x, "fast_path_values")           # x is that family's directional case
    assert not bad, bad

"""The bf16 weight gradient (csrc/conv_wgrad_bf16.hip) on every path its launchers can take -- the XCD order with a padding group, the
plain order, pixel-table reuse, slices that end on a K-step and one pixel past it, the edges of the matrix, stride 2, grouped launches
with padded ranges -- with integer inputs (tests/wgrad_bf16_cases.py): every product and partial sum is exact in fp32 whatever the order
of the atomics, so dw and colsum must EQUAL the float64 reference.  No tolerance.  The plans the cases are named for are pinned on the
host by tests/test_wgrad_plan_host.py; only entry points of the C ABI are used."""
import pytest
import torch

import wgrad_bf16_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv(dev):
    from retinanet_mi355x import conv
    return conv


def operands(c, dev):
    """-> (x, dy as guarded bf16 device views with their buffers, float64 dw [Cout, Kflat] and colsum references on the device)."""
    x, dy = bc.inputs(c)
    xb, xv = bc.guarded(x.bfloat16(), dev)
    gb, gv = bc.guarded(dy.bfloat16(), dev)
    assert torch.equal(xv.float().cpu(), x) and torch.equal(gv.float().cpu(), dy)        # integers of {-2 .. 2}: bf16 holds them exactly
    dw_ref, cs_ref = bc.reference(xv.float(), gv.float(), c)
    return (xb, xv), (gb, gv), dw_ref, cs_ref


def check(c, dw_buf, dw, cs_buf, cs, dw0, cs0, dw_ref, cs_ref):
    kf = bc.kflat(c)
    assert bc.guards_intact(dw_buf) and bc.guards_intact(cs_buf)
    assert bool((dw[:, kf:] == bc.SENTINEL).all()), "columns Kflat .. Kpad written"
    want = dw0[:, :kf].double().to(dw.device) + dw_ref
    assert float(dw_ref.abs().max()) > 0 and float(want.abs().max()) < 2 ** 24
    assert torch.equal(dw[:, :kf].double(), want), "dw: %d elements differ, max %g" % (
        int((dw[:, :kf].double() != want).sum()), float((dw[:, :kf].double() - want).abs().max()))
    want_cs = cs0.double().to(cs.device) + cs_ref
    assert torch.equal(cs.double(), want_cs), "colsum: max difference %g" % float((cs.double() - want_cs).abs().max())


@pytest.mark.parametrize("c", bc.CASES, ids=lambda c: c.name)
def test_single_launch_is_exact(cv, dev, c):
    (xb, xv), (gb, gv), dw_ref, cs_ref = operands(c, dev)
    dw0, cs0 = bc.start_dw(c)
    dw_buf, dw = bc.guarded(dw0, dev)
    cs_buf, cs = bc.guarded(cs0, dev)
    cv.wgrad_bf16(gv, xv, dw, c.cout, c.k, c.stride, c.pad, colsum=cs)
    torch.cuda.synchronize()
    check(c, dw_buf, dw, cs_buf, cs, dw0, cs0, dw_ref, cs_ref)
    # without column sums: the same dw
    dw_buf2, dw2 = bc.guarded(dw0, dev)
    cv.wgrad_bf16(gv, xv, dw2, c.cout, c.k, c.stride, c.pad)
    torch.cuda.synchronize()
    assert bc.guards_intact(dw_buf2) and torch.equal(dw2, dw)
    assert bc.guards_intact(xb) and bc.guards_intact(gb)


@pytest.mark.parametrize("name", sorted(bc.GROUPS))
def test_grouped_launch_is_the_exact_sum(cv, dev, name):
    """One grouped launch == the sum of the float64 references of its levels == the sum of the single launches, element for element."""
    cs_, _ = bc.group_cases(name)
    c0 = cs_[0]
    xs, gs, dw_ref, cs_ref = [], [], 0, 0
    for c in cs_:
        (_, xv), (_, gv), r, s = operands(c, dev)
        xs.append(xv)
        gs.append(gv)
        dw_ref, cs_ref = dw_ref + r, cs_ref + s
    dw0, cs0 = bc.start_dw(c0)
    dw_buf, dw = bc.guarded(dw0, dev)
    cs_buf, cs = bc.guarded(cs0, dev)
    cv.wgrad_bf16_grouped(gs, xs, dw, c0.cout, c0.k, c0.stride, c0.pad, colsum=cs)
    torch.cuda.synchronize()
    check(c0, dw_buf, dw, cs_buf, cs, dw0, cs0, dw_ref, cs_ref)
    dw_buf1, dw1 = bc.guarded(dw0, dev)
    cs_buf1, cs1 = bc.guarded(cs0, dev)
    for g, x, c in zip(gs, xs, cs_):
        cv.wgrad_bf16(g, x, dw1, c.cout, c.k, c.stride, c.pad, colsum=cs1)
    torch.cuda.synchronize()
    assert bc.guards_intact(dw_buf1) and bc.guards_intact(cs_buf1)
    assert torch.equal(dw1, dw) and torch.equal(cs1, cs)

"""CPU: what tests/wgrad_cases.py gives tests/test_gpu_wgrad_paths.py is right -- the float64 reference against torch autograd, the one-hot
closed form against the reference, the case tables against the launcher's own plan (rn_conv_wgrad_plan is host code)."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as wc

MODES = ("native", "split", "split3")


@pytest.fixture(scope="module")
def conv():
    from retinanet_mi355x import _hip, conv as _conv
    import os
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    before = _conv.get_fp32_mfma()
    yield _conv
    _conv.set_fp32_mfma(before)


def plans(conv, c, det=0):
    out = {}
    for mode in MODES:
        conv.set_fp32_mfma(mode)
        out[mode] = conv.wgrad_plan(c.ldy, 1, 0, 0, 0, 0, wc.geom(c), have_amax=mode == "split3", det=det)
    return out


TINY = [
    wc.case("tiny-3x3-s1", 8, 7, 3, 1, 1, 2, 6, 7, ldy=8),
    wc.case("tiny-3x3-s2-odd", 8, 9, 3, 2, 1, 2, 7, 9, ldy=12),
    wc.case("tiny-1x1-s2", 12, 7, 1, 2, 0, 2, 5, 6, ldy=8),
    wc.case("tiny-7x7-s2-kw8", 4, 10, 7, 2, 3, 2, 13, 15, kw=8, ldy=12),
    wc.case("tiny-3x3-relu", 8, 5, 3, 1, 1, 2, 6, 7, ldy=8, relu=True),
]


@pytest.mark.parametrize("c", TINY, ids=lambda c: c.name)
def test_reference_against_autograd(c):
    """The kh x kw gradient is that of a kh x kw convolution without padding over x padded by (pad, pad + kw - k) -- the extra tap of kw = 8
    included --, float64 autograd, 1e-12 of the max magnitude."""
    x, dy = wc.inputs(c)
    ho, wo = wc.out_hw(c)
    xd = x.double().permute(0, 3, 1, 2)
    if c.relu:
        xd = xd.clamp_min(0)
    xd = F.pad(xd, (c.pad, c.pad + c.kw - c.k, c.pad, c.pad))
    w = torch.zeros((c.cout, c.cin, c.k, c.kw), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xd, w, None, c.stride, 0)
    assert tuple(y.shape) == (c.N, c.cout, ho, wo)
    g = dy[..., :c.cout].double().permute(0, 3, 1, 2)
    (y * g).sum().backward()
    dw, cs = wc.reference(x, dy, c)
    want = w.grad.permute(0, 2, 3, 1)
    assert float((dw - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((cs - g.sum(dim=(0, 2, 3))).abs().max()) <= 1e-12 * float(cs.abs().max())


@pytest.mark.parametrize("c", TINY[:4], ids=lambda c: c.name)
def test_closed_form_against_the_dense_reference(c):
    """One value of dy at a corner, an edge, an interior pixel, the last pixel of image 0 and the first of image 1: the closed form is the
    reference of that dy, bit for bit in float64 (one product per element), and zero in every other row."""
    ho, wo = wc.out_hw(c)
    x, _ = wc.inputs(c)
    px = [0, wo - 1, (ho // 2) * wo + wo // 2, ho * wo - 1, ho * wo, wc.pixels(c) - 1]
    hot = [(p, i, 1.5 - i) for i, p in enumerate(px)]
    dy = torch.zeros((c.N, ho, wo, c.ldy))
    for p, ch, g in hot:
        dy.view(-1, c.ldy)[p, ch] = g
    dw, _ = wc.reference(x, dy, c)
    closed = wc.onehot_dw(x, c, hot, dtype=torch.float64)
    assert torch.equal(closed, dw)
    assert float(closed[0].abs().max()) > 0
    if c.pad:                                                                        # pixel 0 under tap (0, 0) is padding
        assert float(closed[0, 0, 0].abs().max()) == 0.0
    assert float(closed[len(hot):].abs().max()) == 0.0


def test_seam_pixels():
    assert wc.seam_pixels(512, 667, 2001) == [0, 511, 512, 666, 667, 1023, 1024, 1536, 2000]
    assert wc.seam_pixels(288, 180, 540) == [0, 179, 180, 287, 288, 539]
    assert wc.seam_pixels(512, 16, 16) == [0, 15]
    assert wc.seam_pixels(32, 1, 1) == [0]


@pytest.mark.parametrize("c", wc.DENSE + wc.ONEHOT, ids=lambda c: c.name)
def test_cases_take_the_path_they_are_named_for(conv, c):
    """Every case's plan, in every product mode and both reductions, on the host: the GPU test asserts the same before it launches."""
    for det in (0, 1):
        for mode, plan in plans(conv, c, det).items():
            assert plan is not None and plan["arith"] == MODES.index(mode), (mode, plan)
            assert not wc.check_plan(c, plan, mode != "native"), (mode, plan, wc.check_plan(c, plan, mode != "native"))
            assert plan["grid"] == plan["tiles"] * ((plan["splits"] + 7) // 8 * 8 if plan["xcd_map"] else plan["splits"])
            assert (plan["splits"] - 1) * plan["per_split"] < wc.pixels(c) <= plan["splits"] * plan["per_split"]


@pytest.mark.parametrize("c", wc.ONEHOT, ids=lambda c: c.name)
def test_onehot_tables(conv, c):
    """Seam pixels of every mode's plan lie inside the problem, in distinct channels, and every hot element the GPU test divides by is
    nonzero unless its tap is padding."""
    for mode, plan in plans(conv, c).items():
        x, dy, hot = wc.onehot_inputs(c, plan["per_split"])
        assert all(0 <= p < wc.pixels(c) for p, _, _ in hot) and len({ch for _, ch, _ in hot}) == len(hot)
        assert plan["per_split"] - 1 in [p for p, _, _ in hot] and plan["per_split"] in [p for p, _, _ in hot]
        assert int((dy != 0).sum()) == len(hot)
        assert float(x.abs().min()) >= 2.0 ** -6 and float(x.abs().max()) < 4.0
        want = wc.onehot_dw(x, c, hot)
        rows = want[[ch for _, ch, _ in hot]]
        assert bool((rows != 0).reshape(len(hot), -1).any(dim=1).all())
        assert int((want != 0).sum()) == int((rows != 0).sum())


def test_plan_follows_the_launcher(conv):
    """The plan query against facts the launcher's source states: the kernel of the split modes on the 128 x 128 tile, the fp16 form only
    with both amax operands, the flags form only where the once kernel runs, refusals where the call refuses."""
    c = wc.BY_NAME["relu-128-128-3x3"]
    g = wc.geom(c)
    conv.set_fp32_mfma("split3")
    assert conv.wgrad_plan(c.ldy, 1, 0, 0, 0, 0, g, have_amax=True)["arith"] == 2
    assert conv.wgrad_plan(c.ldy, 1, 0, 0, 0, 0, g, have_amax=False)["arith"] == 1
    assert conv.wgrad_plan(c.ldy, 1, 0, 0, 0, 0, g, have_flags=True) is None                  # in_relu, and not a flat 1 x 1 problem's kernel
    flat = (1, 1, 700, 128, 1, 700, 128, 1, 1, 1, 0, 0)
    assert conv.wgrad_plan(128, 3, 0, 0, 0, 0, flat, have_flags=True)["kernel"] == 1
    conv.set_fp32_mfma("native")
    assert conv.wgrad_plan(128, 3, 0, 0, 0, 0, flat, have_flags=True) is None                 # native mode cannot skip
    assert conv.wgrad_plan(c.ldy, 1, 0, 0, 0, 0, g)["kernel"] == 0
    assert conv.wgrad_plan(c.ldy, 0, 0, 0, 0, 0, g) is None and conv.wgrad_plan(c.ldy - 4, 1, 0, 0, 0, 0, g) is None
    for b in wc.BATCHED.values():
        p = conv.wgrad_plan(b["cout"], b["nbatch"], 0, 0, 0, 0, (1, 1, b["T"], b["cin"], 1, b["T"], b["cout"], 1, 1, 1, 0, 0))
        assert p["shape"] == b["shape"] and p["tiles"] == b["nbatch"] and p["splits"] == 2 and p["per_split"] == 352


def test_references_are_usable():
    """Where the GPU test divides: every dense case's reference has a nonzero maximum, for dw and for the column sums (the three large
    cases are left to the GPU run, which computes them anyway and asserts the same)."""
    for c in wc.DENSE:
        if c in wc.LARGE:
            continue
        _, _, _, dw, cs = wc.get(c.name)
        assert float(dw.abs().max()) > 0 and float(cs.abs().max()) > 0 and bool(torch.isfinite(dw).all()), c.name
    for cin, b in wc.BATCHED.items():
        x, dy, dw, cs = wc.batched_inputs(cin)
        assert float(dw.abs().max()) > 0 and float(cs.abs().max()) > 0 and bool(torch.isfinite(dw).all())
        assert bool(torch.isnan(dy[:, b["T"]:]).all()) and bool(torch.isnan(x[:, b["T"]:]).all())


def test_guarded_allocator():
    t = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    buf, v = wc.guarded(t)
    assert v.is_contiguous() and torch.equal(v, t) and wc.guards_intact(buf) and buf.numel() == 24 + 2 * wc.GUARD
    assert v.data_ptr() == buf.data_ptr() + 4 * wc.GUARD
    buf[wc.GUARD - 1] = 0.0
    assert not wc.guards_intact(buf)

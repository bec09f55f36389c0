"""The fp32 weight gradient (csrc/conv_wgrad.hip) on every path wgrad_launch can choose -- tile shape x kernel x arithmetic x
workgroup-to-slice mapping x reduction -- against the float64 reference and the one-hot closed form of tests/wgrad_cases.py
(tests/test_wgrad_cases_host.py proves those on the CPU).

Every case first asks rn_conv_wgrad_plan which path the launcher takes and asserts that it is the one the case is named for; then it
launches through conv.wgrad / conv._wgrad_call (the C ABI).  Every call starts from a random nonzero dw and colsum (the kernels
accumulate), with the sentinel in the columns Kflat .. Kpad of dw, and with dy and x inside NaN guard bands; afterwards the difference
is held to the reference at 2e-5 of its max magnitude (test_gpu_conv.py::test_wgrad_long_k's bound), the sentinel columns must be
bit-unchanged and the guard bands intact.  The one-hot cases say which pixel went to which tap: one value of dy per seam pixel of the
plan (slice seams, image seams, both ends), exact in native mode, 2^-19 relative in the split modes, exact zeros everywhere else.

All of it runs in the four product modes of test_gpu_conv.py's fixture, with the fixed-order reduction off and on; on, two runs must also
agree bit for bit.  The three large shapes keep all four modes: the whole module takes well under a minute."""
import pytest
import torch

import wgrad_cases as wc

pytestmark = pytest.mark.gpu

RN_EINVAL = 10001


@pytest.fixture(scope="module", params=[(m, d) for m in ("native", "split", "split-in-kernel", "split3") for d in (0, 1)],
                ids=lambda p: "%s-%s" % (p[0], "fixed-order" if p[1] else "atomics"))
def cv(dev, request):
    """test_gpu_conv.py's product modes (for this kernel "split" and "split-in-kernel" are one path: both operands are activations and
    always split in the kernel), each with RN_OPT_DETERMINISTIC off and on."""
    from retinanet_mi355x import conv
    mode, det = request.param
    before = conv.get_fp32_mfma(), conv.PRESPLIT, conv.get_option(conv.OPT_DETERMINISTIC)
    conv.set_fp32_mfma(mode.split("-")[0])
    conv.PRESPLIT = mode in ("split", "split3")
    conv.set_option(conv.OPT_DETERMINISTIC, det)
    yield conv
    conv.set_fp32_mfma(before[0])
    conv.PRESPLIT = before[1]
    conv.set_option(conv.OPT_DETERMINISTIC, before[2])


def det_on(cv):
    return bool(cv.get_option(cv.OPT_DETERMINISTIC))


def the_plan(cv, c):
    """The plan of cv.wgrad's launch of case c, asserted to be the case's path."""
    mode = cv.get_fp32_mfma()
    plan = cv.wgrad_plan(c.ldy, 1, 0, 0, 0, 0, wc.geom(c), have_amax=mode == "split3")
    bad = wc.check_plan(c, plan, mode != "native")
    assert not bad, (c.name, mode, plan, bad)
    assert plan["arith"] == cv.FP32_MFMA_MODES.index(mode), plan
    return plan


def launch(cv, dev, c, xg, dyg, dw0, cs0):
    dw, cs = dw0.to(dev), cs0.to(dev)
    cv.wgrad(dyg, xg, dw, c.cout, c.k, c.stride, c.pad, kw_pad=c.kw, in_relu=c.relu, colsum=cs)
    torch.cuda.synchronize()
    return dw.cpu(), cs.cpu()


def rel_err(got, want):
    """max |got - want| / max |want| (a NaN anywhere gives NaN, which fails every <=)."""
    return float((got.double() - want).abs().max()) / float(want.abs().max())


def run_dense(cv, dev, name):
    c, x, dy, dw_ref, cs_ref = wc.get(name)
    assert float(dw_ref.abs().max()) > 0 and float(cs_ref.abs().max()) > 0
    plan = the_plan(cv, c)
    xbuf, xg = wc.guarded(x, dev)
    dbuf, dyg = wc.guarded(dy, dev)
    dw0, cs0 = wc.start_dw(c)
    dw, cs = launch(cv, dev, c, xg, dyg, dw0, cs0)
    kf = wc.kflat(c)
    e_dw = rel_err(dw[:, :kf].double() - dw0[:, :kf].double(), dw_ref)
    e_cs = rel_err(cs.double() - cs0.double(), cs_ref)
    print("%s %s %s: %s | dw %.3g colsum %.3g of max" % (name, cv.get_fp32_mfma(), "fixed-order" if det_on(cv) else "atomics", plan, e_dw, e_cs))
    assert e_dw <= wc.TOL, (name, e_dw)
    assert e_cs <= wc.TOL, (name, e_cs)
    assert torch.equal(dw[:, kf:], dw0[:, kf:]), "columns Kflat .. Kpad of dw were written"
    assert wc.guards_intact(xbuf.cpu()) and wc.guards_intact(dbuf.cpu())
    if det_on(cv):
        dw2, cs2 = launch(cv, dev, c, xg, dyg, dw0, cs0)
        assert torch.equal(dw, dw2) and torch.equal(cs, cs2), "the fixed-order form differs from run to run"
    return c, dw, dw0, plan


@pytest.mark.parametrize("name", [c.name for c in wc.LARGE])
def test_slices_kept_on_one_xcd(cv, dev, name):
    """xcd_map on (whole slices per XCD, the slice count rounded up to 8): 16 slices of 704 pixels = three pixel-table batches; 39 / 31
    slices, so that the last group of 8 has padding workgroups, in every mode; 896 pixels = four table batches (its own shape: the first
    one's slices stop at three)."""
    run_dense(cv, dev, name)


@pytest.mark.parametrize("name", [c.name for c in wc.RELU])
def test_in_relu_on_each_tile_shape(cv, dev, name):
    """max(x, 0) on load with x half negative: 64 x 256, 256 x 64 and 128 x 128 tiles, the last on the once kernel in the split modes (in
    split3 its fp16 form)."""
    c, _, _, plan = run_dense(cv, dev, name)
    if c.expect["once"] and cv.get_fp32_mfma() != "native":
        assert plan["kernel"] == 1


@pytest.mark.parametrize("name", [c.name for c in wc.SWITCH])
def test_tile_shape_switches(cv, dev, name):
    """Both sides of Cout <= 64 and of Kflat <= 64, one output channel, four input channels."""
    run_dense(cv, dev, name)


@pytest.mark.parametrize("name", [c.name for c in wc.PIXELS])
def test_pixel_counts(cv, dev, name):
    """Fewer pixels than a K-step, exactly one, one more; a slice of exactly per_split pixels and the 513 that make two; a 1 x 1 image under
    a 3 x 3 kernel, where eight of the nine taps meet padding only: their part of dw must not change by a bit."""
    c, dw, dw0, _ = run_dense(cv, dev, name)
    if name == "image-1x1-under-3x3":
        got, was = dw[:, :wc.kflat(c)].reshape(c.cout, 9, c.cin), dw0[:, :wc.kflat(c)].reshape(c.cout, 9, c.cin)
        off = [t for t in range(9) if t != 4]
        assert torch.equal(got[:, off], was[:, off])
        assert not torch.equal(got[:, 4], was[:, 4])


@pytest.mark.parametrize("name", [c.name for c in wc.STRIDE + wc.LDY])
def test_stride_padding_and_row_pitch(cv, dev, name):
    """Stride 2 on odd and even sizes, 1 x 1 stride 2, the stem's 7 x 7 stride 2 with kw = 8 on four channels; dy rows wider than Cout with
    random values in the columns past it."""
    run_dense(cv, dev, name)


@pytest.mark.parametrize("name", [c.name for c in wc.ONEHOT])
def test_one_value_per_seam_pixel(cv, dev, name):
    """dy is zero but for one value at each seam pixel of the plan, each in its own channel, dw starts at zero: row ch of dw is g * x under
    the nine taps of that pixel -- bit for bit in native mode (one product, one rounding; every other addend is an exact zero), within
    2^-19 in the split modes (22 significand bits per operand give a product to about 2^-21; two bits of margin) -- and every other element,
    padding taps included, is exactly 0.0.  A pixel dropped, taken twice or met under a shifted tap shows as a whole wrong row."""
    c = wc.BY_NAME[name]
    plan = the_plan(cv, c)
    x, dy, hot = wc.onehot_inputs(c, plan["per_split"])
    xbuf, xg = wc.guarded(x, dev)
    dbuf, dyg = wc.guarded(dy, dev)
    dw0, cs0 = wc.start_dw(c, zero=True)
    dw, cs = launch(cv, dev, c, xg, dyg, dw0, cs0)
    kf = wc.kflat(c)
    want = wc.onehot_dw(x, c, hot).reshape(c.cout, kf)
    got = dw[:, :kf]
    assert torch.equal(dw[:, kf:], dw0[:, kf:])
    assert torch.equal(got == 0, want == 0), "nonzero elements of dw are not those of the closed form: %d against %d" % (
        int((got != 0).sum()), int((want != 0).sum()))
    nz = want != 0
    rel = float(((got[nz].double() - want[nz].double()).abs() / want[nz].double().abs()).max())
    print("%s %s: seam pixels %s, worst relative error of a hot element %.3g" % (name, cv.get_fp32_mfma(), [p for p, _, _ in hot], rel))
    if cv.get_fp32_mfma() == "native":
        assert torch.equal(got, want)
    else:
        assert rel <= 2.0 ** -19, rel
    cs_want = torch.zeros(c.cout, dtype=torch.float64)
    for _, ch, g in hot:
        cs_want[ch] = g
    assert rel_err(cs.double() - cs0.double(), cs_want) <= wc.TOL
    assert wc.guards_intact(xbuf.cpu()) and wc.guards_intact(dbuf.cpu())


def batched_setup(cv, dev, cin):
    b = wc.BATCHED[cin]
    x, dy, dw_ref, cs_ref = wc.batched_inputs(cin)
    stride = b["cout"] * b["kpad"] + b["gap"]
    g = torch.Generator().manual_seed(77)
    dw0 = torch.full((b["nbatch"], stride), wc.SENTINEL)
    dw0[:, :b["cout"] * b["kpad"]] = torch.randn((b["nbatch"], b["cout"] * b["kpad"]), generator=g) + 3.0
    cs0 = torch.randn(b["cout"], generator=g) - 3.0
    geom = (1, 1, b["T"], b["cin"], 1, b["T"], b["cout"], 1, 1, 1, 0, 0)
    # split3: ONE plain word per operand, an fp32 bit pattern whose exponent bounds the tensor (count -1), as wino_wgrad_group passes
    amax = (None, None)
    if cv.get_fp32_mfma() == "split3":
        word = lambda t: t[:, :b["T"]].abs().max().reshape(1).view(torch.int32).to(dev)
        amax = (word(dy), word(x))
    return b, x, dy, dw_ref, cs_ref, stride, dw0, cs0, geom, amax


@pytest.mark.parametrize("cin", sorted(wc.BATCHED))
def test_batched_form(cv, dev, cin):
    """Three flat 1 x 1 problems in one launch (the Winograd weight gradient's form; from 64 channels on the 256 x 64 tile, from 128 on the
    128 x 128 tile and, in the split modes, the once kernel): results dw_bstride = Cout * Kpad + 64 apart with the
    gaps sentinel-filled, the column sums of entry 2 only, operands Tpad rows apart with NaN in the rows past T; in the fixed-order form
    the slabs are images of all three entries (slab_stride = nbatch * dw_bstride) with the column-sum rows behind them."""
    from retinanet_mi355x import _hip
    lib = _hip.load()
    b, x, dy, dw_ref, cs_ref, stride, dw0, cs0, geom, amax = batched_setup(cv, dev, cin)
    plan = cv.wgrad_plan(b["cout"], b["nbatch"], b["Tpad"] * b["cout"], b["Tpad"] * b["cin"], stride, b["colsum_batch"], geom,
                         have_amax=amax[0] is not None)
    assert plan["tiles"] == b["nbatch"] and plan["splits"] == 2 and plan["arith"] == cv.FP32_MFMA_MODES.index(cv.get_fp32_mfma()), plan
    assert plan["shape"] == b["shape"] and plan["kernel"] == int(b["shape"] == 2 and cv.get_fp32_mfma() != "native"), plan
    xbuf, xg = wc.guarded(x, dev)
    dbuf, dyg = wc.guarded(dy, dev)

    def call():
        dw, cs = dw0.to(dev), cs0.to(dev)
        rc = cv._wgrad_call(lib, dev, dyg.data_ptr(), b["cout"], xg.data_ptr(), dw.data_ptr(), cs.data_ptr(), b["nbatch"],
                            b["Tpad"] * b["cout"], b["Tpad"] * b["cin"], stride, b["colsum_batch"], geom, amax=amax)
        assert rc == 0
        torch.cuda.synchronize()
        return dw.cpu(), cs.cpu()
    dw, cs = call()
    n = b["cout"] * b["kpad"]
    got = (dw[:, :n].double() - dw0[:, :n].double()).view(b["nbatch"], b["cout"], b["kpad"])
    e_dw, e_cs = rel_err(got, dw_ref), rel_err(cs.double() - cs0.double(), cs_ref)
    print("batched-%d %s: %s | dw %.3g colsum %.3g of max" % (cin, cv.get_fp32_mfma(), plan, e_dw, e_cs))
    assert e_dw <= wc.TOL and e_cs <= wc.TOL, (e_dw, e_cs)
    assert torch.equal(dw[:, n:], dw0[:, n:]), "the gaps between batch entries were written"
    assert wc.guards_intact(xbuf.cpu()) and wc.guards_intact(dbuf.cpu())
    if not det_on(cv):
        return
    dw2, cs2 = call()
    assert torch.equal(dw, dw2) and torch.equal(cs, cs2)
    # the workspace contract: one byte short is refused and nothing is touched
    nb = lib.rn_conv_wgrad_det_workspace_bytes(b["cout"], b["nbatch"], stride, *geom[:9])
    assert nb == plan["splits"] * (b["nbatch"] * stride + b["cout"]) * 4
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    dwg, csg = dw0.to(dev), cs0.to(dev)
    cnt = lambda a: 0 if a is None else -1
    args = (dyg.data_ptr(), b["cout"], xg.data_ptr(), dwg.data_ptr(), csg.data_ptr(), b["nbatch"], b["Tpad"] * b["cout"],
            b["Tpad"] * b["cin"], stride, b["colsum_batch"]) + geom + (_hip.ptr(amax[0]), cnt(amax[0]), _hip.ptr(amax[1]), cnt(amax[1]))
    assert lib.rn_conv_wgrad_batched_det(*args, ws.data_ptr(), nb - 1, _hip.stream()) == RN_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(dwg.cpu(), dw0) and torch.equal(csg.cpu(), cs0)


def test_refusals(cv, dev):
    """Arguments the launcher's checks turn away: RN_EINVAL, no launch, dw bit-unchanged."""
    from retinanet_mi355x import _hip
    lib = _hip.load()
    cin, cout, T = 64, 128, 64
    dw0 = torch.randn((cout, 64), generator=torch.Generator().manual_seed(5))
    dw = dw0.to(dev)
    x, dy = torch.ones((T, cin), device=dev), torch.ones((T, cout), device=dev)
    flags = torch.ones(T, dtype=torch.uint8, device=dev)
    none = (None, 0, None, 0)

    def batched(ldy=cout, nbatch=1, cs_batch=0, cin_=cin):
        return lib.rn_conv_wgrad_batched(dy.data_ptr(), ldy, x.data_ptr(), dw.data_ptr(), None, nbatch, 0, 0, 0, cs_batch,
                                         1, 1, T, cin_, 1, T, cout, 1, 1, 1, 0, 0, *none, _hip.stream())

    def flagged(kh=1, in_relu=0):
        return lib.rn_conv_wgrad_batched_flags(dy.data_ptr(), cout, x.data_ptr(), dw.data_ptr(), None, 1, 0, 0, 0, 0,
                                               1, 1, T, cin, 1, T, cout, kh, kh, 1, 0, in_relu, *none, flags.data_ptr(), None, 0, _hip.stream())
    assert batched(cin_=6) == RN_EINVAL
    assert batched(ldy=cout - 4) == RN_EINVAL
    assert batched(ldy=cout + 1) == RN_EINVAL
    assert batched(nbatch=0) == RN_EINVAL
    assert batched(nbatch=2, cs_batch=2) == RN_EINVAL
    assert lib.rn_conv_wgrad_batched_det(dy.data_ptr(), cout, x.data_ptr(), dw.data_ptr(), None, 1, 0, 0, 0, 0,
                                         1, 1, T, cin, 1, T, cout, 1, 1, 1, 0, 0, *none, None, 1 << 20, _hip.stream()) == RN_EINVAL
    assert flagged(in_relu=1) == RN_EINVAL
    assert flagged(kh=3) == RN_EINVAL
    for a in ((cout, 0), (cout - 4, 1), (cout + 1, 1)):
        assert cv.wgrad_plan(a[0], a[1], 0, 0, 0, 0, (1, 1, T, cin, 1, T, cout, 1, 1, 1, 0, 0)) is None
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), dw0)

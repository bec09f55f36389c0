"""The fused backward of a 1x1 stride-1 layer 64 -> 256 (csrc/conv_bwd_1x1.hip: rn_conv_bwd_1x1, conv.bwd_1x1_fused): data gradient,
weight gradient and column sums from ONE pass over dy, against a float64 reference built here.

Shapes [N, H, W]: [1,4,4] one K-step exactly; [1,5,7] 35 pixels, a ragged last K-step; [3,3,11] 33 pixels per image, so that slices end at
image boundaries that are no K-step multiples; [2,24,40] more than one slice per image.  Each with mask none / fp32 activations (mode 1) /
sign bits (mode 2).  Image i of dy is scaled by 2^(12 i) and of x by 2^(-12 i): the per-image scales differ by 2^12 from image to image
while every image contributes alike to dw.

Bounds (the project's own): dx within 1e-4 of its largest magnitude (tests/test_gpu_conv.py) -- asserted per image, which is no weaker --
dw and colsum within 2e-5 of theirs (tests/test_gpu_wgrad_paths.py).  The errors of the pair of launches the kernel replaces are printed
beside the kernel's, on the same inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RN_EINVAL = 10001
CIN, COUT = 64, 256
DX_TOL, DW_TOL = 1e-4, 2e-5
SHAPES = [(1, 4, 4), (1, 5, 7), (3, 3, 11), (2, 24, 40)]


@pytest.fixture(scope="module")
def cv(dev):
    from retinanet_mi355x import conv
    before = conv.get_fp32_mfma(), conv.PRESPLIT, conv.get_option(conv.OPT_DETERMINISTIC)
    conv.set_fp32_mfma("split3")
    conv.PRESPLIT = True
    conv.set_option(conv.OPT_DETERMINISTIC, 0)
    yield conv
    conv.set_fp32_mfma(before[0])
    conv.PRESPLIT = before[1]
    conv.set_option(conv.OPT_DETERMINISTIC, before[2])


def sign_words(t):
    """The sign bits of t as its producer would leave them: bit (e & 31) of word (e >> 5) = element e > 0."""
    b = (t.flatten() > 0).view(-1, 32).to(torch.int64)
    w = (b << torch.arange(32, device=t.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


_CASES = {}


def case(shape):
    """Inputs (CPU) and the float64 reference of a shape, computed once: dy, x, weight [256,64,1,1], activations for the mask,
    dx_ref (unmasked), dw_ref, cs_ref."""
    if shape not in _CASES:
        N, H, W = shape
        g = torch.Generator().manual_seed(1000 + 100 * N + 10 * H + W)
        dy = torch.randn(N, H, W, COUT, generator=g)
        x = torch.randn(N, H, W, CIN, generator=g)
        for i in range(N):
            dy[i] *= 2.0 ** (12 * i)
            x[i] *= 2.0 ** (-12 * i)
        weight = torch.randn(COUT, CIN, 1, 1, generator=g) * 0.1
        act = torch.randn(N, H, W, CIN, generator=g).clamp(min=0)          # a ReLU output: about half of it zero
        dyd, xd = dy.double().reshape(-1, COUT), x.double().reshape(-1, CIN)
        dx_ref = (dyd @ weight.double().reshape(COUT, CIN)).reshape(N, H, W, CIN)
        _CASES[shape] = (dy, x, weight, act, dx_ref, dyd.t() @ xd, dyd.sum(0))
    return _CASES[shape]


def rel_err(got, want):
    """max |got - want| / max |want| (a NaN anywhere gives NaN, which fails every <=)."""
    return float((got.double() - want).abs().max()) / float(want.abs().max())


def run_fused(cv, dev, dy, x, wd, act, mask_mode, dw0, cs0, sign=False):
    dw, cs = dw0.to(dev), cs0.to(dev)
    mask = None
    if mask_mode:
        mask = act.to(dev)
        if mask_mode == 2:
            mask._rn_sign = sign_words(mask)
    dx = cv.bwd_1x1_fused(dy.to(dev), x.to(dev), wd, dw, cs, mask=mask, mask_mode=mask_mode or None, sign=sign)
    torch.cuda.synchronize()
    return dx, dw.cpu(), cs.cpu()


@pytest.mark.parametrize("mask_mode", [0, 1, 2], ids=["nomask", "mask-fp32", "mask-bits"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64(cv, dev, shape, mask_mode):
    N, H, W = shape
    dy, x, weight, act, dx_ref, dw_ref, cs_ref = case(shape)
    wd = cv.pack_weights(weight.to(dev), 1)                                 # [64][256] with its fp16 twin
    assert tuple(wd.shape) == (CIN, COUT) and getattr(wd, "_rn_split16", None) is not None
    want_dx = dx_ref * (act > 0) if mask_mode else dx_ref
    g = torch.Generator().manual_seed(7)
    dw0 = torch.randn(COUT, CIN, generator=g) * (1e-3 * float(dw_ref.abs().max()))     # the kernel accumulates: a nonzero start
    cs0 = torch.randn(COUT, generator=g) * (1e-3 * float(cs_ref.abs().max()))
    dx, dw, cs = run_fused(cv, dev, dy, x, wd, act, mask_mode, dw0, cs0)
    dxc = dx.cpu()
    # the pair on the same inputs
    dw_p, cs_p = dw0.to(dev), cs0.to(dev)
    mask_p = None
    if mask_mode:
        mask_p = act.to(dev)
        if mask_mode == 2:
            mask_p._rn_sign = sign_words(mask_p)
    dyg, xg = dy.to(dev), x.to(dev)
    cv.wgrad(dyg, xg, dw_p, COUT, 1, 1, 0, colsum=cs_p)
    dx_p = cv.dgrad(dyg, wd, (H, W), CIN, 1, 1, 0, mask=mask_p, mask_mode=2)
    torch.cuda.synchronize()
    e_dx = [rel_err(dxc[i], want_dx[i]) for i in range(N)]
    e_dxp = [rel_err(dx_p[i].cpu(), want_dx[i]) for i in range(N)]
    e_dw, e_cs = rel_err(dw.double() - dw0.double(), dw_ref), rel_err(cs.double() - cs0.double(), cs_ref)
    e_dwp, e_csp = rel_err(dw_p.cpu().double() - dw0.double(), dw_ref), rel_err(cs_p.cpu().double() - cs0.double(), cs_ref)
    print("%s mask %d: fused dx %s dw %.3g colsum %.3g | pair dx %s dw %.3g colsum %.3g (of max)" % (
        shape, mask_mode, ["%.3g" % e for e in e_dx], e_dw, e_cs, ["%.3g" % e for e in e_dxp], e_dwp, e_csp))
    assert rel_err(dxc, want_dx) <= DX_TOL
    for i in range(N):
        assert e_dx[i] <= DX_TOL, (shape, i, e_dx)
    assert e_dw <= DW_TOL, (shape, e_dw)
    assert e_cs <= DW_TOL, (shape, e_cs)
    if mask_mode:
        assert bool((dxc[act <= 0] == 0).all()), "masked-out elements of dx are not exactly zero"
    # amax bytes of dx: the highest set byte of image i's table is the exponent field of its largest magnitude
    words, _ = dx._rn_amax
    tables = words.cpu().view(torch.uint8).reshape(N, 256)
    for i in range(N):
        e_max = (int(dxc[i].abs().max().view(torch.int32)) >> 23) & 0xff
        set_bytes = tables[i].nonzero().flatten()
        assert len(set_bytes) and int(set_bytes.max()) == e_max, (shape, i, e_max, set_bytes.tolist())
    # every image alone: the same bits
    if N > 1:
        for i in range(N):
            dx1, _, _ = run_fused(cv, dev, dy[i:i + 1].contiguous(), x[i:i + 1].contiguous(), wd, act[i:i + 1].contiguous(), mask_mode,
                                  torch.zeros_like(dw0), torch.zeros_like(cs0))
            assert torch.equal(dx1[0].cpu(), dxc[i]), "dx of image %d depends on its neighbours in the batch" % i


def test_sign_bits_of_dx(cv, dev):
    """sign=True: the bits of dx as a consumer reads them (element e > 0), with and without a mask."""
    shape = (3, 3, 11)
    dy, x, weight, act, _, dw_ref, cs_ref = case(shape)
    wd = cv.pack_weights(weight.to(dev), 1)
    for mask_mode in (0, 2):
        dx, _, _ = run_fused(cv, dev, dy, x, wd, act, mask_mode, torch.zeros(COUT, CIN), torch.zeros(COUT), sign=True)
        assert torch.equal(dx._rn_sign.cpu(), sign_words(dx).cpu())


def test_one_hot(cv, dev):
    """One pixel and one channel of dy and of x: the product lands in exactly one element of dw (2^-19 relative, as
    tests/test_gpu_wgrad_paths.py holds the split modes to), the column sum in one element, and dx in that pixel's 64 channels."""
    N, H, W = 3, 3, 11
    _, _, weight, _, _, _, _ = case((N, H, W))
    wd = cv.pack_weights(weight.to(dev), 1)
    for (n0, p0, c0, ci0, a, b) in [(1, 17, 201, 37, 1.7182817, -0.5772157), (2, 32, 0, 63, -3.1415927, 2.5e-3), (0, 0, 255, 0, 0.3, 7.0)]:
        dy, x = torch.zeros(N, H, W, COUT), torch.zeros(N, H, W, CIN)
        dy.view(N, H * W, COUT)[n0, p0, c0] = a
        x.view(N, H * W, CIN)[n0, p0, ci0] = b
        dx, dw, cs = run_fused(cv, dev, dy, x, wd, None, 0, torch.zeros(COUT, CIN), torch.zeros(COUT))
        want = float(torch.tensor(a).double() * torch.tensor(b).double())
        assert abs(float(dw[c0, ci0]) - want) <= 2.0 ** -19 * abs(want), (float(dw[c0, ci0]), want)
        dw[c0, ci0] = 0
        assert int(dw.count_nonzero()) == 0, "the one-hot product reached other elements of dw"
        assert float(cs[c0]) == float(torch.tensor(a)) and int(cs.count_nonzero()) == 1
        dxc = dx.cpu().view(N, H * W, CIN)
        want_dx = torch.tensor(a).double() * weight.double().reshape(COUT, CIN)[c0]
        assert rel_err(dxc[n0, p0], want_dx) <= DX_TOL
        assert int(dxc[n0, p0].count_nonzero()) == CIN
        dxc[n0, p0] = 0
        assert int(dxc.count_nonzero()) == 0, "the one-hot gradient reached other pixels of dx"


def test_refuses_what_is_not_built(cv, dev):
    from retinanet_mi355x import _hip
    lib = _hip.load()
    N, H, W = 1, 4, 4
    dy, x, weight, _, _, _, _ = case((N, H, W))
    wd = cv.pack_weights(weight.to(dev), 1)
    tw = wd._rn_split16
    dyg, xg = dy.to(dev), x.to(dev)
    dx = torch.empty(N, H, W, CIN, device=dev)
    dw, cs = torch.zeros(COUT, CIN, device=dev), torch.zeros(COUT, device=dev)
    dy_am, x_am = cv.amax_words(dyg), cv.amax_words(xg)

    def call(cin=CIN, cout=COUT, stride=1, add=None, mask=None, mask_mode=0, dy_amax=dy_am):
        return lib.rn_conv_bwd_1x1(dyg.data_ptr(), xg.data_ptr(), tw[0].data_ptr(), tw[1].data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                   cs.data_ptr(), _hip.ptr(mask), mask_mode, _hip.ptr(add), None, _hip.ptr(dy_amax), x_am.data_ptr(), None,
                                   N, H, W, cin, cout, stride, _hip.stream())

    assert call() == 0
    assert call(cin=32) == RN_EINVAL
    assert call(cin=128) == RN_EINVAL
    assert call(cout=128) == RN_EINVAL
    assert call(cout=512) == RN_EINVAL
    assert call(stride=2) == RN_EINVAL
    assert call(add=dx) == RN_EINVAL
    assert call(mask_mode=1) == RN_EINVAL                                  # a mask mode without a mask
    assert call(mask=xg, mask_mode=3) == RN_EINVAL
    assert call(dy_amax=None) == RN_EINVAL
    before = cv.get_fp32_mfma()
    try:
        for mode in ("native", "split"):
            cv.set_fp32_mfma(mode)
            assert call() == RN_EINVAL
        cv.set_fp32_mfma("split3")
        cv.set_option(cv.OPT_DETERMINISTIC, 1)
        assert call() == RN_EINVAL
    finally:
        cv.set_option(cv.OPT_DETERMINISTIC, 0)
        cv.set_fp32_mfma(before)
    torch.cuda.synchronize()


def test_engine_takes_the_path_for_layer1(cv, dev, monkeypatch):
    """ResNet-50 at 64 x 96, batch 2: one backward with the pair of launches (RN_BWD_FUSED_1X1=0) and one with the default.  The fused path
    runs for exactly the four 64 -> 256 layers of layer1; every parameter gradient agrees within the weight gradient's bound."""
    from retinanet_mi355x import modules, synth
    net = modules.resnet50(num_classes=8)
    net.load_state_dict(synth.state_dict("resnet50", 8, 12, seed=2))
    net = net.to(dev)
    net.train()
    net.freeze_bn()
    h, w = 64, 96
    img = synth.frames(2, h, w, seed=11).to(dev)
    ann = synth.labels_dir(2, 4, h, w, 8, seed=12, size_px=(12, 40)).to(dev)

    def step():
        for p in net.parameters():
            p.grad = None
        sum(l.mean() for l in net([img, ann])).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}

    monkeypatch.setattr(cv, "BWD_FUSED_1X1", False)
    n0 = cv.BWD_FUSED_LAUNCHES
    g_pair = step()
    assert cv.BWD_FUSED_LAUNCHES == n0
    monkeypatch.setattr(cv, "BWD_FUSED_1X1", True)
    g_fused = step()
    assert cv.BWD_FUSED_LAUNCHES == n0 + 4, "the fused path ran for %d layers" % (cv.BWD_FUSED_LAUNCHES - n0)
    assert set(g_pair) == set(g_fused) and len(g_pair) > 50
    worst = ("", 0.0)
    for n, want in g_pair.items():
        m = float(want.abs().max())
        err = float((g_fused[n].double() - want.double()).abs().max()) / m if m > 0 else float(g_fused[n].abs().max())
        worst = max(worst, (n, err), key=lambda t: t[1])
        assert err <= DW_TOL, (n, err)
    print("fused against pair, ResNet-50 %dx%d batch 2: worst parameter gradient %s %.3g of its max" % (h, w, worst[0], worst[1]))

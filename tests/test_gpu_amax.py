"""split3 amax tables end to end (csrc/mfma_split.h "AMAX TABLES"; DESIGN.md 3 "Amax tables", 4.6b).

In RN_FP32_SPLIT3 every activation / gradient operand of a convolution is scaled by a power of two taken from ITS IMAGE's table, then
split into two fp16 terms.  Each kind of table error is silent in another way: under-reporting by two binades overflows fp16 (inf /
NaN), over-reporting loses precision below 2^-18 of the stale maximum, another image's table breaks "an image's result depends on that
image alone".  The other conv tests feed N(0,1) data alike in every image and measure error against the whole output's maximum: they
see none of these.  Here the batches are adversarial -- images scaled by 1, 2^-60, 2^40 and 0, each with one NEGATIVE outlier 2^8 above
the rest, at the first pixel of images that start mid-tile and at the last pixel of the last image, the largest outputs in the last real
column of a Cout that is not a multiple of the tile width, images down to 1 x 1 -- and

  A. every producer's tables are decoded and checked against the stored values (highest set byte == the largest exponent field of the
     image, nothing above it; bounds where the table is only a bound: max-pool, ReLU mask, the Winograd row / tensor words);
  B. every image of fprop / dgrad is compared with fp64 at ITS OWN maximum (the tolerances of test_gpu_conv.py / test_gpu_conv_mf16.py),
     and with split-K off is bit-identical to the same image run alone -- in split3 and, as controls of the tests themselves, in the
     native and split modes, which have no tables;
  C. a destination reused through a path that leaves no tables, and a torch in-place edit, leave no stale table behind;
  D. graphs captured one after the other on one stream, or on a stream that ran eagerly, replay bit-identically to eager runs while
     the magnitudes shrink and grow from replay to replay (module level, and a captured training step + eval forward);
  E. the split3 corners (inf, 3.4e38, tiny, subnormal-only and all-zero images) are pinned.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTORS = (1.0, 2.0 ** -60, 2.0 ** 40, 0.0)        # per image, cycled: tables of neighbours 2^40 .. 2^100 apart, an all-zero image
OUTLIER = -1024.0                                   # 2^8 above N(0,1) data, negative: a missing fabs shows
TOL_TILE, TOL_MF16 = 1e-4, 1e-5                    # test_gpu_conv.py / test_gpu_conv_mf16.py


def rnd(shape, seed, std=1.0):
    from retinanet_mi355x import synth
    return torch.from_numpy(synth.normal(shape, seed, std))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _modes(conv, mode, opts):
    before = (conv.get_fp32_mfma(), conv.PRESPLIT, {k: conv.get_option(k) for k in opts})
    conv.set_fp32_mfma(mode)
    conv.PRESPLIT = True
    for k, v in opts.items():
        conv.set_option(k, v)
    return before


def _restore(conv, before):
    conv.set_fp32_mfma(before[0])
    conv.PRESPLIT = before[1]
    for k, v in before[2].items():
        conv.set_option(k, v)


@pytest.fixture
def s3(dev):
    """split3 (the tables exist in this mode only)."""
    from retinanet_mi355x import conv
    before = _modes(conv, "split3", {})
    yield conv
    _restore(conv, before)


@pytest.fixture(params=["split3", "native", "split"])
def cv(dev, request):
    """The accuracy / identity tests run in split3 and, as controls (no tables there), in native and split."""
    from retinanet_mi355x import conv
    before = _modes(conv, request.param, {})
    yield conv                                       # (the mode: conv.get_fp32_mfma())
    _restore(conv, before)


def factors(n):
    return torch.tensor([FACTORS[i % len(FACTORS)] for i in range(n)], dtype=torch.float32)


def adversarial(shape, seed, outlier=True):
    """NCHW N(0,1) images scaled by FACTORS, each with one negative outlier: at pixel 0 (images after the first start mid-tile when
    H*W is not a multiple of the tile rows) and, for the last image, at its last pixel."""
    x = rnd(shape, seed)
    N, C, H, W = shape
    if outlier:
        for n in range(N):
            h, w = (H - 1, W - 1) if n == N - 1 else (0, 0)
            x[n, (3 * n + 1) % C, h, w] = OUTLIER
    return x * factors(N).view(N, 1, 1, 1)


def weights(cout, cin, k, seed):
    """He-scaled weights whose last output AND input channel are 16x larger: the largest outputs of fprop and dgrad fall in the last
    real column."""
    w = rnd((cout, cin, k, k), seed, (2.0 / (k * k * cin)) ** 0.5)
    w[-1] *= 16.0
    w[:, -1] *= 16.0
    return w


# ---------------------------------------------------------------------------------------------------------------- table decoding
def tables(words, n):
    """amax words [n * 64] int32 -> uint8 [n, 256] on the host."""
    assert words.numel() == n * 64, (words.numel(), n)
    return words.contiguous().view(torch.uint8).view(n, 256).cpu()


def top_byte(row):
    nz = torch.nonzero(row).flatten()
    return int(nz.max()) if nz.numel() else -1


def max_exp(t):
    """Largest fp32 exponent field of |t| (host)."""
    t = t.detach().float().cpu().abs().contiguous()
    return int(((t.view(torch.int32) >> 23) & 0xff).max()) if t.numel() else 0


def words_of(t):
    a = getattr(t, "_rn_amax", None)
    assert a is not None, "producer left no amax words"
    assert a[1] == t._version
    return a[0]


def check_tables(t, words=None, exact=True, what=""):
    """Image n's highest set byte == the largest exponent field of what is stored in image n (exact), or >= it (a bound).  An image
    whose largest exponent is 0 (all zero / subnormal) may set byte 0, nothing above it."""
    words = words_of(t) if words is None else words
    N = t.shape[0]
    tab = tables(words, N)
    tc = t.detach().cpu().reshape(N, -1)
    for n in range(N):
        e, top = max_exp(tc[n]), top_byte(tab[n])
        if exact:
            ok = top == e or (e == 0 and top <= 0)
        else:
            ok = top >= e
        assert ok, "%s image %d: highest table byte %d, largest exponent field stored %d" % (what, n, top, e)


def close_per_image(got, want, tol, what=""):
    """Error of image n against ITS OWN maximum (an all-zero image: exactly zero)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    for n in range(got.shape[0]):
        err = float((got[n] - want[n]).abs().max())
        ref = float(want[n].abs().max())
        assert err <= tol * ref, "%s image %d: max err %.3e vs max |ref| %.3e" % (what, n, err, ref)


def close(got, want, tol):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = float((got - want).abs().max())
    assert err <= tol * (float(want.abs().max()) + 1e-300), "max err %.3e vs max |ref| %.3e" % (err, float(want.abs().max()))


KERNELS = {"mf16": lambda cv: {cv.OPT_MF16: 1, cv.OPT_MF16_MIN: 1, cv.OPT_SPLITK: 0},      # the 16x16x32 kernel where it applies
           "tile": lambda cv: {cv.OPT_MF16: 0, cv.OPT_SPLITK: 0}}                        # conv_igemm_tile.h 2x2 / 4x1


def reaches_mf16(cin, cout, k, div_shift=0):
    """Whether a launch of this geometry runs on conv_igemm_mf16.hip in the split modes (pre-split weights) when OPT_MF16 = 1 and
    OPT_MF16_MIN = 1 (every tile count): the library's mf16_ok / mf16_geom_ok (Cin % 32 == 0, no stride-2 data-gradient divisibility test, kh * kw <= 24, Cout % 4 == 0, Cout > 64) and a
    reduction the split kernels take (kh * kw * Cin >= 64).  Otherwise the conv_igemm_tile.h tiles run it, whatever the option."""
    return cin % 32 == 0 and div_shift == 0 and k * k <= 24 and cout % 4 == 0 and cout > 64 and k * k * cin >= 64


CONV_CASES = [  # cin, cout, k, stride, pad, N, H, W
    (64, 192, 3, 1, 1, 4, 9, 11),        # Ho*Wo = 99: images 1..3 start mid-tile; Cout 192: a column tile with 64 real columns
    (128, 96, 1, 1, 0, 4, 7, 9),         # 1x1; fprop and dgrad both on the 16x16x32 kernel
    (64, 40, 3, 1, 1, 4, 5, 7),          # Cout <= 64 (the 4x1 tile), not a multiple of 32: never the 16x16x32 kernel
    (64, 128, 3, 2, 1, 4, 9, 11),        # stride 2 (generic dgrad: every tap tried, on the tiles)
    (64, 128, 3, 1, 1, 8, 1, 1),         # 1 x 1 images: one wave spans several of them
]


def _kernel_params():
    """(kernel, case) pairs: "tile" for every case, "mf16" only where fprop or dgrad does reach the 16x16x32 kernel -- so the two
    parametrisations never test the same kernels under two names."""
    out = []
    for c in CONV_CASES:
        cin, cout, k, stride = c[:4]
        out.append(("tile", c))
        if reaches_mf16(cin, cout, k) or reaches_mf16(cout, cin, k, stride.bit_length() - 1):
            out.append(("mf16", c))
    return out


def test_mf16_parametrisation_matches_the_dispatch_rule():
    """Which cases reach conv_igemm_mf16.hip, spelled out: fprop of cases 0, 1, 3, 4 and dgrad of case 1; case 2 never."""
    want = {0: (True, False), 1: (True, True), 2: (False, False), 3: (True, False), 4: (True, False)}
    for i, (cin, cout, k, stride, *_r) in enumerate(CONV_CASES):
        assert (reaches_mf16(cin, cout, k), reaches_mf16(cout, cin, k, stride.bit_length() - 1)) == want[i], i
    assert [c for kn, c in _kernel_params() if kn == "mf16"] == [CONV_CASES[i] for i in (0, 1, 3, 4)]


@pytest.mark.parametrize("kernel,case", _kernel_params())
def test_fprop_dgrad_tables_per_image_accuracy_and_independence(cv, dev, case, kernel):
    cin, cout, k, stride, pad, N, H, W = case
    mode = cv.get_fp32_mfma()
    before = _modes(cv, mode, KERNELS[kernel](cv))
    try:
        x = adversarial((N, cin, H, W), 1)
        w = weights(cout, cin, k, 2)
        y_ref = F.conv2d(x.double(), w.double(), None, stride, pad)
        gy = adversarial(tuple(y_ref.shape), 3)
        dx_ref = torch.nn.grad.conv2d_input((N, cin, H, W), w.double(), gy.double(), stride, pad)
        tol = TOL_MF16 if (kernel == "mf16" and mode != "native") else TOL_TILE
        xg, wg = nhwc(x).to(dev), w.to(dev)
        wp, wd = cv.pack_weights(wg, 0), cv.pack_weights(wg, 1)
        gyg = nhwc(gy).to(dev)
        y = cv.fprop(xg, wp, cout, k, stride, pad)
        dx = cv.dgrad(gyg, wd, (H, W), cin, k, stride, pad)
        close_per_image(nchw(y), y_ref, tol, "fprop")
        close_per_image(nchw(dx), dx_ref, tol, "dgrad")
        if mode == "split3":
            check_tables(y, what="fprop")
            check_tables(dx, what="dgrad")
        for n in range(N):                           # split-K off: each image alone gives the same bits
            assert torch.equal(cv.fprop(xg[n:n + 1].contiguous(), wp, cout, k, stride, pad), y[n:n + 1]), "fprop image %d" % n
            assert torch.equal(cv.dgrad(gyg[n:n + 1].contiguous(), wd, (H, W), cin, k, stride, pad), dx[n:n + 1]), "dgrad image %d" % n
        if kernel == "tile":                         # wgrad: ONE scale for the batch by design -- the whole-tensor tolerance
            wr = w.double().requires_grad_(True)
            (F.conv2d(x.double(), wr, None, stride, pad) * gy.double()).sum().backward()
            dw = torch.zeros_like(wp)
            cv.wgrad(gyg, xg, dw, cout, k, stride, pad)
            close(cv.unpack_wgrad(dw, wp, tuple(w.shape))[0], wr.grad, TOL_TILE)
    finally:
        _restore(cv, before)


SPLITK_CASES = [  # cin, cout, k, stride, pad, N, H, W : test_gpu_conv.py's split-K classes with adversarial images
    (512, 256, 3, 2, 1, 4, 9, 7),
    (256, 256, 3, 1, 1, 3, 4, 4),
    (512, 40, 3, 1, 1, 4, 5, 7),
]


@pytest.mark.parametrize("case", SPLITK_CASES)
def test_splitk_tables_and_per_image_accuracy(cv, dev, case):
    from retinanet_mi355x import _hip
    cin, cout, k, stride, pad, N, H, W = case
    x = adversarial((N, cin, H, W), 4)
    w = weights(cout, cin, k, 5)
    y_ref = F.conv2d(x.double(), w.double(), None, stride, pad)
    xg = nhwc(x).to(dev)
    Ho, Wo = y_ref.shape[2], y_ref.shape[3]
    d = cv._make_desc(xg, (Ho, Wo, cout, k, k, stride, 1, -pad, 0), 0, 0, (0, 0), 0, False, None, None, None, None)
    assert _hip.load().rn_conv_splitk_workspace_bytes(ctypes.byref(d)) > 0, "case no longer takes the split-K path"
    y = cv.fprop(xg, cv.pack_weights(w.to(dev), 0), cout, k, stride, pad)
    close_per_image(nchw(y), y_ref, TOL_TILE, "split-K fprop")
    if cv.get_fp32_mfma() == "split3":
        check_tables(y, what="split-K")


def test_grouped_and_stride2_classes(cv, dev):
    """conv_igemm_grouped (pyramid levels in one launch) and dgrad_s2_classes (four launches fill ONE table)."""
    cin, cout, N = 64, 96, 4
    w = weights(cout, cin, 3, 6)
    wg = w.to(dev)
    wp = cv.pack_weights(wg, 0)
    xs = [adversarial((N, cin, h, ww), 10 + i) for i, (h, ww) in enumerate([(9, 11), (5, 6), (1, 1)])]
    probs = []
    for x in xs:
        h, ww = x.shape[2], x.shape[3]
        probs.append(dict(x=nhwc(x).to(dev), y=torch.empty((N, h, ww, cout), device=dev), geom=(h, ww, cout, 3, 3, 1, 1, -1, 0)))
    cv.conv_igemm_grouped(probs, wp)
    for x, pr in zip(xs, probs):
        close_per_image(nchw(pr["y"]), F.conv2d(x.double(), w.double(), None, 1, 1), TOL_TILE, "grouped")
        if cv.get_fp32_mfma() == "split3":
            check_tables(pr["y"], what="grouped")
    # stride-2 data gradient by parity classes
    H, W = 9, 11
    gy = adversarial((N, cout, 5, 6), 13)
    wcls = [cv.pack_weights(wg, 1, taps=c[2]) for c in cv.s2_classes(3, 1)]
    dx = cv.dgrad_s2_classes(nhwc(gy).to(dev), wcls, (H, W), cin, 3, 1)
    want = torch.nn.grad.conv2d_input((N, cin, H, W), w.double(), gy.double(), 2, 1)
    close_per_image(nchw(dx), want, TOL_TILE, "dgrad_s2_classes")
    if cv.get_fp32_mfma() == "split3":
        check_tables(dx, what="dgrad_s2_classes")


def test_winograd_group_tables_accuracy_and_independence(cv, dev):
    cin = cout = 64
    N = 4
    w = weights(cout, cin, 3, 20)
    b = rnd((cout,), 21, 0.1)
    shapes = [(9, 11), (3, 5), (1, 1)]
    xs = [adversarial((N, cin, h, ww), 30 + i) for i, (h, ww) in enumerate(shapes)]
    U = cv.wino_weights(w.to(dev), 0)
    xg = [nhwc(x).to(dev) for x in xs]
    ys = cv.wino_conv_group(xg, U)
    for x, y in zip(xs, ys):
        close_per_image(nchw(y), F.conv2d(x.double(), w.double(), None, 1, 1), TOL_TILE, "winograd")
        if cv.get_fp32_mfma() == "split3":
            check_tables(y, what="winograd output")
    before = _modes(cv, cv.get_fp32_mfma(), {cv.OPT_SPLITK: 0})
    try:
        for n in range(N):                           # an image alone: other tile counts, other neighbours -- the same bits
            alone = cv.wino_conv_group([t[n:n + 1].contiguous() for t in xg], U)
            for y, a in zip(ys, alone):
                assert torch.equal(a, y[n:n + 1]), "winograd image %d" % n
    finally:
        _restore(cv, before)
    # a bias keeps the all-zero image's outputs at the epilogue's value: still its own scale, still exact
    ys_b = cv.wino_conv_group(xg, U, shift=b.to(dev))
    for x, y in zip(xs, ys_b):
        close_per_image(nchw(y), F.conv2d(x.double(), w.double(), b.double(), 1, 1), TOL_TILE, "winograd + bias")


def test_winograd_transform_words_bound_the_transform(s3, dev):
    """The row words of B^T d B (one per tile row, its image's bound) and the tensor words of B^T d B / A dy A^T (weight gradient):
    every element within its word, the word at most 2^8 above the source image's maximum, rows past T zero."""
    cv = s3
    C, N = 64, 4
    xs = [nhwc(adversarial((N, C, h, ww), 40 + i)).to(dev) for i, (h, ww) in enumerate([(9, 11), (3, 5), (1, 1)])]
    tiles = [x.shape[0] * ((x.shape[1] + 3) // 4) * ((x.shape[2] + 3) // 4) for x in xs]
    T = sum(tiles)
    Tpad = cv.wino_tpad(T)
    for dy_form in (0, 1):
        V = torch.zeros(36 * Tpad * C, device=dev)
        rows, tword = cv._wino_transform_in(xs, V, C, Tpad, dy_form, want_rows=dy_form == 0, want_tensor=True)
        Vv = V.view(36, Tpad, C).abs().amax(dim=(0, 2)).cpu()
        src_exp = []                                 # per tile row: the exponent field of its image's largest |value|
        for x in xs:
            per_img = (x.shape[1] + 3) // 4 * ((x.shape[2] + 3) // 4)
            for n in range(x.shape[0]):
                src_exp += [max_exp(x[n])] * per_img
        tw = tword.cpu().view(torch.float32)
        assert float(tw[0]) >= float(Vv.max()), (float(tw[0]), float(Vv.max()))
        assert max_exp(tw) <= max(src_exp) + 8
        if dy_form == 0:
            rw = rows.cpu()
            assert int(rw[T:].abs().sum()) == 0
            rf = rw[:T].view(torch.float32)
            assert bool((Vv[:T] <= rf).all()), "a transformed row exceeds its word"
            re = ((rw[:T] >> 23) & 0xff).tolist()
            for t in range(T):
                assert re[t] <= src_exp[t] + 8 and (src_exp[t] > 0 or re[t] == 0), (t, re[t], src_exp[t])


def test_elementwise_producers(s3, dev):
    cv = s3
    N = 4
    # stem staging
    img = adversarial((N, 3, 9, 13), 50)
    x4 = cv.nchw_to_nhwc4(img.to(dev))
    check_tables(x4, what="nchw_to_nhwc4")
    # max-pool forward (table carried from the input: a bound) and backward
    z = torch.relu(adversarial((N, 64, 9, 11), 51)).abs()
    zg = nhwc(z).to(dev)
    cv.amax_words(zg)
    y, arg = cv.maxpool_fwd(zg, want_argmax=True)
    check_tables(y, exact=False, what="maxpool_fwd")
    g = nhwc(adversarial(tuple(nchw(y).shape), 52)).to(dev)
    check_tables(cv.maxpool_bwd(zg, g, arg, relu_mask=False), what="maxpool_bwd")
    # upsample + crop backward into an odd-sized coarse map
    dst = nhwc(adversarial((N, 32, 5, 7), 53)).to(dev)
    src = nhwc(adversarial((N, 32, 9, 13), 54)).to(dev)
    want = nchw(dst).double() + F.avg_pool2d(F.pad(nchw(src).double(), (0, 1, 0, 1)), 2, 2, divisor_override=1)
    cv.upsample_add_bwd(src, dst)
    close_per_image(nchw(dst), want, 1e-6, "upsample_add_bwd")
    check_tables(dst, what="upsample_add_bwd")
    # sigmoid backward + channel padding of a concatenated head output
    rows, C, ld = 35, 36, 64
    dy = adversarial((N, rows * C, 1, 1), 55).view(N, rows * C).to(dev)
    s = torch.sigmoid(rnd((N, rows * C), 56)).to(dev)
    out = cv.sigmoid_bwd_pad(dy.data_ptr(), s.data_ptr(), N, rows, C, ld, rows * C, dev)
    check_tables(out.view(N, rows * ld), words=out._rn_amax_words, what="sigmoid_bwd_pad")
    # add_
    a = nhwc(adversarial((N, 16, 7, 9), 57)).to(dev)
    cv.add_(a, nhwc(adversarial((N, 16, 7, 9), 58) * 3.0).to(dev))
    check_tables(a, what="add_")
    # ReLU mask: the table stays a bound
    m = nhwc(rnd((N, 16, 7, 9), 59)).to(dev)
    cv.relu_mask_(a, m)
    check_tables(a, exact=False, what="relu_mask_")
    # rn_amax on a torch-made tensor: 105 floats per image (image starts misaligned: the scalar branch)
    t = adversarial((5, 3, 7, 5), 60).to(dev)
    check_tables(t, words=cv.amax_words(t), what="amax_words")


# ---------------------------------------------------------------------------------------------------------------- C. stale tables
def test_reused_destination_drops_stale_tables(s3, dev):
    """Mirror of test_gpu_bitmasks.py::test_reusing_an_output_tensor_drops_the_old_bits for the amax words: write y with tables, then
    2^12-larger values through every path that leaves none.  No stale ._rn_amax may survive, and a consumer of y matches fp64."""
    cv = s3
    cin, cout, N, H, W = 64, 128, 2, 9, 11
    x1 = adversarial((N, cin, H, W), 70)
    x2 = x1 * 4096.0
    w = weights(cout, cin, 1, 71)
    w2 = weights(96, cout, 3, 72)
    wg, w2p = w.to(dev), cv.pack_weights(w2.to(dev), 0)
    wp = cv.pack_weights(wg, 0)
    w3 = w.repeat(1, 1, 3, 3) / 9.0                 # a 3x3 layer for the Winograd path
    U = cv.wino_weights(w3.to(dev), 0)
    geom = (H, W, cout, 1, 1, 1, 1, 0, 0)
    x1g, x2g = nhwc(x1).to(dev), nhwc(x2).to(dev)
    y_small = F.conv2d(x2.double(), w.double())

    def rewrite(path, y):
        if path == "y_batch_stride":
            cv.conv_igemm(x2g, wp, y, geom, y_batch_stride=H * W * cout)
        elif path == "out_map":
            cv.conv_igemm(x2g, wp, y, geom, out_map=(1, 0, 0, H, W))
        elif path == "grouped":
            cv.conv_igemm_grouped([dict(x=x2g, y=y, geom=geom, y_batch_stride=H * W * cout)], wp)
        elif path == "winograd":
            cv.wino_conv_group([x2g], U, outs=[y], y_batch_stride=H * W * cout)
        return y

    for path in ("y_batch_stride", "out_map", "grouped", "winograd"):
        y = cv.fprop(x1g, wp, cout, 1, 1, 0)
        assert getattr(y, "_rn_amax", None) is not None
        rewrite(path, y)
        a = getattr(y, "_rn_amax", None)
        if a is not None:                            # whatever words y carries now must describe what it holds
            check_tables(y, what=path)
        want_y = F.conv2d(x2.double(), w3.double(), None, 1, 1) if path == "winograd" else y_small
        close_per_image(nchw(y), want_y, TOL_TILE, path)
        z = cv.fprop(y, w2p, 96, 3, 1, 1)
        close_per_image(nchw(z), F.conv2d(want_y, w2.double(), None, 1, 1), TOL_TILE, path + " -> consumer")


def test_inplace_torch_edits_invalidate_the_tables(s3, dev):
    cv = s3
    cin, cout, N, H, W = 64, 128, 4, 9, 11
    x = adversarial((N, cin, H, W), 80)
    w, w2 = weights(cout, cin, 3, 81), weights(96, cout, 3, 82)
    wp, w2p = cv.pack_weights(w.to(dev), 0), cv.pack_weights(w2.to(dev), 0)
    y_ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    y = cv.fprop(nhwc(x).to(dev), wp, cout, 3, 1, 1)
    y.mul_(2.0 ** 20)
    close_per_image(nchw(cv.fprop(y, w2p, 96, 3, 1, 1)), F.conv2d(y_ref * 2.0 ** 20, w2.double(), None, 1, 1), TOL_TILE, "mul_")
    y = cv.fprop(nhwc(x).to(dev), wp, cout, 3, 1, 1)
    y[0] = y[0] * 2.0 ** 30                          # one image only, by index assignment
    want = y_ref.clone()
    want[0] *= 2.0 ** 30
    close_per_image(nchw(cv.fprop(y, w2p, 96, 3, 1, 1)), F.conv2d(want, w2.double(), None, 1, 1), TOL_TILE, "index assignment")


# ---------------------------------------------------------------------------------------------------------------- D. graphs
class _Layers:
    """fprop -> fprop -> one Winograd conv: every consumer reads its producer's tables."""

    def __init__(self, cv, dev):
        self.cv = cv
        self.wp1 = cv.pack_weights(weights(128, 64, 3, 90).to(dev), 0)
        self.wp2 = cv.pack_weights(weights(64, 128, 1, 91).to(dev), 0)
        self.U = cv.wino_weights(weights(64, 64, 3, 92).to(dev), 0)

    def __call__(self, x):
        cv = self.cv
        y1 = cv.fprop(x, self.wp1, 128, 3, 1, 1, act=cv.ACT_RELU)
        y2 = cv.fprop(y1, self.wp2, 64, 1, 1, 0)
        return cv.wino_conv_group([y2], self.U)[0]


SCALES = (2.0 ** 20, 1.0, 2.0 ** -20, 2.0 ** 10, 2.0 ** -30)      # shrinking and growing from replay to replay


def _frames(dev):
    return nhwc(adversarial((4, 64, 9, 11), 93)).to(dev)


def test_two_captures_on_the_default_capture_stream_replay_like_eager(s3, dev):
    layers = _Layers(s3, dev)
    base = _frames(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                      # warm-up off the capture stream (torch's recipe)
        layers(base)
    torch.cuda.current_stream().wait_stream(s)
    xa, xb = base.clone(), base.clone()
    ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(ga):
        out_a = layers(xa)
    with torch.cuda.graph(gb):                      # the same shared capture stream
        out_b = layers(xb)
    for f in SCALES:                                # the second graph replayed alone, several times
        xb.copy_(base * f)
        gb.replay()
        assert torch.equal(out_b, layers(base * f)), "second graph, scale %g" % f
    for f in SCALES[::-1]:
        xa.copy_(base * f)
        ga.replay()
        assert torch.equal(out_a, layers(base * f)), "first graph, scale %g" % f


def test_capture_on_a_stream_that_ran_eagerly_replays_like_eager(s3, dev):
    layers = _Layers(s3, dev)
    base = _frames(dev)
    s = torch.cuda.Stream()
    x = base.clone()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layers(x)                                   # eager work on the stream the capture will use
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = layers(x)
    for f in SCALES:
        x.copy_(base * f)
        g.replay()
        assert torch.equal(out, layers(base * f)), "scale %g" % f


def test_captured_train_step_and_eval_forward_interleaved(dev):
    """A captured training step and a captured eval forward in one process (resnet18, 256 x 384, batch 2, deterministic): replayed
    interleaved, the eval graph on frames of different brightness gives the same bits as an eager forward with the same weights.
    (The engine's cache of packed weights is emptied before the eval capture, so that graph packs from the current parameters on
    every replay, and the eager forward after it reads what the replay packed: both see the same weights.)"""
    from retinanet_mi355x import conv, modules, optim, synth
    before = (conv.get_fp32_mfma(), conv.get_option(conv.OPT_DETERMINISTIC))
    conv.set_fp32_mfma("split3")
    conv.set_deterministic(True)
    try:
        H, W = 256, 384
        net = modules.resnet18(num_classes=4)
        net.load_state_dict(synth.state_dict("resnet18", 4, 12, seed=3))
        net = net.to(dev)
        net.train()
        net.freeze_bn()
        net.use_flat_gradients()
        opt = optim.ClipAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
        img_t = synth.frames(2, H, W, seed=4).to(dev)
        ann = synth.labels_dir(2, 6, H, W, 4, seed=5, size_px=(30, 90)).to(dev)
        base = synth.frames(2, H, W, seed=6).to(dev)
        img_e = base.clone()

        def step():
            opt.zero_grad(set_to_none=True)
            loss = sum(l.mean() for l in net([img_t, ann]))
            loss.backward()
            opt.step()
            return loss

        def evalf():                                # the detector's eval forward: both heads' outputs
            with torch.no_grad():
                reg, cls, _ = net._engine.forward(net._tensor_dict(), img_e, save=False)
            return reg, cls

        for _ in range(2):                          # eager warm-up of both
            step()
            evalf()
        gt, ge = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(gt):
            step()
        net._engine.cache.store.clear()
        with torch.cuda.graph(ge):
            boxes_g, cls_g = evalf()
        prev = None
        for i, f in enumerate((1.0, 2.0 ** -16, 4.0, 2.0 ** -12, 1.0)):
            # The weights move between eval replays -- but only before a BRIGHTER frame.  A darker frame follows the last eval replay
            # directly, with no training replay in between (and the first eval replay precedes every training replay): tables that
            # are not zeroed by the eval graph itself keep the brighter frame's exponents exactly where that changes the result.
            if prev is not None and f > prev:
                gt.replay()
            prev = f
            img_e.copy_(base * f)
            ge.replay()
            ge.replay()                             # and the eval graph twice in a row
            boxes_e, cls_e = evalf()                # eager, same weights, same frames
            assert torch.equal(cls_g, cls_e), "classification, replay %d (brightness %g)" % (i, f)
            assert torch.equal(boxes_g, boxes_e), "regression, replay %d (brightness %g)" % (i, f)
    finally:
        conv.set_fp32_mfma(before[0])
        conv.set_option(conv.OPT_DETERMINISTIC, before[1])


# ---------------------------------------------------------------------------------------------------------------- E. corners
def test_split3_corners(s3, dev):
    """What split3 does where the tables meet non-finite, huge, tiny, subnormal and zero images (the split mode's corners:
    test_gpu_conv.py::test_split_mode_corners_that_differ_from_ieee_fp32; DESIGN.md 4.6, the deviations table):
      * an inf in image k: the scale stays finite (rn_f16_scale_exp: 2^-114), the inf's own row turns NaN (inf - fp16(inf) in the
        residual) -- and every FINITE element of image k falls below fp16's range at that scale: the rest of image k keeps only the
        epilogue's value.  The other images are untouched;
      * a finite 3.4e38: the scale (2^-113) is finite and so are the fp16 terms, but the epilogue multiplies the accumulator by the
        row's inverse scale (2^113) BEFORE the weight's (2^-15 here): the intermediate overflows and that pixel is inf where IEEE
        fp32 gives 1.7e38.  Every other pixel stays finite;
      * an image below 2^-112 (scaled by 2^126 only): still within the tolerance;
      * a subnormal-only image: its table is byte 0 at most, like an all-zero image's: scale 1, the subnormals flush -- the epilogue's
        value only (IEEE fp32 would give the products, ~1e-38 here);
      * an all-zero image: exactly the epilogue's value."""
    cv = s3
    cin, cout, N, H, W = 256, 128, 4, 8, 16                 # K = 256: the split kernels
    w = torch.full((cout, cin, 1, 1), 0.5)
    wp = cv.pack_weights(w.to(dev), 0)
    bias = rnd((cout,), 100).to(dev)

    def run(x, shift=None):
        return cv.fprop(x.to(dev), wp, cout, 1, 1, 0, shift=shift).cpu()

    base = rnd((N, H, W, cin), 101).abs() + 0.5
    ref = lambda x: torch.einsum("nhwc,oc->nhwo", x.double(), w.view(cout, cin).double())
    # an inf in image 1: NaN at its pixel, the rest of image 1 the epilogue's value (0: flushed), every other image accurate
    x = base.clone()
    x[1, 2, 3, 5] = float("inf")
    y = run(x)
    assert torch.isnan(y[1, 2, 3]).all()
    rest = torch.ones(H, W, dtype=torch.bool)
    rest[2, 3] = False
    assert torch.equal(y[1][rest], torch.zeros_like(y[1][rest])), "the finite part of the image with the inf"
    others = [0, 2, 3]
    close_per_image(y[others], ref(x)[others], TOL_TILE, "next to an inf image")
    # a finite 3.4e38 operand: inf at its pixel (the epilogue's order of the two inverse scales), finite elsewhere
    x = base.clone()
    x[2, 0, 0, 0] = 3.4e38
    y = run(x)
    assert torch.isinf(y[2, 0, 0]).all()
    rest = torch.ones(H, W, dtype=torch.bool)
    rest[0, 0] = False
    assert torch.isfinite(y[2][rest]).all()
    close_per_image(y[[0, 1, 3]], ref(x)[[0, 1, 3]], TOL_TILE, "next to a 3.4e38 image")
    # an image below 2^-112 (scaled by 2^126 only) next to normal ones: error measured ~1e-7 relative, pinned at 1e-4
    x = base.clone()
    x[3] *= 2.0 ** -120
    close_per_image(run(x), ref(x), TOL_TILE, "tiny image")
    # a subnormal-only image: byte 0 cannot tell it from zero -- the epilogue's value only
    x = base.clone()
    x[0] = 1e-40
    y = run(x, shift=bias)
    assert torch.equal(y[0], bias.cpu().expand(H, W, cout)), "subnormal-only image"
    close_per_image(y[1:], (ref(x) + bias.cpu().double())[1:], TOL_TILE, "next to a subnormal image")
    # an all-zero image: exactly the epilogue's value
    x = base.clone()
    x[2] = 0.0
    y = run(x, shift=bias)
    assert torch.equal(y[2], bias.cpu().expand(H, W, cout)), "all-zero image"

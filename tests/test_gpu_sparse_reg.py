"""Tile activity flags of the regression tower's backward pass: a Winograd backward that skips the all-zero tiles of a
sparse gradient must give what the dense one gives.

Cases 1-3 run ONE group of two pyramid levels, N = 2, C = Cout = 256: 34 x 60 (9 x 15 tiles per image, 270 in all; H is no multiple of
4) and 17 x 30 (5 x 8 tiles per image, 80 in all) -- T = 350 rows of V / Z / M in planes of 768: several GEMM row blocks and K-steps, some
of them partly active.  The non-zero pixels of dy: an image corner; column 0 / row 3 of a tile (the left and lower neighbours wake); the
last, partial tile row; the first row of image 1; a pixel whose ReLU mask is 0.  One level of one variant is entirely zero.

Bit identity is asked in the fixed-order mode (conv.set_deterministic) with the Winograd workspaces filled with NaN before the sparse
call: a skipped tile's stale rows must never reach a sum.  np.array_equal treats +0 and -0 as equal -- the one difference the invariant
allows.  The atomic mode is held to the tolerances tests/test_gpu_conv.py uses for the Winograd path (1e-4 of the largest magnitude,
2e-5 for the column sums).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc

pytestmark = pytest.mark.gpu

N, C = 2, 256
LEVELS = [(34, 60), (17, 30)]
PIXELS = [[(0, 0, 0), (0, 11, 20), (0, 33, 30), (1, 0, 17), (1, 20, 41)],      # level one; the last one is masked (MASKED below)
          [(1, 16, 29), (0, 7, 8)]]                                            # level two: last partial tile row / column, a tile corner
MASKED = (0, 1, 20, 41)                                                        # (level, n, h, w): the activation there is <= 0


def rnd(shape, seed, std=1.0):
    from retinanet_mi355x import synth
    return torch.from_numpy(synth.normal(shape, seed, std))


def tiles_of(shape):
    return shape[0] * ((shape[1] + 3) // 4) * ((shape[2] + 3) // 4)


def rule_flags(ts, length):
    """The producers' rule restated: a non-zero pixel sets its own tile; column 0 / 3 of a tile the left / right neighbour, rows
    likewise, the four corner pixels the diagonal neighbours too.  ts: [N,H,W,C] tensors in group order -> uint8 [length]."""
    out = np.zeros(length, dtype=np.uint8)
    base = 0
    for t in ts:
        n_, H, W = t.shape[:3]
        TH, TW = (H + 3) // 4, (W + 3) // 4
        f = out[base:base + n_ * TH * TW].reshape(n_, TH, TW)
        for n, h, w in (t.cpu() != 0).any(dim=3).nonzero().tolist():
            th, tw = h // 4, w // 4
            for a in (-1, 0, 1):
                for b in (-1, 0, 1):
                    ok_r = a == 0 or (h % 4 == 0 and th > 0 if a < 0 else h % 4 == 3 and th + 1 < TH)
                    ok_c = b == 0 or (w % 4 == 0 and tw > 0 if b < 0 else w % 4 == 3 and tw + 1 < TW)
                    if ok_r and ok_c:
                        f[n, th + a, tw + b] = 1
        base += n_ * TH * TW
    return out


def patch_flags(ts, length):
    """Independently: does the tile's 6x6 patch (its 4x4 block plus the one-pixel halo) hold a non-zero value?"""
    out = np.zeros(length, dtype=np.uint8)
    base = 0
    for t in ts:
        n_, H, W = t.shape[:3]
        TH, TW = (H + 3) // 4, (W + 3) // 4
        nz = (t.cpu() != 0).any(dim=3).float()
        pad = torch.zeros(n_, 1, 4 * TH + 2, 4 * TW + 2)
        pad[:, 0, 1:1 + H, 1:1 + W] = nz
        out[base:base + n_ * TH * TW] = F.max_pool2d(pad, 6, 4).reshape(-1).numpy().astype(np.uint8)
        base += n_ * TH * TW
    return out


def sign_bits(m):
    """The sign words a producer would have left on m (conv._sign_words): bit (e & 31) of word (e >> 5) = m[e] > 0."""
    b = (m.flatten() > 0).view(-1, 32).to(torch.int64)
    w = (b << torch.arange(32, device=m.device, dtype=torch.int64)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


@pytest.fixture(scope="module")
def data(dev):
    """The layer's inputs (which are also the ReLU masks of its data gradient), weights, addends and the gradients of the variants."""
    shapes = [(N, h, w, C) for h, w in LEVELS]
    xs = [rnd(s, 300 + i) for i, s in enumerate(shapes)]
    lv, n, h, w = MASKED
    xs[lv][n, h, w, :] = -xs[lv][n, h, w, :].abs() - 0.1
    wt = rnd((C, C, 3, 3), 310, (2.0 / (9 * C)) ** 0.5)
    adds = [rnd(s, 320 + i) for i, s in enumerate(shapes)]
    vals = [rnd(s, 330 + i) for i, s in enumerate(shapes)]

    def sparse(levels):
        gs = [torch.zeros(s) for s in shapes]
        for lvl in levels:
            for (n_, h_, w_) in PIXELS[lvl]:
                gs[lvl][n_, h_, w_, :] = vals[lvl][n_, h_, w_, :]
        return gs
    grads = {"level_two_zero": sparse([0]), "both": sparse([0, 1]), "zero": [torch.zeros(s) for s in shapes], "dense": vals}
    T = sum(tiles_of(s) for s in shapes)
    return {"xs": [x.to(dev) for x in xs], "w": wt.to(dev), "adds": [a.to(dev) for a in adds], "T": T,
            "grads": {k: [g.to(dev) for g in v] for k, v in grads.items()}}


@pytest.fixture
def cv(dev):
    from retinanet_mi355x import conv
    before = conv.get_fp32_mfma(), conv.PRESPLIT, conv.get_option(conv.OPT_DETERMINISTIC)
    yield conv
    conv.set_fp32_mfma(before[0])
    conv.PRESPLIT = before[1]
    conv.set_deterministic(bool(before[2]))


def set_mode(cv, mode, det):
    cv.set_fp32_mfma(mode)
    cv.PRESPLIT = mode != "native"
    cv.set_deterministic(det)


def nan_fill_workspaces(cv, dev, floats):
    for t in cv._wino_workspace(dev, floats, floats):
        t.fill_(float("nan"))
    for st in cv._WINO_Z.values():
        for b in st["bufs"]:
            if b is not None:
                b.fill_(float("nan"))


def backward(cv, dev, data, gs, flags, add, bits, side=None, nan=False, flags_out=False):
    """One tower layer's backward as the engine runs it: wino_wgrad_group(fuse_dgrad_input) then wino_conv_group(V_ready)."""
    xs = data["xs"]
    masks = [x.clone() for x in xs]
    if bits:
        for m in masks:
            m._rn_sign = sign_bits(m)
    _, V = cv.wino_conv_group(xs, cv.wino_weights(data["w"], 0), keep_v=True)
    Ud = cv.wino_weights(data["w"], 1)
    wp = cv.pack_weights(data["w"], 0)
    dw, cs = torch.zeros_like(wp), torch.zeros(C, device=dev)
    dU = torch.zeros((36, C, C), device=dev)
    Tpad = cv.wino_tpad(data["T"])
    fo = cv.tile_flags(dev, data["T"]) if flags_out else None
    if nan:
        torch.cuda.synchronize()
        nan_fill_workspaces(cv, dev, 36 * Tpad * C)
    v_dy = cv.wino_wgrad_group(gs, xs, dw, cs, V=V, dU=dU, fuse_dgrad_input=True, side=side, flags=flags)
    dxs = cv.wino_conv_group(gs, Ud, adds=data["adds"] if add else None, masks=masks, mask_mode=2, V_ready=v_dy, flags_out=fo)
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
        cv.side_release(side)
    torch.cuda.synchronize()
    res = {"dw": dw, "colsum": cs, "dU": dU}
    res.update({"dx%d" % i: d for i, d in enumerate(dxs)})
    return {k: v.cpu().numpy() for k, v in res.items()}, len(v_dy) > 3, fo


def dev_flags(cv, dev, data, gs):
    f = cv.tile_flags(dev, data["T"])
    f.copy_(torch.from_numpy(rule_flags(gs, f.numel())))
    return f


def close(got, want, tol):
    err, ref = float(np.abs(got - want).max()), float(np.abs(want).max()) + 1e-12
    assert err <= tol * ref, "max err %.3e vs max |ref| %.3e" % (err, ref)


# ------------------------------------------------------------------------------------------------ 1. bit identity, fixed-order mode
@pytest.mark.parametrize("bits", [True, False], ids=["sign_bits", "fp32_masks"])
@pytest.mark.parametrize("add", [True, False], ids=["addend", "no_addend"])
@pytest.mark.parametrize("mode", ["native", "split", "split3"])
def test_sparse_backward_is_bit_identical_in_fixed_order_mode(cv, dev, data, mode, add, bits):
    set_mode(cv, mode, True)
    gs = data["grads"]["level_two_zero" if add else "both"]
    want, _, _ = backward(cv, dev, data, gs, None, add, bits)
    got, skipped, _ = backward(cv, dev, data, gs, dev_flags(cv, dev, data, gs), add, bits, nan=True)
    assert skipped == (mode != "native")                         # the split modes do take the skipping kernels; native stays dense
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_sparse_backward_with_the_reductions_on_a_side_stream(cv, dev, data):
    set_mode(cv, "split3", True)
    gs = data["grads"]["both"]
    side = torch.cuda.Stream(dev)
    want, _, _ = backward(cv, dev, data, gs, None, True, True, side=side)
    backward(cv, dev, data, gs, None, True, True, side=side)     # (both of the side form's Z buffers exist now)
    got, skipped, _ = backward(cv, dev, data, gs, dev_flags(cv, dev, data, gs), True, True, side=side, nan=True)
    assert skipped
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------ 2. atomic mode
@pytest.mark.parametrize("mode", ["split", "split3"])
def test_sparse_backward_in_atomic_mode(cv, dev, data, mode):
    set_mode(cv, mode, False)
    gs = data["grads"]["both"]
    want, _, _ = backward(cv, dev, data, gs, None, True, True)
    got, skipped, _ = backward(cv, dev, data, gs, dev_flags(cv, dev, data, gs), True, True, nan=True)
    assert skipped
    for k in want:
        print(k, float(np.abs(got[k] - want[k]).max()), float(np.abs(want[k]).max()))
        close(got[k], want[k], 2e-5 if k == "colsum" else 1e-4)


# ------------------------------------------------------------------------------------------------ 3. the producers' flags
def test_flags_of_the_producers(cv, dev, data):
    set_mode(cv, "split3", True)
    # depth 0: sigmoid_bwd_pad over the slices of a concatenated [B, A, width] head gradient (9 anchors x 12 values -> 108 channels)
    width, ld = 12, 108
    rows = [h * w for h, w in LEVELS]
    A = 9 * sum(rows)
    dout = torch.zeros((N, A, width), device=dev)
    src = rnd((N, A, width), 340).to(dev)
    off = 0
    picks = []
    for lvl, (h, w) in enumerate(LEVELS):
        for (n_, h_, w_) in PIXELS[lvl]:
            a = off + 9 * (h_ * w + w_) + (h_ + w_) % 9           # one anchor of that pixel
            dout[n_, a] = src[n_, a]
            picks.append((lvl, n_, h_, w_))
        off += 9 * rows[lvl]
    T = data["T"]
    f0 = cv.tile_flags(dev, T)
    gs, off, t_off = [], 0, 0
    for (h, w) in LEVELS:
        t = tiles_of((N, h, w))
        g = cv.sigmoid_bwd_pad(dout.data_ptr() + 4 * off * width, None, N, h * w, 9 * width, ld, A * width, dev, hw=(h, w),
                               flags=f0[t_off:t_off + t])
        gs.append(g.view(N, h, w, ld))
        off += 9 * h * w
        t_off += t
    torch.cuda.synchronize()
    for (lvl, n_, h_, w_) in picks:
        assert bool((gs[lvl][n_, h_, w_] != 0).any())
    assert int(sum((g != 0).any(dim=3).sum() for g in gs)) == len(picks)
    assert np.array_equal(f0.cpu().numpy(), rule_flags(gs, f0.numel()))
    assert np.array_equal(f0.cpu().numpy(), patch_flags(gs, f0.numel()))
    # next depth: wino_out's flags of the tensor it stores, after the mask (no addend: the stored gradient stays sparse)
    g256 = data["grads"]["both"]
    _, skipped, fo = backward(cv, dev, data, g256, dev_flags(cv, dev, data, g256), False, True, flags_out=True)
    assert skipped
    xs = data["xs"]
    Ud = cv.wino_weights(data["w"], 1)
    dxs = cv.wino_conv_group(g256, Ud, masks=xs, mask_mode=2)    # the dense path's stored tensor
    torch.cuda.synchronize()
    got = fo.cpu().numpy()
    assert np.array_equal(got, rule_flags(dxs, got.size))
    need = patch_flags(dxs, got.size)
    assert not np.any((need == 1) & (got == 0))                  # every tile with a non-zero patch is flagged
    assert 0 < int(got.sum()) < T                                # (sparse, but not empty: the check above is not vacuous)
    lv, n, h, w = MASKED
    assert not bool((dxs[lv][n, h, w] != 0).any())


# ------------------------------------------------------------------------------------------------ 4. extremes
def test_all_zero_gradient(cv, dev, data):
    set_mode(cv, "split3", True)
    gs = data["grads"]["zero"]
    xs, Ud = data["xs"], cv.wino_weights(data["w"], 1)
    _, V = cv.wino_conv_group(xs, cv.wino_weights(data["w"], 0), keep_v=True)
    wp = cv.pack_weights(data["w"], 0)
    dw, cs, dU = torch.zeros_like(wp), torch.zeros(C, device=dev), torch.zeros((36, C, C), device=dev)
    torch.cuda.synchronize()
    nan_fill_workspaces(cv, dev, 36 * cv.wino_tpad(data["T"]) * C)
    v_dy = cv.wino_wgrad_group(gs, xs, dw, cs, V=V, dU=dU, fuse_dgrad_input=True, flags=cv.tile_flags(dev, data["T"]))
    assert len(v_dy) > 3
    dxs = cv.wino_conv_group(gs, Ud, adds=data["adds"], V_ready=v_dy)
    torch.cuda.synchronize()
    for t in (dw, cs, dU):
        assert not bool((t != 0).any())
    for dx, a in zip(dxs, data["adds"]):
        assert np.array_equal(dx.cpu().numpy(), a.cpu().numpy())


def test_dense_gradient_with_every_flag_set(cv, dev, data):
    set_mode(cv, "split3", True)
    gs = data["grads"]["dense"]
    flags = dev_flags(cv, dev, data, gs)
    assert int(flags.sum()) == data["T"]
    want, _, _ = backward(cv, dev, data, gs, None, True, True)
    got, skipped, _ = backward(cv, dev, data, gs, flags, True, True, nan=True)
    assert skipped
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------ 5. whole step
def _net(dev):
    from retinanet_mi355x import modules
    sd, img, ann = gc.model_inputs("resnet18", True)
    net = modules.resnet18(num_classes=4, directional=True)
    net.load_state_dict(sd)
    net = net.to(dev)
    net.train()
    net.freeze_bn()
    return net, img.to(dev), ann.to(dev)


def _grads(net, img, ann):
    for p in net.parameters():
        p.grad = None
    sum(l.mean() for l in net([img, ann])).backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("labels", ["all_images", "an_image_without_positives"])
def test_whole_step_sparse_against_dense(cv, dev, labels):
    from retinanet_mi355x import engine
    set_mode(cv, "split3", True)
    net, img, ann = _net(dev)
    if labels != "all_images":
        ann = ann.clone()
        ann[1] = -1
    before = engine.SPARSE_REG
    try:
        engine.SPARSE_REG = False
        want = _grads(net, img, ann)
        engine.SPARSE_REG = True
        got = _grads(net, img, ann)
        flags = [f.cpu().numpy() for f in net._engine._reg_flags]
    finally:
        engine.SPARSE_REG = before
    assert len(flags) == 5 and 0 < int(flags[0].sum()) and all(int(f.sum()) < f.size for f in flags)
    assert set(got) == set(want) and len(want) > 20
    for n in want:
        assert np.array_equal(got[n], want[n]), n


# ------------------------------------------------------------------------------------------------ 6. captured graph
def test_flags_are_zeroed_again_inside_a_captured_graph(cv, dev):
    from retinanet_mi355x import engine
    assert engine.SPARSE_REG
    set_mode(cv, "split3", True)
    net, img, ann = _net(dev)
    net.use_flat_gradients()
    fewer = ann.clone()
    fewer[1] = -1
    fewer[0, 2:] = -1
    buf = ann.clone()

    def step():
        for p in net.parameters():
            p.grad = None
        sum(l.mean() for l in net([img, buf])).backward()
    step(); step()                                               # eager warm-up: job tables, gradient buffer
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    many = [int(f.sum()) for f in net._engine._reg_flags]
    buf.copy_(fewer)
    g.replay()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None}
    got_flags = [f.cpu().numpy().copy() for f in net._engine._reg_flags]
    step()                                                       # eager, same labels
    torch.cuda.synchronize()
    want = {n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None}
    want_flags = [f.cpu().numpy() for f in net._engine._reg_flags]
    assert 0 < int(want_flags[0].sum()) < many[0]                # the set of positives did shrink
    for a, b in zip(got_flags, want_flags):
        assert np.array_equal(a, b)                              # flags of the first replay did not survive into the second
    assert set(got) == set(want)
    for n in want:
        assert np.array_equal(got[n], want[n]), n

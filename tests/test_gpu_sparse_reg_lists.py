"""Work lists of the regression tower's sparse backward: the flagged stages that walk a device-side list -- the fused
input transform over the active 16-row units, the Winograd-stage GEMM over the active 128-row blocks -- must store exactly what the
early-exit instances and the dense path store.  The rules are restated in tests/sparse_reg_list_cases.py.

Shapes: N = 2, 128 channels (the narrowest the flagged path takes), a group of three levels of 34 x 60, 9 x 15 and 3 x 4 pixels (H and W no
multiples of 4): 270 + 24 + 2 = 296 tiles in planes of wino_tpad(296) = 768 rows -- six 128-row blocks, three of which hold tiles, the
third only 40, and 472 padding rows.  The chain's first gradient has 128 or 108 channels: 108 (the head's padded output) is no multiple of
32 and takes the other GEMM kernel.  Bits are compared in the split3 product mode with fixed-order reductions; np.array_equal treats +0
and -0 as equal, the one difference the flags' invariant allows.
"""
import numpy as np
import pytest
import torch

import golden_cases as gc
import sparse_reg_list_cases as sc

pytestmark = pytest.mark.gpu

N, C = 2, 128
LEVELS = [(34, 60), (9, 15), (3, 4)]
SHAPES = [(N, h, w) for h, w in LEVELS]
T = sum(sc.tiles_of(s) for s in SHAPES)
# non-zero pixels of the first gradient, (n, h, w) per level: an image corner, column 0 / row 3 of a tile, the last partial tile row, the
# first row of image 1 (the tile before it in memory belongs to image 0), the smallest level's only tile
PIXELS = {"spread": [[(0, 0, 0), (0, 11, 20), (0, 33, 30), (1, 0, 17), (1, 20, 41)], [(1, 8, 14), (0, 3, 4)], [(1, 2, 3)]],
          "one_block": [[(0, 5, 9)], [], []],
          "zero": [[], [], []]}


def rnd(shape, seed, std=1.0):
    from retinanet_mi355x import synth
    return torch.from_numpy(synth.normal(shape, seed, std))


@pytest.fixture
def cv(dev):
    from retinanet_mi355x import conv
    before = conv.get_fp32_mfma(), conv.PRESPLIT, conv.get_option(conv.OPT_DETERMINISTIC)
    conv.set_fp32_mfma("split3")
    conv.PRESPLIT = True
    conv.set_deterministic(True)
    yield conv
    conv.set_fp32_mfma(before[0])
    conv.PRESPLIT = before[1]
    conv.set_deterministic(bool(before[2]))


# ------------------------------------------------------------------------------------------------ 1. the list builder
def test_list_builder_against_flatnonzero(cv, dev):
    Tpad = cv.wino_tpad(T)
    assert Tpad == 768 and T % 128 != 0
    plane = (sc.tiles_of(SHAPES[0]) // N, 9, 15)                 # image 1 of the first level: 9 x 15 tiles from row 135
    pats = sc.builder_patterns(T, Tpad, plane)
    pats.update({"big_" + k: v for k, v in sc.builder_patterns(21896, 22272, (2 * 34 * 60, 34, 60)).items()})   # the benchmark's planes
    for name, f in pats.items():
        flags = torch.from_numpy(f).to(dev)
        buf = torch.full((cv.tile_lists_numel(f.size),), -7, dtype=torch.int32, device=dev)
        tl = cv.tile_lists(flags, buf=buf)
        torch.cuda.synchronize()
        want = sc.lists_of(f)
        assert tl.lengths() == tuple(len(w) for w in want), name
        for got, w in zip((tl.tiles, tl.units, tl.blocks), want):
            g = got.cpu().numpy()
            assert np.array_equal(g[:len(w)], w), name            # exact and ascending
            assert np.all(g[len(w):] == -7), name                 # nothing written past the count


# ------------------------------------------------------------------------------------------------ 2. three stacked layers
@pytest.fixture(scope="module")
def data(dev):
    """Three stacked 3x3 layers: inputs (= the ReLU masks of their data gradients) and weights; layer 0 is the chain's first (the one
    whose output gradient is given), with 128 or 108 output channels."""
    xs = [[rnd(s + (C,), 400 + 10 * k + i).to(dev) for i, s in enumerate(SHAPES)] for k in range(3)]
    ws = {c0: [rnd((c0 if k == 0 else C, C, 3, 3), 440 + k + c0, (2.0 / (9 * C)) ** 0.5).to(dev) for k in range(3)] for c0 in (128, 108)}
    vals = {c0: [rnd(s + (c0,), 450 + i + c0) for i, s in enumerate(SHAPES)] for c0 in (128, 108)}
    return {"xs": xs, "ws": ws, "vals": vals}


def first_gradient(data, dev, c0, pixels):
    gs = [torch.zeros(s + (c0,)) for s in SHAPES]
    for lvl, pts in enumerate(PIXELS[pixels]):
        for (n, h, w) in pts:
            gs[lvl][n, h, w, :] = data["vals"][c0][lvl][n, h, w, :]
    return [g.to(dev) for g in gs]


def nan_fill_workspaces(cv, dev, floats):
    for t in cv._wino_workspace(dev, floats, floats):
        t.fill_(float("nan"))


def chain(cv, dev, data, c0, pixels, mode, grid=0):
    """The backward of the three layers as the engine chains them.  mode: dense (no flags), exit (flags, every tile visited), lists."""
    Tpad = cv.wino_tpad(T)
    gs = first_gradient(data, dev, c0, pixels)
    F = [cv.tile_flags(dev, T) for _ in range(3)] if mode != "dense" else [None] * 3
    if mode != "dense":
        F[0].copy_(torch.from_numpy(sc.rule_flags([(g != 0).any(dim=3).cpu().numpy() for g in gs], Tpad)))
    res, lens = {}, []
    fl = F[0]
    for k in range(3):
        xs, w = data["xs"][k], data["ws"][c0][k]
        cout = w.shape[0]
        _, V = cv.wino_conv_group(xs, cv.wino_weights(w, 0), keep_v=True)
        Ud = cv.wino_weights(w, 1)
        dw, cs = torch.zeros_like(cv.pack_weights(w, 0)), torch.zeros(cout, device=dev)
        dU = torch.zeros((36, cout, C), device=dev)
        torch.cuda.synchronize()
        nan_fill_workspaces(cv, dev, 36 * Tpad * C)              # V of dy, Z and M: nothing unwritten may reach a result
        tl = cv.tile_lists(fl, Tpad, grid=grid) if mode == "lists" else None
        v_dy = cv.wino_wgrad_group(gs, xs, dw, cs, V=V, dU=dU, fuse_dgrad_input=True, flags=fl, lists=tl)
        assert len(v_dy) == {"dense": 3, "exit": 4, "lists": 5}[mode]
        fo = F[k + 1] if (fl is not None and k < 2) else None
        outs = [torch.full(tuple(x.shape), float("nan"), device=dev) for x in xs]      # the intermediate dx buffers too
        gs = cv.wino_conv_group(gs, Ud, outs=outs, masks=xs, mask_mode=2, V_ready=v_dy, flags_out=fo)
        torch.cuda.synchronize()
        if tl is not None:
            want = sc.lists_of(fl.cpu().numpy())
            assert tl.lengths() == tuple(len(x) for x in want)
            lens.append(tl.lengths())
        res.update({"dw%d" % k: dw, "cs%d" % k: cs, "dU%d" % k: dU})
        fl = fo
    res.update({"dx%d" % i: g for i, g in enumerate(gs)})
    res = {k: v.cpu().numpy() for k, v in res.items()}
    res["M"] = cv._wino_workspace(dev, 0, 0)[1][:36 * Tpad * C].cpu().numpy()        # (what the last GEMM left)
    res["flags"] = [None if f is None else f.cpu().numpy() for f in F]
    res["lens"] = lens
    return res


def same(got, want):
    for k in want:
        if k not in ("M", "flags", "lens"):
            assert not np.isnan(want[k]).any(), k
            bad = np.argwhere(got[k] != want[k])
            assert bad.shape[0] == 0, "%s: %d elements differ (%d NaN), the first at %s: %r against %r" % (
                k, bad.shape[0], int(np.isnan(got[k]).sum()), tuple(bad[0]), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


@pytest.mark.parametrize("c0", [128, 108])
def test_three_layers_lists_against_early_exit_against_dense(cv, dev, data, c0):
    dense = chain(cv, dev, data, c0, "spread", "dense")
    early = chain(cv, dev, data, c0, "spread", "exit")
    lists = chain(cv, dev, data, c0, "spread", "lists")
    same(early, dense)
    same(lists, dense)
    for a, b in zip(early["flags"], lists["flags"]):
        assert np.array_equal(a, b)
    # the case is what it says: sparse at every depth, tiles in all three blocks that hold any, more at each depth
    assert [l[2] for l in lists["lens"]] == [3, 3, 3]
    assert 0 < lists["lens"][0][0] < lists["lens"][1][0] < lists["lens"][2][0] < T


# ------------------------------------------------------------------------------------------------ 4. lists longer and shorter than the grid
@pytest.mark.parametrize("c0", [128, 108])
def test_list_longer_than_a_grid_of_two_workgroups(cv, dev, data, c0):
    """Three blocks x 36 positions = 108 GEMM items on TWO workgroups: the stride loop (TileLists.grid caps the GEMM's grid)."""
    dense = chain(cv, dev, data, c0, "spread", "dense")
    lists = chain(cv, dev, data, c0, "spread", "lists", grid=2)
    same(lists, dense)


def test_exactly_one_block(cv, dev, data):
    dense = chain(cv, dev, data, 128, "one_block", "dense")
    lists = chain(cv, dev, data, 128, "one_block", "lists")
    same(lists, dense)
    assert lists["lens"][0] == (1, 1, 1) and [l[2] for l in lists["lens"]] == [1, 1, 1]


@pytest.mark.parametrize("c0", [128, 108])
def test_zero_blocks_leave_the_outputs_untouched(cv, dev, data, c0):
    dense = chain(cv, dev, data, c0, "zero", "dense")
    lists = chain(cv, dev, data, c0, "zero", "lists")
    same(lists, dense)
    assert lists["lens"] == [(0, 0, 0)] * 3
    assert np.isnan(lists["M"]).all()                            # the GEMM returned at once: M is what it was
    assert not np.isnan(dense["M"][:36 * cv.wino_tpad(T) * 108]).all()
    for k in ("dw0", "dw1", "dw2", "dx0", "dx1", "dx2"):
        assert not lists[k].any(), k


# ------------------------------------------------------------------------------------------------ 7. whole step
def _net(dev):
    from retinanet_mi355x import modules
    sd, img, ann = gc.model_inputs("resnet18", True)
    net = modules.resnet18(num_classes=4, directional=True)
    net.load_state_dict(sd)
    net = net.to(dev)
    net.train()
    net.freeze_bn()
    return net, img.to(dev), ann.to(dev)


def _step(net, img, ann):
    for p in net.parameters():
        p.grad = None
    losses = net([img, ann])
    sum(l.mean() for l in losses).backward()
    torch.cuda.synchronize()
    return ([l.detach().cpu().numpy().copy() for l in losses],
            {n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None})


def _engine_lists(eng, cv):
    """Per depth: (flags, lists as the builder left them) read back from the engine's buffers."""
    out = []
    for f, buf in zip(eng._reg_flags, eng._reg_lists):
        f = f.cpu().numpy()
        b = buf.cpu().numpy()
        nb, nu = f.size // 128, f.size // 16
        cnt = b[:3]
        out.append((f, (b[4 + nb + nu:][:cnt[0]], b[4 + nb:][:cnt[1]], b[4:][:cnt[2]])))
    return out


@pytest.mark.parametrize("labels", ["all_images", "an_image_without_positives"])
def test_whole_step_three_configurations(cv, dev, labels):
    from retinanet_mi355x import engine
    net, img, ann = _net(dev)
    if labels != "all_images":
        ann = ann.clone()
        ann[1] = -1
    before = engine.SPARSE_REG, engine.SPARSE_REG_LISTS
    try:
        engine.SPARSE_REG, engine.SPARSE_REG_LISTS = False, True             # (the lists are inert without the flags)
        off = _step(net, img, ann)
        engine.SPARSE_REG, engine.SPARSE_REG_LISTS = True, False
        early = _step(net, img, ann)
        engine.SPARSE_REG, engine.SPARSE_REG_LISTS = True, True
        on = _step(net, img, ann)
        built = _engine_lists(net._engine, cv)
    finally:
        engine.SPARSE_REG, engine.SPARSE_REG_LISTS = before
    assert len(off[1]) > 20
    for got in (early, on):
        for a, b in zip(got[0], off[0]):
            assert np.array_equal(a, b)
        assert set(got[1]) == set(off[1])
        for n in off[1]:
            assert np.array_equal(got[1][n], off[1][n]), n
    assert len(built) == 5
    for f, got in built:                                         # the lists the step walked are the lists of its flags
        assert 0 < int(f.sum()) < f.size
        for g, w in zip(got, sc.lists_of(f)):
            assert np.array_equal(g, w)


# ------------------------------------------------------------------------------------------------ 8. captured graph
def test_lists_are_rebuilt_inside_a_captured_graph(cv, dev):
    from retinanet_mi355x import engine
    assert engine.SPARSE_REG and engine.SPARSE_REG_LISTS
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
    step(); step()                                               # eager warm-up: job tables, gradient buffer, list buffers
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    many = _engine_lists(net._engine, cv)
    buf.copy_(fewer)                                             # the labels change in place
    g.replay()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None}
    got_lists = _engine_lists(net._engine, cv)
    step()                                                       # eager, same labels
    torch.cuda.synchronize()
    want = {n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None}
    want_lists = _engine_lists(net._engine, cv)
    assert 0 < len(want_lists[0][1][0]) < len(many[0][1][0])     # the set of positives did shrink
    for (fa, la), (fb, lb) in zip(got_lists, want_lists):
        assert np.array_equal(fa, fb)
        for a, b, w in zip(la, lb, sc.lists_of(fb)):
            assert np.array_equal(a, b) and np.array_equal(b, w)
    assert set(got) == set(want)
    for n in want:
        assert np.array_equal(got[n], want[n]), n

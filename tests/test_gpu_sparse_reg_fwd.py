"""Sparse forward of the regression tower: the loss reads the tower's result at the positive anchors only, so each layer
is computed on its need set -- the label tiles P0, dilated once per 3x3 layer below.  The rules are restated in tests/reg_need_cases.py.

1. the need-set kernel against the restatement, byte for byte, and its work lists;
2. one tower layer on a need set against the dense call: bit-identical on the needed tiles, nothing stored elsewhere;
3. a whole training step: finite with every skipped byte poisoned, as close to the dense forward as the project's two product modes are
   to one another, and the three backward configurations bit-identical on top of it.
Captured graphs keep the dense forward (Engine.reg_need): there is nothing of this path to test in them.
Bits are compared in the split3 product mode with fixed-order reductions, as in test_gpu_sparse_reg_lists.py.
"""
import numpy as np
import pytest
import torch

import golden_cases as gc
import reg_need_cases as rc
import sparse_reg_list_cases as sc

pytestmark = pytest.mark.gpu


def rnd(shape, seed, std=1.0):
    from retinanet_mi355x import synth
    return torch.from_numpy(synth.normal(shape, seed, std))


@pytest.fixture
def cv(dev):
    from retinanet_mi355x import conv
    before = conv.get_fp32_mfma(), conv.PRESPLIT, conv.get_option(conv.OPT_DETERMINISTIC), conv.NEED_POISON
    conv.set_fp32_mfma("split3")
    conv.PRESPLIT = True
    conv.set_deterministic(True)
    yield conv
    conv.set_fp32_mfma(before[0])
    conv.PRESPLIT = before[1]
    conv.set_deterministic(bool(before[2]))
    conv.NEED_POISON = before[3]


def box_label(x1, y1, x2, y2, cls=1.0):
    """One directional label row whose corner envelope is the box (synth.labels_dir's geometry)."""
    f = np.float32
    w, h = f(x2 - x1), f(y2 - y1)
    bottom = np.array([x1, y1 + h, x1 + f(.6) * w, y1 + f(.9) * h, x1 + f(.4) * w, y1 + f(.6) * h, x1 + w, y1 + f(.5) * h], dtype=f)
    top = bottom.copy()
    top[1::2] -= f(.5) * h
    row = np.zeros(27, dtype=f)
    row[:16] = np.concatenate((bottom, top))
    row[16:20] = (x1, y1, x2, y2)
    row[20] = cls
    return row


def labels_on_anchors(anc, picks, B, n_rows):
    """[B, n_rows, 27]: image j gets one label per anchor index of picks[j] -- the anchor's own box, so that anchor is positive."""
    ann = np.zeros((B, n_rows, 27), dtype=np.float32)
    ann[:, :, 20] = -1
    for j, idx in enumerate(picks):
        for r, ai in enumerate(idx):
            ann[j, r] = box_label(*anc[ai])
    return ann


# ------------------------------------------------------------------------------------------------ 1. the need-set kernel
@pytest.mark.parametrize("hw", [(40, 56), (160, 224)])
def test_need_sets_against_the_restatement(cv, dev, hw):
    from retinanet_mi355x import arch, ops
    H, W = hw
    B = 3
    hws = arch.pyramid_shapes(H, W)
    anc_t = ops.anchors(H, W, dev)
    anc = anc_t.cpu().numpy().reshape(-1, 4)
    A = anc.shape[0]
    offs = np.cumsum([0] + [h * w * 9 for h, w in hws])
    assert offs[-1] == A
    # image 0: anchors of the first level (its last pixel among them), of the second and of the coarsest; image 1: no labels; image 2:
    # the first level's first pixel and the third level
    picks = [[offs[1] - 5, offs[0] + 9 * (hws[0][1] + 1) + 4, offs[1] + 4, offs[4] + 1], [], [offs[0] + 1, offs[2] + 3]]
    ann = labels_on_anchors(anc, picks, B, 5)
    need = cv.reg_need_tiles(anc_t, torch.from_numpy(ann).to(dev), True, B, hws, 9)
    torch.cuda.synchronize()
    pos = rc.positive_pixels(anc, ann, hws)
    assert all(pos[lvl][j].any() for j, lvl in ((0, 0), (0, 1), (0, 4), (2, 0), (2, 2))) and not any(p[1].any() for p in pos)
    p0 = rc.tiles_of_pixels(pos)
    F, E = rc.need_sets(p0)
    T = sum(m.size for m in p0)
    assert need.Tpad == cv.wino_tpad(T) and len(need.flags) == 6
    for k, want in enumerate(F + [E]):
        got = need.flags[k].cpu().numpy()
        w = rc.flat(want, need.Tpad)
        assert np.array_equal(got, w), "array %d: %d bytes differ" % (k, int((got != w).sum()))
        tl = need.lists[k]
        lists = sc.lists_of(w)
        assert tl.lengths() == tuple(len(x) for x in lists)
        for g, x in zip((tl.tiles, tl.units, tl.blocks), lists):
            assert np.array_equal(g.cpu().numpy()[:len(x)], x)
    if hw == (160, 224):
        assert 0 < int(F[0][0].sum()) < int(F[4][0].sum()) < F[0][0].size      # the first level: sparse at every depth


def test_need_sets_without_any_label(cv, dev):
    from retinanet_mi355x import arch, ops
    hws = arch.pyramid_shapes(40, 56)
    anc_t = ops.anchors(40, 56, dev)
    ann = torch.full((2, 3, 27), -1.0, device=dev)
    need = cv.reg_need_tiles(anc_t, ann, True, 2, hws, 9)
    torch.cuda.synchronize()
    assert all(not f.any() for f in need.flags) and all(tl.lengths() == (0, 0, 0) for tl in need.lists)


# ------------------------------------------------------------------------------------------------ 2. one tower layer
N, C = 2, 128
LEVELS = [(9, 13), (5, 7)]
SHAPES = [(N, h, w) for h, w in LEVELS]
GRIDS = [rc.grid(l) for l in LEVELS]                             # 3 x 4 and 2 x 2 tiles
T = sum(sc.tiles_of(s) for s in SHAPES)
# needed tiles (level, n, th, tw): a corner, the last (partial) tile of an image, the first tile of image 1, the second level
NEEDED = {"spread": [(0, 0, 0, 0), (0, 0, 2, 3), (0, 1, 0, 0), (0, 1, 1, 2), (1, 0, 1, 1), (1, 1, 0, 1)],
          "one": [(0, 1, 2, 1)],
          "zero": []}


def need_flags(name, Tpad):
    maps = [np.zeros((N,) + g, dtype=bool) for g in GRIDS]
    for lvl, n, th, tw in NEEDED[name]:
        maps[lvl][n, th, tw] = True
    return maps, rc.flat(maps, Tpad)


@pytest.fixture(scope="module")
def layer(dev):
    xs = [rnd(s + (C,), 700 + i).to(dev) for i, s in enumerate(SHAPES)]
    ws = {c: rnd((c, C, 3, 3), 710 + c, (2.0 / (9 * C)) ** 0.5).to(dev) for c in (128, 108)}
    bs = {c: rnd((c,), 720 + c, 0.1).to(dev) for c in (128, 108)}
    return xs, ws, bs


def run_layer(cv, dev, layer, cout, name=None, grid=0):
    xs, ws, bs = layer
    Tpad = cv.wino_tpad(T)
    U = cv.wino_weights(ws[cout], 0)
    need = None
    if name is not None:
        tl = cv.tile_lists(torch.from_numpy(need_flags(name, Tpad)[1]).to(dev), Tpad, grid=grid)
        need = tl
        cv.NEED_POISON = True                                    # outputs, kept V, sign words, the workspace's M: NaN / all-ones first
    try:
        ys, (V, _, v_am) = cv.wino_conv_group(xs, U, shift=bs[cout], act=cv.ACT_RELU, keep_v=True, sign=True, need=need)
        torch.cuda.synchronize()
    finally:
        cv.NEED_POISON = False
    out = {"y": [y.cpu().numpy() for y in ys], "V": V.view(36, Tpad, C).cpu().numpy(),
           "rows": None if v_am[0] is None else v_am[0].cpu().numpy(),
           "sign": [getattr(y, "_rn_sign", None) for y in ys]}
    out["sign"] = [None if s is None else s.cpu().numpy().reshape(y.shape[0], y.shape[1], y.shape[2], -1) for s, y in zip(out["sign"], ys)]
    return out


def check_layer(dense, got, name, Tpad):
    maps, flat = need_flags(name, Tpad)
    base = 0
    for lvl, (h, w) in enumerate(LEVELS):
        px = np.repeat(np.repeat(maps[lvl], 4, axis=1), 4, axis=2)[:, :h, :w]       # pixels of the needed tiles
        y, yd = got["y"][lvl], dense["y"][lvl]
        assert np.array_equal(y[px].view(np.uint32), yd[px].view(np.uint32)), "level %d: needed tiles differ" % lvl
        assert np.isnan(y[~px]).all(), "level %d: stored outside the need set" % lvl
        assert not np.isnan(yd).any()
        if dense["sign"][lvl] is not None:
            assert np.array_equal(got["sign"][lvl][px], dense["sign"][lvl][px])
            assert (got["sign"][lvl][~px] == -1).all()
        else:
            assert got["sign"][lvl] is None
        base += maps[lvl].size
    needed = flat != 0
    in_unit = np.repeat(needed.reshape(-1, 16).any(axis=1), 16)
    V, Vd = got["V"], dense["V"]
    assert np.array_equal(V[:, needed].view(np.uint32), Vd[:, needed].view(np.uint32))
    assert not V[:, in_unit & ~needed].view(np.uint32).any()     # zero rows: the weight gradient reads whole units
    assert np.isnan(V[:, ~in_unit]).all()
    if dense["rows"] is not None:
        assert np.array_equal(got["rows"][needed], dense["rows"][needed]) and dense["rows"][needed].all()


@pytest.mark.parametrize("cout", [128, 108])
@pytest.mark.parametrize("name,grid", [("spread", 0), ("spread", 2), ("one", 0), ("zero", 0)])
def test_one_layer_on_a_need_set(cv, dev, layer, cout, name, grid):
    """grid = 2: the GEMM's 36 items (one block x one column tile x 36 positions) on two workgroups."""
    Tpad = cv.wino_tpad(T)
    assert Tpad == 256 and T == 32
    dense = run_layer(cv, dev, layer, cout)
    got = run_layer(cv, dev, layer, cout, name, grid)
    check_layer(dense, got, name, Tpad)
    if name == "zero":                                           # nothing written at all
        assert all(np.isnan(y).all() for y in got["y"]) and np.isnan(got["V"]).all()


# ------------------------------------------------------------------------------------------------ 3. whole step
HW = (384, 512)


def _net(dev):
    from retinanet_mi355x import modules
    sd, img, _ = gc.model_inputs("resnet18", True, hw=HW)
    net = modules.resnet18(num_classes=4, directional=True)
    net.load_state_dict(sd)
    net = net.to(dev)
    net.train()
    net.freeze_bn()
    return net, img.to(dev)


def _corner_labels(net, dev, B):
    """One small box near a corner per image: the box of a first-level anchor near the top left / the bottom right."""
    from retinanet_mi355x import arch
    hws = arch.pyramid_shapes(*HW)
    anc = net._engine.anchors(HW[0], HW[1], dev).cpu().numpy().reshape(-1, 4)
    h0, w0 = hws[0]
    picks = [[9 * (2 * w0 + 3) + 4], [9 * ((h0 - 3) * w0 + w0 - 4) + 4]][:B]
    return torch.from_numpy(labels_on_anchors(anc, picks, B, 2)).to(dev)


def _step(net, img, ann):
    for p in net.parameters():
        p.grad = None
    losses = net([img, ann])
    sum(l.mean() for l in losses).backward()
    torch.cuda.synchronize()
    return ([l.detach().cpu().numpy().copy() for l in losses],
            {n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None})


def _distance(a, b):
    """The largest, over the losses and every gradient, of max|a - b| / max|b|."""
    d = 0.0
    for x, y in list(zip(a[0], b[0])) + [(a[1][n], b[1][n]) for n in b[1]]:
        d = max(d, float(np.abs(x.astype(np.float64) - y).max()) / (float(np.abs(y).max()) + 1e-300))
    return d


def _finite(r):
    return all(np.isfinite(x).all() for x in r[0]) and all(np.isfinite(g).all() for g in r[1].values())


def test_whole_step_sparse_forward(cv, dev):
    """Sparse against dense forward: no farther apart than the dense split3 and the dense native product modes, which the project already
    accepts as the same step (margin 1x: a need set can only lower an image's amax, and a finer power-of-two scale moves the split
    products towards fp64).  Then the three backward configurations on top of the sparse forward: bit-identical."""
    from retinanet_mi355x import engine
    net, img = _net(dev)
    ann = _corner_labels(net, dev, img.shape[0])
    before = engine.SPARSE_REG, engine.SPARSE_REG_LISTS, engine.SPARSE_REG_FWD
    try:
        engine.SPARSE_REG_FWD = False
        dense = _step(net, img, ann)
        cv.set_fp32_mfma("native")
        native = _step(net, img, ann)
        cv.set_fp32_mfma("split3")
        engine.SPARSE_REG_FWD = True
        cv.NEED_POISON = True
        poisoned = _step(net, img, ann)
        cv.NEED_POISON = False
        eng = net._engine
        sizes = [tl.lengths() for tl in eng._reg_need_lists]
        T_ = sum(img.shape[0] * th * tw for th, tw in (rc.grid(x) for x in eng_hws(HW)))
        on = _step(net, img, ann)
        engine.SPARSE_REG, engine.SPARSE_REG_LISTS = True, False
        early = _step(net, img, ann)
        engine.SPARSE_REG, engine.SPARSE_REG_LISTS = False, True
        off = _step(net, img, ann)
    finally:
        engine.SPARSE_REG, engine.SPARSE_REG_LISTS, engine.SPARSE_REG_FWD = before
        cv.NEED_POISON = False
        cv.set_fp32_mfma("split3")
    for k in range(6):
        assert 0 < sizes[k][0] < T_, (k, sizes[k], T_)           # void otherwise: sparse at every depth
    assert [s[0] for s in sizes[:5]] == sorted(s[0] for s in sizes[:5]) and sizes[0][0] < sizes[5][0] < sizes[1][0]
    assert _finite(dense) and _finite(native) and len(dense[1]) > 20
    assert _finite(poisoned), "a skipped byte reached a result"
    d_sparse, d_modes = _distance(poisoned, dense), _distance(native, dense)
    print("need-set sizes (tiles, units, blocks) of %d tiles: %s" % (T_, sizes))
    print("distance sparse forward - dense forward %.3e | dense native - dense split3 %.3e" % (d_sparse, d_modes))
    assert d_sparse <= d_modes, (d_sparse, d_modes)
    for got in (poisoned, early, off):                           # poison or not, sparse / early-exit / dense backward: the same bits
        for a, b in zip(got[0], on[0]):
            assert np.array_equal(a, b)
        assert set(got[1]) == set(on[1])
        for n in on[1]:
            assert np.array_equal(got[1][n], on[1][n]), n


def eng_hws(hw):
    from retinanet_mi355x import arch
    return arch.pyramid_shapes(*hw)

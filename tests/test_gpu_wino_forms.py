"""GPU: the forms of the Winograd transforms (csrc/conv_wino.hip) against each other, bit for bit, at the entry-point level.

The dense forms of both transforms are checked against fp64 elsewhere (test_gpu_wino_transforms.py); here every list / flag / fused /
offset form must give exactly what the dense form gives where it writes, and leave everything else as it was.  Shapes (the smallest at which each piece can
go wrong): two problems in one group, N=3 H=13 W=10 (4 x 3 tiles per image, ragged right and bottom edges) and N=1 H=4 W=4: T = 37 tiles,
Tpad = 256; C = 4 (one thread per tile) and 8; Cout = 32 (sign words are legal).  Flags: tiles 3 and 36, so units 0 and 2 are listed and
unit 1 holds tiles but is not.  Every output, V and Z starts as NaN, row words and sign words as all-ones (what conv.NEED_POISON does).

Both-without-flags against rn_wino_input_group: V (dy_form 0) and Z (dy_form 1) are compared bit for bit as well -- the fused kernel
runs the same bt6 / a6 on the same loaded values, and the comparison holds on the kernels as they were before they shared one body.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 13, 10), (1, 4, 4)]
T, TPAD, COUT = 37, 256, 32
ACTIVE = [3, 36]
LISTED_UNITS = [0, 2]
POISON_WORD = -1


def tile_geometry():
    """Per global tile: (problem, image, th, tw)."""
    out = []
    for p, (N, H, W) in enumerate(SHAPES):
        TH, TW = (H + 3) // 4, (W + 3) // 4
        out += [(p, n, th, tw) for n in range(N) for th in range(TH) for tw in range(TW)]
    assert len(out) == T
    return out


TILES = tile_geometry()
INACTIVE_OF_LISTED = [t for t in range(T) if t // 16 in LISTED_UNITS and t not in ACTIVE]
UNLISTED_ROWS = [r for r in range(TPAD) if r // 16 not in LISTED_UNITS or r >= T]


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def words(n, dev, fill=POISON_WORD):
    return torch.full((n,), fill, dtype=torch.int32, device=dev)


def is_poison(a):
    return np.isnan(a.view(np.float32)) if a.dtype == np.int32 else np.isnan(a)


class Env:
    def __init__(self, dev):
        from retinanet_mi355x import _hip, conv
        self.hip, self.cv, self.dev, self.lib = _hip, conv, dev, _hip.load()
        assert conv.wino_tpad(T) == TPAD
        self.flags = torch.zeros(TPAD, dtype=torch.uint8, device=dev)
        self.flags[ACTIVE] = 1
        self.lists = conv.tile_lists(self.flags, TPAD)
        assert self.lists.lengths() == (2, 2, 1)
        assert self.lists.tiles[:2].tolist() == ACTIVE and self.lists.units[:2].tolist() == LISTED_UNITS

    def inputs(self, C, seed):
        g = torch.Generator().manual_seed(seed)
        xs = [(torch.randn((N, H, W, C), generator=g) * 2.0 ** (3 * i)).to(self.dev) for i, (N, H, W) in enumerate(SHAPES)]
        return xs, [self.cv.amax_words(x) for x in xs]

    def check(self, rc, what):
        self.hip.check(rc, what)
        torch.cuda.synchronize()

    # ---- the entry points; every call returns fresh tensors that started as poison: V / Z [36, Tpad, C], row words [Tpad], tensor word
    def input(self, xs, am, C, dy_form=0, off=0, lists=False):
        V, rows, word = nan((36, TPAD, C), self.dev), words(TPAD, self.dev), words(1, self.dev, 0)
        g = self.cv._wino_group(xs, srcs=xs, amaxs=am)
        rw = None if dy_form else rows.data_ptr()
        if lists:
            self.check(self.lib.rn_wino_input_group_list(ctypes.byref(g), V.data_ptr(), C, off, TPAD, rw, word.data_ptr(), self.flags.data_ptr(),
                                                         self.lists.units.data_ptr(), self.lists.counts.data_ptr() + 4, self.hip.stream()), "input_group_list")
        else:
            self.check(self.lib.rn_wino_input_group(ctypes.byref(g), V.data_ptr(), C, off, TPAD, dy_form, rw, word.data_ptr(), self.hip.stream()), "input_group")
        return bits(V), rows.cpu().numpy(), int(word)

    def both(self, xs, am, C, form, off=0):
        V, Z, rows, word = nan((36, TPAD, C), self.dev), nan((36, TPAD, C), self.dev), words(TPAD, self.dev), words(1, self.dev, 0)
        g = self.cv._wino_group(xs, srcs=xs, amaxs=am)
        head = (ctypes.byref(g), V.data_ptr(), Z.data_ptr(), C, off, TPAD, rows.data_ptr(), word.data_ptr())
        if form == "plain":
            rc = self.lib.rn_wino_input_both_group(*head, self.hip.stream())
        elif form == "flags":
            rc = self.lib.rn_wino_input_both_group_flags(*head, self.flags.data_ptr(), self.hip.stream())
        else:
            rc = self.lib.rn_wino_input_both_group_lists(*head, self.flags.data_ptr(), self.lists.units.data_ptr(), self.lists.counts.data_ptr() + 4,
                                                         self.hip.stream())
        self.check(rc, "input_both_group " + form)
        return bits(V), bits(Z), rows.cpu().numpy(), int(word)

    def output(self, M, form="dense", off=0, shapes=SHAPES, shift=None, act=0, flags_out=False):
        """-> (ys, sign words, amax tables as uint8 [N, 256]) per problem, and flags_out or None."""
        ys = [nan((N, H, W, COUT), self.dev) for N, H, W in shapes]
        signs = [words(y.numel() // 32, self.dev) for y in ys]
        ams = [torch.zeros(y.shape[0] * self.cv.AMAX_SUB, dtype=torch.int32, device=self.dev) for y in ys]
        g = self.cv._wino_group(ys, dsts=ys, signs=signs, amaxs=ams)
        fo = torch.zeros(TPAD, dtype=torch.uint8, device=self.dev) if flags_out else None
        head = (ctypes.byref(g), M.data_ptr(), COUT, off, TPAD, None, self.hip.ptr(shift), 0, act, 0)
        if form == "dense":
            rc = self.lib.rn_wino_output_group(*head, self.hip.stream())
        elif form == "flags":
            rc = self.lib.rn_wino_output_group_flags(*head, self.flags.data_ptr(), self.hip.ptr(fo), self.hip.stream())
        else:
            rc = self.lib.rn_wino_output_group_list(*head, self.lists.tiles.data_ptr(), self.lists.counts.data_ptr(), self.hip.stream())
        self.check(rc, "output_group " + form)
        return ([bits(y) for y in ys], [s.cpu().numpy() for s in signs], [a.view(torch.uint8).view(-1, 256).cpu().numpy() for a in ams],
                None if fo is None else fo.cpu().numpy())


@pytest.fixture(scope="module")
def env(dev):
    return Env(dev)


@pytest.fixture(scope="module", params=[4, 8])
def case(request, env):
    """One set of inputs per C and the dense transforms of it, shared by the tests and left unchanged."""
    C = request.param
    xs, am = env.inputs(C, seed=C)
    dense_v = env.input(xs, am, C)
    assert not is_poison(dense_v[0][:, :T]).any() and is_poison(dense_v[0][:, T:]).all()
    assert (dense_v[1][:T] > 0).all() and (dense_v[1][T:] == POISON_WORD).all()
    return C, xs, am, dense_v


def test_list_v_against_dense_v(env, case):
    C, xs, am, (Vd, rows_d, _) = case
    Vl, rows_l, _ = env.input(xs, am, C, lists=True)
    assert np.array_equal(Vl[:, ACTIVE], Vd[:, ACTIVE])
    assert (Vl[:, INACTIVE_OF_LISTED] == 0).all()                   # +0.0: zero rows for the weight gradient's whole units
    assert is_poison(Vl[:, UNLISTED_ROWS]).all()
    assert np.array_equal(rows_l[ACTIVE], rows_d[ACTIVE])
    assert (np.delete(rows_l, ACTIVE) == POISON_WORD).all()


def test_both_with_flags_against_both_with_lists(env, case):
    C, xs, am, (Vd, rows_d, _) = case
    Vf, Zf, rows_f, word_f = env.both(xs, am, C, "flags")
    Vl, Zl, rows_l, word_l = env.both(xs, am, C, "lists")
    Zd = env.input(xs, am, C, dy_form=1)[0]
    inactive = [t for t in range(TPAD) if t not in ACTIVE]
    for V, Z in ((Vf, Zf), (Vl, Zl)):
        assert np.array_equal(V[:, ACTIVE], Vd[:, ACTIVE]) and np.array_equal(Z[:, ACTIVE], Zd[:, ACTIVE])
        assert (Z[:, INACTIVE_OF_LISTED] == 0).all()
        assert is_poison(Z[:, UNLISTED_ROWS]).all()                  # a unit without an active tile: the reduction skips it whole
        assert is_poison(V[:, inactive]).all()
    assert np.array_equal(Vf, Vl) and np.array_equal(Zf, Zl) and word_f == word_l and word_f != 0
    assert np.array_equal(rows_f[:T], rows_d[:T]) and (rows_f[T:] == POISON_WORD).all()      # the flag form visits every tile
    listed = [t for t in range(T) if t // 16 in LISTED_UNITS]
    assert np.array_equal(rows_l[listed], rows_d[listed])
    assert (np.delete(rows_l, listed) == POISON_WORD).all()          # ... the list form nothing at all of unit 1


def test_both_without_flags_against_the_two_single_transforms(env, case):
    C, xs, am, (Vd, rows_d, _) = case
    V, Z, rows, word = env.both(xs, am, C, "plain")
    Zd, _, word_d = env.input(xs, am, C, dy_form=1)
    assert np.array_equal(V, Vd) and np.array_equal(rows, rows_d)
    assert np.array_equal(Z, Zd) and word == word_d != 0


def tile_pixels(t):
    """(problem, image, rows, columns) of global tile t's stored pixels."""
    p, n, th, tw = TILES[t]
    _, H, W = SHAPES[p]
    return p, n, slice(4 * th, min(4 * th + 4, H)), slice(4 * tw, min(4 * tw + 4, W))


def amax_tables(ys, tiles):
    """What the output transform notes for `tiles`: per problem [N, 256] bytes, byte e set when a thread (a tile x 4 channels) stored
    a largest magnitude with exponent field e."""
    out = [np.zeros((N, 256), dtype=np.uint8) for N, _, _ in SHAPES]
    for t in tiles:
        p, n, hs, ws = tile_pixels(t)
        am = np.abs(ys[p].view(np.float32)[n, hs, ws]).reshape(-1, COUT // 4, 4).max(axis=(0, 2))
        out[p][n, (am.view(np.int32) >> 23) & 0xff] = 1
    return out


@pytest.fixture(scope="module")
def out_case(env):
    g = torch.Generator().manual_seed(5)
    M = torch.randn((36, TPAD, COUT), generator=g).to(env.dev)
    shift = torch.randn((COUT,), generator=g).to(env.dev)
    dense = env.output(M, shift=shift, act=1)
    for y, s in zip(dense[0], dense[1]):
        assert not is_poison(y).any() and (y == 0).any() and (y != 0).any() and (s != POISON_WORD).any()
    return M, shift, dense


def test_output_list_against_dense(env, out_case):
    M, shift, (yd, sd, ad, _) = out_case
    yl, sl, al, _ = env.output(M, "list", shift=shift, act=1)
    written = [np.zeros(y.shape[:3], dtype=bool) for y in yd]
    for t in ACTIVE:
        p, n, hs, ws = tile_pixels(t)
        written[p][n, hs, ws] = True
    for p in range(len(SHAPES)):
        assert written[p].any()
        assert np.array_equal(yl[p][written[p]], yd[p][written[p]]) and is_poison(yl[p][~written[p]]).all()
        spix, dpix = sl[p].reshape(written[p].shape), sd[p].reshape(written[p].shape)      # Cout = 32: one sign word per pixel
        assert np.array_equal(spix[written[p]], dpix[written[p]]) and (spix[~written[p]] == POISON_WORD).all()
    for got, listed, every, dense in zip(al, amax_tables(yd, ACTIVE), amax_tables(yd, range(T)), ad):
        assert np.array_equal(got, listed) and np.array_equal(dense, every)


def test_output_flags_against_dense(env, out_case):
    M, shift, (yd, sd, ad, _) = out_case
    y0, s0, _, _ = env.output(torch.zeros_like(M), shift=shift, act=1)              # the dense epilogue on M = 0
    yf, sf, af, _ = env.output(M, "flags", shift=shift, act=1)
    expect_y, expect_s = [y.copy() for y in y0], [s.copy().reshape(y.shape[:3]) for s, y in zip(s0, y0)]
    for t in ACTIVE:
        p, n, hs, ws = tile_pixels(t)
        expect_y[p][n, hs, ws] = yd[p][n, hs, ws]
        expect_s[p][n, hs, ws] = sd[p].reshape(yd[p].shape[:3])[n, hs, ws]
    for p in range(len(SHAPES)):
        assert np.array_equal(yf[p], expect_y[p]) and np.array_equal(sf[p].reshape(expect_s[p].shape), expect_s[p])
    for got, want in zip(af, amax_tables(expect_y, range(T))):
        assert np.array_equal(got, want)


def test_output_flags_out(env, out_case):
    """Without a shift a flag-0 tile stores zeros only: the stored tensor's flags are those of the pixels of tiles 3 and 36."""
    M = out_case[0]
    ys, _, _, fo = env.output(M, "flags", flags_out=True)
    want, dilated = np.zeros(TPAD, dtype=np.uint8), np.zeros(TPAD, dtype=np.uint8)
    for t, (p, n, th, tw) in enumerate(TILES):
        _, H, W = SHAPES[p]
        nz = (ys[p].view(np.float32)[n] != 0).any(axis=2)
        patch = nz[max(4 * th - 1, 0):4 * th + 5, max(4 * tw - 1, 0):4 * tw + 5]    # the 6x6 patch of the next layer's input transform
        want[t] = patch.any()
        stores = [nz[4 * a:4 * a + 4, 4 * b:4 * b + 4].any() for a in range(th - 1, th + 2) for b in range(tw - 1, tw + 2)
                  if 0 <= a < (H + 3) // 4 and 0 <= b < (W + 3) // 4]
        dilated[t] = any(stores)                                                      # the 3x3 dilation of "tile stores a non-zero", clipped
    assert np.array_equal(fo, want) and np.array_equal(want, dilated)
    assert np.flatnonzero(want).tolist() == [0, 1, 3, 4, 6, 7, 36]


def test_tile_offset(env, case, out_case):
    """The second problem alone, at the offset it has in the group: the same rows as the group's call, and nothing else."""
    C, xs, am, (Vd, rows_d, _) = case
    last, rest = [T - 1], [r for r in range(TPAD) if r != T - 1]
    V, rows, _ = env.input(xs[1:], am[1:], C, off=T - 1)
    assert np.array_equal(V[:, last], Vd[:, last]) and is_poison(V[:, rest]).all()
    assert rows[T - 1] == rows_d[T - 1] and (np.delete(rows, last) == POISON_WORD).all()
    V0 = env.input(xs[1:], am[1:], C)[0]
    assert np.array_equal(V0[:, [0]], Vd[:, last])                  # ... and at offset 0: the same row, shifted
    Vl, rows_l, _ = env.input(xs[1:], am[1:], C, off=T - 1, lists=True)
    assert np.array_equal(Vl[:, last], Vd[:, last]) and is_poison(Vl[:, rest]).all() and rows_l[T - 1] == rows_d[T - 1]
    Zd = env.input(xs, am, C, dy_form=1)[0]
    for form in ("plain", "flags", "lists"):
        Vb, Zb, rows_b, _ = env.both(xs[1:], am[1:], C, form, off=T - 1)
        assert np.array_equal(Vb[:, last], Vd[:, last]) and np.array_equal(Zb[:, last], Zd[:, last]), form
        assert is_poison(Vb[:, rest]).all() and is_poison(Zb[:, rest]).all() and rows_b[T - 1] == rows_d[T - 1], form
    M, shift, (yd, sd, ad, _) = out_case
    for form in ("dense", "flags", "list"):
        ys, ss, aa, _ = env.output(M, form, off=T - 1, shapes=SHAPES[1:], shift=shift, act=1)
        assert np.array_equal(ys[0], yd[1]) and np.array_equal(ss[0], sd[1]) and np.array_equal(aa[0], ad[1]), form

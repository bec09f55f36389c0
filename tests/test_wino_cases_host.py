"""CPU: the references, bounds and cases of tests/wino_cases.py.  The references are proved by composition against torch's float64
convolution, the epilogue against plain torch expressions; the bounds hold a float32 evaluation of the same matrix products in two
association orders (not too tight), and every comparison rejects each of a list of deliberately wrong float64 references (not vacuous)."""
import numpy as np
import pytest
import torch

import wino_cases as wc

RAGGED = [(2, 9, 6), (1, 5, 11)]              # two small problems, ragged on both edges
TOL = 1e-12


def close(got, want):
    return float(np.abs(got - want).max()) <= TOL * float(np.abs(want).max())


@pytest.mark.parametrize("shape", RAGGED)
def test_references_compose_to_the_convolution(shape):
    N, H, W = shape
    C, K = 5, 3
    rng = np.random.default_rng(7)
    x, g, dy = rng.standard_normal((N, H, W, C)), rng.standard_normal((K, C, 3, 3)), rng.standard_normal((N, H, W, K))
    tx = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    tg = torch.from_numpy(g).requires_grad_(True)
    ty = torch.nn.functional.conv2d(tx, tg, padding=1)
    ty.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    V = wc.ref_v(x)
    Uw = np.einsum("ir,kcrs,js->ijck", wc.G, g, wc.G).reshape(36, C, K)
    y = wc.ref_y(np.einsum("ptc,pck->ptk", V, Uw), shape)
    assert close(y, ty.detach().permute(0, 2, 3, 1).numpy())
    Z = wc.ref_z(dy)
    dU = np.einsum("ptk,ptc->pkc", Z, V).reshape(6, 6, K, C)
    assert close(np.einsum("ir,ijkc,js->kcrs", wc.G, dU, wc.G), tg.grad.numpy())
    assert close(Z[6 * 1 + 1].sum(axis=0), dy.sum(axis=(0, 1, 2)))
    # ... and the epilogue's pieces on top of it: the data gradient's form, dx = mask * conv + addend
    add, mask = rng.standard_normal(y.shape), rng.standard_normal(y.shape)
    r, _ = wc.ref_epilogue(y, np.abs(y), 0, on=mask > 0, mask_mode=1, add=add)
    assert close(r, (ty.detach().permute(0, 2, 3, 1) * (torch.from_numpy(mask) > 0) + torch.from_numpy(add)).numpy())


def test_matrices_are_lavin_and_grays():
    """A^T [(G g) .* (B^T d)] = the 1-D correlation F(4, 3), for unit vectors: every entry of the three matrices takes part."""
    for a in range(6):
        for b in range(3):
            d, g = np.eye(6)[a], np.eye(3)[b]
            want = np.array([d[i:i + 3] @ g for i in range(4)])
            assert np.abs(wc.AT @ ((wc.G @ g) * (wc.BT @ d)) - want).max() < 1e-15


def torch_epilogue(v, e, scale, shift, on, add):
    t = torch.from_numpy(np.array(v))
    if scale is not None:
        t = t * torch.from_numpy(scale)
    if shift is not None:
        t = t + torch.from_numpy(shift)
    if e.mask_mode == 1:
        t = torch.where(torch.from_numpy(on), t, torch.zeros_like(t))
    if add is not None:
        t = t + torch.from_numpy(add)
    t = torch.relu(t) if e.act == 1 else (torch.sigmoid(t) if e.act == 2 else t)
    if e.mask_mode == 2:
        t = torch.where(torch.from_numpy(on), t, torch.zeros_like(t))
    return t.numpy()


@pytest.mark.parametrize("name,shapes,cout", wc.OUT_CASES)
def test_epilogue_reference_against_torch(name, shapes, cout):
    e = wc.EPILOGUES[name]
    for exact in ([False] if e.real_only else [True, False]):
        shapes, ops, want = wc.out_case(name, cout, exact)
        f64 = lambda a: None if a is None else a.astype(np.float64)
        for p, shape in enumerate(shapes):
            on = None
            if e.mask_mode:
                on = torch.from_numpy(np.nan_to_num(ops.masks[p].astype(np.float64), nan=-1.0)).gt(0).numpy()       # a NaN mask is off
                if e.bits:
                    words = ops.bits[p]
                    assert words.size * 32 == on.size
                    unpacked = np.array([(int(words[i >> 5]) >> (i & 31)) & 1 for i in range(0, on.size, 7)], dtype=bool)
                    assert np.array_equal(unpacked, on.reshape(-1)[::7])
            got = torch_epilogue(wc.ref_y(ops.M[p], shape), e, f64(ops.scale), f64(ops.shift), on, f64(ops.adds[p]))
            assert got.shape == shape + (cout,)
            assert float(np.abs(got - want[p][0]).max()) <= TOL * max(1.0, float(np.abs(want[p][0]).max())), (name, p)
            if e.mask_mode == 2:
                assert (want[p][1][~on] == 0).all() and (want[p][0][~on] == 0).all()
            assert (want[p][1] >= 0).all() and np.isfinite(want[p][1]).all()


def test_exactness_conditions():
    """Every intermediate of the EXACT set is a multiple of 1/2 below 2^23 (wc.check_exact, inside in_case / out_case); the sizes seen."""
    biggest = 0.0
    for name, shapes, C in wc.IN_CASES:
        _, xs, want = wc.in_case(name, C, True)
        for k in ("v", "z"):
            assert np.array_equal(want[k][0], np.round(want[k][0]))
        biggest = max(biggest, float(np.abs(want["v"][0]).max()))
        assert max(np.abs(x).max() for x in xs) == 8 and all(np.array_equal(x, np.round(x)) for x in xs)
    assert 100 < biggest <= 100 * 8                                  # |B^T d B| <= 100 max|d|
    for name, shapes, cout in wc.OUT_CASES:
        if not wc.EPILOGUES[name].real_only:
            _, ops, want = wc.out_case(name, cout, True)
            for r, _ in want:
                assert np.array_equal(2 * r, np.round(2 * r)) and np.abs(r).max() < 2.0 ** 23


def test_modes_1_and_2_differ_where_there_is_a_mask_and_an_addend():
    seen = 0
    for name, shapes, cout in wc.OUT_CASES:
        e = wc.EPILOGUES[name]
        if e.mask_mode and e.add:
            for exact in (True, False):
                _, ops, want = wc.out_case(name, cout, exact)
                for p in e.add:
                    if p < len(shapes):
                        off = ~wc.mask_on(ops.masks[p], None)
                        assert (off & (ops.adds[p] != 0)).any()
                        swapped = wc.expect_out(name, shapes, ops, p, modes_swapped=True)[0]
                        assert not wc.same_values(swapped, want[p][0])
                        seen += 1
    assert seen >= 2 * (5 + 3 + 5 + 1)


def test_case_geometry():
    """What the issue says each case exercises."""
    assert [wc.n_tiles(s) for s in wc.G5] == [12, 1, 3, 3, 8]
    threads = 40 * (260 // 4)
    assert threads == 2600 and -(-threads // 256) == 11 and 11 * 256 - threads == 216 and (11 >> 3, 11 & 7) == (1, 3)
    assert 256 % (12 // 4) != 0 and 256 % (260 // 4) != 0
    A, rows = wc.head_layout(wc.G5_HEAD, 12)
    assert rows == [3, 58, 75, 77, 100] and A == 142 and (A * 12) % 4 == 0
    t = wc.in_tables(wc.G5)
    assert [None if x is None else [wc.table_exp(i) for i in x] for x in t] == [[130, 0], [250], [1, 127, 200], None, [90, 140]]
    assert wc.word(250, 7) == wc.word(250, 8) == wc.word(254, 0) == 0x7f7fffff and wc.word(0, 7) == 0 and wc.word(1, 7) == (8 << 23) | 0x7fffff
    assert wc.tensor_word(t, 7) == 0x7f7fffff and wc.tensor_word(t, 7, start=0x7f800000) == 0x7f800000
    w = wc.in_tables(wc.WIDE)
    assert wc.tensor_word(w, 7) == (138 << 23) | 0x7fffff and wc.tensor_word(w, 8) == (139 << 23) | 0x7fffff
    rw = wc.row_words(wc.G5, t)
    assert rw.shape == (27,) and rw[0] == wc.word(130, 7) and (rw[6:12] == 0).all() and rw[12] == 0x7f7fffff and (rw[16:19] == 0).all()


# ---------------------------------------------------------------------------------------------- the bounds are not too tight
@pytest.mark.parametrize("name,shapes,C", wc.IN_CASES)
def test_float32_input_transforms_stay_inside_the_bound(name, shapes, C):
    _, xs, want = wc.in_case(name, C, False)
    for order in (0, 1):
        v = wc.concat([wc.f32_transform(wc.BT, wc.patches(x, -1, 6).astype(np.float32), (3, 4), order).transpose(3, 4, 0, 1, 2, 5)
                       .reshape(36, -1, C) for x in xs])
        z = wc.concat([wc.f32_transform(wc.AT.T, wc.patches(x, 0, 4).astype(np.float32), (3, 4), order).transpose(3, 4, 0, 1, 2, 5)
                       .reshape(36, -1, C) for x in xs])
        assert v.dtype == z.dtype == np.float32
        fv, fz = wc.worst(v, *want["v"]), wc.worst(z, *want["z"])
        assert 0.0 < fv <= 1.0 and 0.0 < fz <= 1.0, (order, fv, fz)


@pytest.mark.parametrize("name,shapes,cout", wc.OUT_CASES)
def test_float32_output_transform_stays_inside_the_bound(name, shapes, cout):
    e = wc.EPILOGUES[name]
    shapes, ops, want = wc.out_case(name, cout, False)
    for order in (0, 1):
        for p, (N, H, W) in enumerate(shapes):
            TH, TW = (H + 3) // 4, (W + 3) // 4
            m = ops.M[p].reshape(6, 6, N, TH, TW, cout)
            u = wc.f32_transform(wc.AT, m, (0, 1), order).transpose(2, 3, 0, 4, 1, 5).reshape(N, 4 * TH, 4 * TW, cout)[:, :H, :W]
            assert u.dtype == np.float32
            if ops.scale is not None:
                u = u * ops.scale
            if ops.shift is not None:
                u = u + ops.shift
            on = None if not e.mask_mode else wc.mask_on(ops.masks[p], None)
            if e.mask_mode == 1:
                u = np.where(on, u, np.float32(0))
            if ops.adds[p] is not None:
                u = u + ops.adds[p]
            if e.act == 1:
                u = np.maximum(u, np.float32(0))
            elif e.act == 2:
                with np.errstate(over="ignore"):
                    u = np.float32(1) / (np.float32(1) + np.exp(-u))
            if e.mask_mode == 2:
                u = np.where(on, u, np.float32(0))
            assert u.dtype == np.float32
            f = wc.worst(u, *want[p])
            assert f <= 1.0, (order, p, f)


# ---------------------------------------------------------------------------------------------- ... and not vacuous
def rejected(wrong, exact):
    """A wrong reference (a function of `exact` -> (wrong values, right values, bound)) fails the comparison of that operand set."""
    got, ref, bound = wrong(exact)
    return not (wc.same_values(got, ref) if exact else wc.within(got, ref, bound))


def wrong_v(name, C, **how):
    def f(exact):
        _, xs, want = wc.in_case(name, C, exact)
        return (wc.expect_in(xs, "v", **how)[0],) + want["v"]
    return f


def wrong_z(name, C, **how):
    def f(exact):
        _, xs, want = wc.in_case(name, C, exact)
        return (wc.expect_in(xs, "z", **how)[0],) + want["z"]
    return f


def wrong_out(name, cout, p, **how):
    def f(exact):
        shapes, ops, want = wc.out_case(name, cout, exact)
        return (wc.expect_out(name, shapes, ops, p, **how)[0],) + want[p]
    return f


def wrong_head(exact):
    shapes, ops, want = wc.out_case("head", 12, False)
    ys, bounds = [r for r, _ in want], [b for _, b in want]
    nan0 = lambda a: np.nan_to_num(a, nan=0.0)              # (outside the slices the buffers are compared as poison: here as an error)
    right, wrong = wc.head_buffer(shapes, 12, ys), wc.head_buffer(shapes, 12, ys, stride_ignored=True)
    assert np.isnan(right).any() and not np.array_equal(np.isnan(right), np.isnan(wrong))
    return nan0(wrong), nan0(right), nan0(wc.head_buffer(shapes, 12, bounds))


BT_4_FOR_5 = np.where(wc.BT == -5, -4.0, wc.BT)
WRONG = {
    "halo pixel from the wrapped neighbouring row": wrong_v("G5", 4, wrap=True),
    "positions 6i+j and 6j+i swapped": wrong_v("G5", 12, swap=True),
    "positions swapped, Z": lambda exact: (wc.in_case("wide", 260, exact)[2]["z"][0].reshape(6, 6, 40, 260).swapaxes(0, 1).reshape(36, 40, 260),)
    + wc.in_case("wide", 260, exact)[2]["z"],
    "coefficient 5 replaced by 4 in B^T": wrong_v("single", 12, bt=BT_4_FOR_5),
    "patch corner at 4th instead of 4th-1": wrong_v("wide", 260, corner=0),
    "mask modes 1 and 2 swapped": wrong_out("dgrad1", 32, 2, modes_swapped=True),
    "mask modes 2 and 1 swapped": wrong_out("dgrad2-mixed", 32, 3, modes_swapped=True),
    "clamped edge pixel's addend at a valid pixel of a ragged tile": wrong_out("dgrad1", 32, 0, edge_addend=True),
    "clamped edge pixel's addend, bits form": wrong_out("bits1-add", 64, 3, edge_addend=True),
    "mask bit shift from off & 24": wrong_out("bits1-add", 64, 0, shift_mask=27),
    "mask bit shift from off & 24, mode 2": wrong_out("bits2", 64, 4, shift_mask=27),
    "second problem's tiles start one row early": wrong_v("G5", 64, second_early=True),
    "second problem's tiles start one row early, Z": wrong_z("G5", 4, second_early=True),
}


@pytest.mark.parametrize("what", sorted(WRONG))
def test_wrong_references_are_rejected(what):
    assert BT_4_FOR_5.tolist() != wc.BT.tolist()
    assert rejected(WRONG[what], True), "exact comparison accepts: " + what
    assert rejected(WRONG[what], False), "bounded comparison accepts: " + what


def test_ignored_batch_stride_is_rejected():
    """`head` has real operands only: the bounded comparison over the whole shared buffer."""
    assert rejected(wrong_head, False)


def test_wrong_words_are_rejected():
    """Gain 7 for the Z tensor word shows on `wide` and `single` (on G5 both gains clamp at 254: that case holds the clamp)."""
    w = wc.in_tables(wc.WIDE)
    assert wc.tensor_word(w, wc.GAIN_BT) != wc.tensor_word(w, wc.GAIN_A)
    g = wc.in_tables(wc.G5)
    assert wc.tensor_word(g, wc.GAIN_BT) == wc.tensor_word(g, wc.GAIN_A) == 0x7f7fffff
    rows = wc.row_words(wc.G5, g)
    assert not np.array_equal(rows, wc.row_words(wc.G5, g, wc.GAIN_A))
    lowest = [None if t is None else wc.make_table(*[[int(np.flatnonzero(i)[0])] if i.any() else [] for i in t]) for t in g]
    assert not np.array_equal(rows, wc.row_words(wc.G5, lowest))                # a lower byte taken for the highest
    assert not np.array_equal(rows, wc.row_words(wc.G5, [g[0], g[1], g[2], g[2][:1], g[4]]))      # the NULL problem given a neighbour's table


def test_sign_words_and_tables_follow_the_stored_values():
    y = np.zeros((1, 5, 6, 32), dtype=np.float32)
    y[0, 0, 0, 0], y[0, 4, 5, 31], y[0, 1, 1, 5] = 3.0, 2.0 ** -126, -1.0
    s = wc.sign_words(y)
    assert s.shape == (30,) and s[0] == 1 and s[29] == 1 << 31 and s[1:29].sum() == 0
    t = wc.out_tables(y)
    assert np.flatnonzero(t[0]).tolist() == [0, 1, 127, 128]        # threads that store zeros only set byte 0
    assert not wc.mask_on(np.array([np.nan, 0.0, -0.0, -1.0], dtype=np.float32), None).any()

"""GPU: the dense forms of the Winograd transforms, wino_in_kernel and wino_out_kernel of csrc/conv_wino.hip, per element against the
float64 references and bounds of tests/wino_cases.py (proved on the CPU by tests/test_wino_cases_host.py).  The flag, list, fused-with-flags
and offset forms are held against these dense forms, bit for bit, by tests/test_gpu_wino_forms.py.

Every entry point is called through the C ABI with a hand-filled rn_wino_group, so that the test owns every buffer.  V, Z and y start as
NaN, sign words and row words as all-ones, the result's amax tables as zero; every output has 64 guard bytes behind it; every input (the
sources, M, scale, shift, masks, mask words, addends, the sources' amax tables) sits between two bands of all-ones bytes (NaN as floats,
exponent 255 as table bytes) and must come back unchanged; the rows of M outside [tile_offset, tile_offset + T) hold NaN.  "Wrote what it
owns and nothing else" is part of each comparison.  EXACT operands must give the reference as numbers on every element, REAL operands must
lie within the bound; row words, tensor words, sign words and amax tables are compared exactly.  The largest error seen per kernel and
case family, as a fraction of its bound, is printed when the module finishes (run with -s): information, not a threshold.

Instance -> the case that runs it:
  wino_in_kernel<V>                  G5 (C = 4, 12, 64), wide, single (rn_wino_input_group dy_form 0, rn_wino_input)
  wino_in_kernel<Z>                  the same (dy_form 1, rn_wino_dy)
  wino_in_kernel<VZ>                 the same (rn_wino_input_both_group)
  wino_out_kernel<false, false>      plain, fwd, head, dgrad2-mixed, wide
  wino_out_kernel<false, true>       dgrad1, single (rn_wino_output)
  wino_out_kernel<true, true>        bits1-add
  wino_out_kernel<true, false>       bits2"""
import ctypes

import numpy as np
import pytest
import torch

import wino_cases as wc

pytestmark = pytest.mark.gpu

GUARD = 64                                # bytes behind every output that must keep their poison
BAND = 256                                # bytes of all-ones in front of and behind every input
ONES = 0xFFFFFFFF
WORST = {}                                # family -> largest error seen, as a fraction of its bound


class Env:
    def __init__(self, dev):
        from retinanet_mi355x import _hip
        self.hip, self.dev, self.lib = _hip, dev, _hip.load()
        assert _hip.RN_MAX_GROUP == wc.RN_MAX_GROUP

    def call(self, name, *args):
        self.hip.check(getattr(self.lib, name)(*args, self.hip.stream()), name)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def env(dev):
    yield Env(dev)
    print("\n" + "\n".join("wino %-34s worst error %.3f of its bound" % (k, v) for k, v in sorted(WORST.items())))


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """A kernel fault poisons the context: end the session there, start nothing more on the device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping: %s" % e, returncode=3)


def compare(family, exact, got, ref, bound):
    """EXACT: equal as numbers on every element; REAL: within the bound, with the fraction noted for the module's report."""
    if exact:
        bad = np.argwhere(~(got == ref))
        assert bad.size == 0, "%s: %d elements differ, the first at %s: %r for %r" % (family, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
        return
    w = wc.worst(got, ref, bound)
    WORST[family] = max(WORST.get(family, 0.0), w)
    assert w <= 1.0, "%s: error %.3f of its bound" % (family, w)


class Out:
    """An output buffer of `nbytes` bytes filled with `fill` (255: NaN as fp32, all-ones words), with GUARD all-ones bytes behind it."""

    def __init__(self, nbytes, dev, fill=255):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + GUARD,), 255, dtype=torch.uint8, device=dev)
        self.buf[:self.n] = fill

    def ptr(self, byte_offset=0):
        assert 0 <= byte_offset < self.n
        return self.buf.data_ptr() + byte_offset

    def get(self, dtype, shape=None):
        """The owned bytes as `dtype`; the guard must be untouched."""
        raw = self.buf.cpu().numpy()
        assert (raw[self.n:] == 255).all(), "the bytes behind the output were written"
        a = raw[:self.n].view(dtype)
        return a if shape is None else a.reshape(shape)


class In:
    """An input between two bands of all-ones bytes; unchanged() after the call."""

    def __init__(self, a, dev):
        self.raw = np.concatenate([np.full(BAND, 255, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.full(BAND, 255, np.uint8)])
        self.buf = torch.from_numpy(self.raw).to(dev)

    def ptr(self):
        return self.buf.data_ptr() + BAND

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.raw)


def ptr_of(x):
    return None if x is None else x.ptr()


def group(shapes, **pointers):
    """A hand-filled rn_wino_group: per field a list of addresses (or None) per problem."""
    from retinanet_mi355x import _hip
    g = _hip.WinoGroup()
    g.n = len(shapes)
    for i, (N, H, W) in enumerate(shapes):
        g.N[i], g.H[i], g.W[i] = N, H, W
        for field in ("src", "dst", "add", "mask", "sign", "amax"):
            getattr(g, field)[i] = pointers[field][i] if field in pointers else None
    return g


def is_ones(a):
    return np.ascontiguousarray(a).view(np.uint32) == ONES


# ---------------------------------------------------------------------------------------------- input side
def run_input(env, kind, shapes, srcs, tables, C, tpad, off, rows, start):
    """One call of rn_wino_input_group (kind "v" / "z") or rn_wino_input_both_group ("both") -> {"v": V, "z": Z, "rows": row words or None,
    "word": tensor word or None}.  rows: ask for row words; start: None (no tensor word) or what the word holds before the call."""
    n = 36 * tpad * C * 4
    outs = {k: Out(n, env.dev) for k in (("v", "z") if kind == "both" else (kind,))}
    row_out = Out(tpad * 4, env.dev) if rows else None
    word_out = None
    if start is not None:
        word_out = Out(4, env.dev)
        word_out.buf[:4] = torch.from_numpy(np.array([start], dtype=np.uint32).view(np.uint8)).to(env.dev)
    g = group(shapes, src=[s.ptr() for s in srcs], amax=[ptr_of(t) for t in tables])
    if kind == "both":
        env.call("rn_wino_input_both_group", ctypes.byref(g), outs["v"].ptr(), outs["z"].ptr(), C, off, tpad, ptr_of(row_out), ptr_of(word_out))
    else:
        env.call("rn_wino_input_group", ctypes.byref(g), outs[kind].ptr(), C, off, tpad, int(kind == "z"), ptr_of(row_out), ptr_of(word_out))
    res = {k: o.get(np.float32, (36, tpad, C)) for k, o in outs.items()}
    res["rows"] = None if row_out is None else row_out.get(np.uint32)
    res["word"] = None if word_out is None else int(word_out.get(np.uint32)[0])
    return res


def check_rows(family, exact, got, want, T, off):
    """Rows [off, off + T) against the reference; every other row keeps its poison."""
    ref, bound = want
    own = np.zeros(got.shape[1], dtype=bool)
    own[off:off + T] = True
    assert is_ones(got[:, ~own]).all(), family + ": a row outside the call's tiles was written"
    compare(family, exact, got[:, own], ref, bound)


@pytest.mark.parametrize("tpad,off", wc.PLACEMENTS)
@pytest.mark.parametrize("name,shapes,C", wc.IN_CASES)
def test_input_transforms(env, name, shapes, C, tpad, off):
    T = wc.tile_ends(shapes)[-1]
    tabs = wc.in_tables(shapes)
    tables = [None if t is None else In(t, env.dev) for t in tabs]
    none = [None] * len(shapes)
    for exact in (True, False):
        _, xs, want = wc.in_case(name, C, exact)
        srcs = [In(x, env.dev) for x in xs]
        for kind in ("v", "z", "both"):
            fam = "in %s %s C=%d" % (kind, name, C)
            gain = wc.GAIN_BT if kind == "v" else wc.GAIN_A
            expected_word = wc.tensor_word(tabs, gain)
            assert 0 < expected_word < ONES
            # (with tables?, row words?, the tensor word's start)
            for with_tables, rows, start in ((False, False, None), (True, kind != "z", 0), (True, kind != "z", expected_word + 1),
                                             (False, kind != "z", 5)):
                res = run_input(env, kind, shapes, srcs, tables if with_tables else none, C, tpad, off, rows, start)
                for k in (("v", "z") if kind == "both" else (kind,)):
                    check_rows(fam + ("/" + k if kind == "both" else ""), exact, res[k], want[k], T, off)
                if rows:
                    own = np.zeros(tpad, dtype=bool)
                    own[off:off + T] = True
                    assert (res["rows"][~own] == ONES).all(), fam + ": a row word outside the call's tiles was written"
                    want_rows = wc.row_words(shapes, tabs if with_tables else none)
                    assert np.array_equal(res["rows"][own], want_rows), (fam, res["rows"][own], want_rows)
                if start is not None:
                    assert res["word"] == wc.tensor_word(tabs if with_tables else none, gain, start), (fam, hex(res["word"]), start)
        assert all(s.unchanged() for s in srcs)
    assert all(t is None or t.unchanged() for t in tables)


def test_single_problem_input_entry_points(env):
    """rn_wino_input and rn_wino_dy give what the group call gives for the one problem, bit for bit, and so the reference."""
    (name, shapes, C), (tpad, off) = wc.IN_CASES[-1], wc.PLACEMENTS[1]
    assert name == "single"
    N, H, W = shapes[0]
    for exact in (True, False):
        _, xs, want = wc.in_case(name, C, exact)
        src = In(xs[0], env.dev)
        for kind, entry in (("v", "rn_wino_input"), ("z", "rn_wino_dy")):
            out = Out(36 * tpad * C * 4, env.dev)
            env.call(entry, src.ptr(), out.ptr(), N, H, W, C, off, tpad)
            got = out.get(np.float32, (36, tpad, C))
            check_rows("in %s single C=%d" % (kind, C), exact, got, want[kind], wc.n_tiles(shapes[0]), off)
            grouped = run_input(env, kind, shapes, [src], [None], C, tpad, off, False, None)[kind]
            assert np.array_equal(got.view(np.uint32), grouped.view(np.uint32))
        assert src.unchanged()


# ---------------------------------------------------------------------------------------------- output side
def run_output(env, name, shapes, cout, ops, tpad, off, single=False):
    """One call of rn_wino_output_group (single: rn_wino_output) -> per problem y [N, H, W, cout], sign words or None, amax tables uint8
    [N + 1, 256] or None; for `head` the whole shared buffer as well."""
    e = wc.EPILOGUES[name]
    T = wc.tile_ends(shapes)[-1]
    M = np.full((36, tpad, cout), np.nan, dtype=np.float32)
    M[:, off:off + T] = np.concatenate(ops.M, axis=1)
    assert np.isnan(M[:, :off]).all() and np.isnan(M[:, off + T:]).all() and off + T < tpad
    dev = env.dev
    Md = In(M, dev)
    scale, shift = (None if a is None else In(a, dev) for a in (ops.scale, ops.shift))
    masks = [None if m is None else In(b if e.bits else m, dev) for m, b in zip(ops.masks, ops.bits)]
    adds = [None if a is None else In(a, dev) for a in ops.adds]
    numel = [N * H * W * cout for N, H, W in shapes]
    y_bs, whole = 0, None
    if e.head:
        A, first = wc.head_layout(shapes, cout)
        whole, y_bs = Out(shapes[0][0] * A * cout * 4, dev), A * cout
        dst = [whole.ptr(r * cout * 4) for r in first]
    else:
        ys = [Out(n * 4, dev) for n in numel]
        dst = [y.ptr() for y in ys]
    signs = [Out(n // 32 * 4, dev) if e.signs else None for n in numel]
    amaxs = [Out((N + 1) * 256, dev, fill=0) if e.amax else None for N, _, _ in shapes]          # one more image than the call owns
    mode = e.mask_mode | (wc.MASK_BITS if e.bits else 0)
    if single:
        (N, H, W), = shapes
        assert not e.signs and not e.amax
        env.call("rn_wino_output", Md.ptr(), dst[0], N, H, W, cout, off, tpad, ptr_of(scale), ptr_of(shift), ptr_of(adds[0]), ptr_of(masks[0]),
                 mode, e.act, y_bs)
    else:
        g = group(shapes, dst=dst, add=[ptr_of(a) for a in adds], mask=[ptr_of(m) for m in masks], sign=[ptr_of(s) for s in signs],
                  amax=[ptr_of(a) for a in amaxs])
        env.call("rn_wino_output_group", ctypes.byref(g), Md.ptr(), cout, off, tpad, ptr_of(scale), ptr_of(shift), mode, e.act, y_bs)
    assert all(i is None or i.unchanged() for i in [Md, scale, shift] + masks + adds)
    buf = None
    if e.head:
        buf = whole.get(np.float32, (shapes[0][0], A, cout))
        got = [buf[:, r:r + H * W].reshape(N, H, W, cout) for (N, H, W), r in zip(shapes, first)]
    else:
        got = [y.get(np.float32, s + (cout,)) for y, s in zip(ys, shapes)]
    return (got, [None if s is None else s.get(np.uint32) for s in signs],
            [None if a is None else a.get(np.uint8, (-1, 256)) for a in amaxs], buf)


@pytest.mark.parametrize("tpad,off", wc.PLACEMENTS)
@pytest.mark.parametrize("name,shapes,cout", wc.OUT_CASES)
def test_output_transform(env, name, shapes, cout, tpad, off):
    e = wc.EPILOGUES[name]
    fam = "out %s Cout=%d" % (name, cout)
    for exact in ([False] if e.real_only else [True, False]):
        _, ops, want = wc.out_case(name, cout, exact)
        got, signs, tables, buf = run_output(env, name, shapes, cout, ops, tpad, off)
        for p, (N, H, W) in enumerate(shapes):
            assert np.isfinite(got[p]).all(), "%s: problem %d holds a NaN (poison, or a foreign row of M)" % (fam, p)
            compare(fam, exact, got[p], *want[p])
            if e.signs:
                assert np.array_equal(signs[p], wc.sign_words(got[p])), (fam, p)
                if exact:
                    assert np.array_equal(signs[p], wc.sign_words(want[p][0])), (fam, p)
                assert (signs[p] != ONES).any() and signs[p].any()
            if e.amax:
                assert np.array_equal(tables[p][:N], wc.out_tables(got[p])), (fam, p)
                if exact:
                    assert np.array_equal(tables[p][:N], wc.out_tables(want[p][0])), (fam, p)
                assert not tables[p][N].any(), "%s: the table of an image the call does not own was written" % fam
        if e.head:
            ref = wc.head_buffer(shapes, cout, [r for r, _ in want])
            outside = np.isnan(ref)
            assert outside.any() and is_ones(buf[outside]).all(), fam + ": an element outside the five slices was written"
            compare(fam, exact, buf[~outside], ref[~outside], wc.head_buffer(shapes, cout, [b for _, b in want])[~outside])
        if name == "single":
            alone = run_output(env, name, shapes, cout, ops, tpad, off, single=True)[0][0]
            assert np.array_equal(alone.view(np.uint32), got[0].view(np.uint32))

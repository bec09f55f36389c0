"""The fp32 forward / data-gradient convolutions on every path their launchers can choose -- csrc/conv_igemm.hip, conv_igemm_split.hip,
conv_igemm_mf16.hip and conv_igemm_splitk.hip behind rn_conv_igemm, rn_conv_igemm_splitk and rn_conv_igemm_grouped -- against the float64
reference of tests/igemm_cases.py (proved on the CPU by tests/test_igemm_cases_host.py).

Every run first asserts the plan: the launch goes through conv.conv_igemm / fprop / dgrad / dgrad_s2_classes / conv_igemm_grouped with
`plans=`, which reports rn_conv_igemm_plan's answer for the very descriptor it launches (a hand-filled ConvDesc through ctypes where the
wrappers cannot set a field: x_batch_stride, sign bits through an output map, no y_amax), and that answer must be the path the case names
for the configuration (product mode x conv.PRESPLIT x RN_OPT_SPLITK / MF16 / MF16_MIN).  A threshold that moves fails here instead of
moving the case onto another kernel.

Then each case runs twice.  EXACT operands (small integers): the result must be bit-equal to the reference on every element the launch
owns, in every product mode -- one dropped, doubled or misplaced product is a whole unit.  REAL operands: max |error| <= 1e-5 of the
reference's maximum on the 16x16x32 kernels (test_gpu_conv_mf16.py's bound), 1e-4 elsewhere (test_gpu_conv.py's).  Inputs sit inside NaN
bands with NaN between the images where x_batch_stride exceeds the image; outputs start as all-ones bytes (NaN) with 64 guard bytes
behind: every element of a strided, mapped or sliced output the launch does not own keeps its poison, every owned one is written, the
guards stay.  Split-K launches run twice and must agree bit for bit.  The largest real-operand error per plan, as a fraction of the
reference's maximum, is printed when the module ends (-s shows it): information, not a threshold."""
import ctypes

import numpy as np
import pytest
import torch

import igemm_cases as ic
from test_gpu_glue import stop_at_a_device_error  # noqa: F401  (autouse: a device error ends the session)

pytestmark = pytest.mark.gpu

GUARD_BYTES = 64
WORST = {}
_REF = {}


@pytest.fixture(scope="module")
def conv(dev):
    from retinanet_mi355x import conv
    assert conv.BITMASKS
    yield conv
    print("\n" + "\n".join("igemm %-48s worst real-operand error %.3g of max |ref| (bound %.0e)" % (k, v, tol_of(k))
                           for k, v in sorted(WORST.items())))
    _REF.clear()


@pytest.fixture
def config(conv):
    state = []

    def use(name):
        state.append(ic.apply_config(conv, name))
    yield use
    for s in reversed(state):
        ic.restore_config(conv, s)


def tol_of(plan):
    return 1e-5 if plan.startswith("mf16") else 1e-4


def guarded(a, dev, dtype=torch.float32):
    """-> (buffer, view) of a flat array inside NaN bands of ic.GUARD floats (wgrad_cases.guarded's form)."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a).reshape(-1)
    buf = torch.full((a.size + 2 * ic.GUARD,), float("nan"), dtype=torch.float32)
    buf[ic.GUARD:ic.GUARD + a.size] = torch.from_numpy(a)
    buf = buf.to(dev)
    return buf, buf[ic.GUARD:ic.GUARD + a.size]


def bands_intact(*bufs):
    return all(b is None or (bool(torch.isnan(b[:ic.GUARD]).all()) and bool(torch.isnan(b[-ic.GUARD:]).all())) for b in bufs)


class Out:
    """n 4-byte elements of all-ones bytes (NaN as fp32) with GUARD_BYTES behind them (test_gpu_glue.Out's form)."""

    def __init__(self, n, dev):
        self.n = int(n)
        self.buf = torch.full((4 * self.n + GUARD_BYTES,), 255, dtype=torch.uint8, device=dev)

    def f32(self):
        return self.buf[:4 * self.n].view(torch.float32)

    def i32(self):
        return self.buf[:4 * self.n].view(torch.int32)

    def bits(self):
        """The owned words as uint32 on the host; the guard must be untouched."""
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[4 * self.n:] == 255).all(), "the bytes behind the output were written"
        return raw[:4 * self.n].view(np.uint32).copy()


def ref_of(c, exact, name=None, w_from=None):
    key = (name or c.name, exact)
    if key not in _REF:
        o = ic.operands(c, exact, name, w_from)
        v, off = ic.reference(c, o)
        _REF[key] = (o, v, off, ic.expected_buffer(c, o, v, off))
    return _REF[key]


def check_result(what, plan, bits, want, exact, wrote_all=False):
    """bits: the y buffer as uint32; want: float64, NaN where the launch owns nothing."""
    got = bits.view(np.float32)
    owned = ~np.isnan(want)
    assert owned.any() and (not wrote_all or owned.all())
    assert (bits[~owned] == 0xFFFFFFFF).all(), "%s: %d elements the launch does not own were written" % (what, int((bits[~owned] != 0xFFFFFFFF).sum()))
    g, w = got[owned].astype(np.float64), want[owned]
    if exact:
        bad = np.flatnonzero(~(g == w))
        assert bad.size == 0, "%s: %d of %d owned elements differ, first at %d: got %r want %r" % (what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])
    else:
        err = float(np.abs(g - w).max()) / float(np.abs(w).max())
        print("%s [%s]: %.3g of max |ref|" % (what, plan, err))
        if err == err:
            WORST[plan] = max(WORST.get(plan, 0.0), err)
        assert err <= tol_of(plan), "%s: error %.3g of max |ref| on %s" % (what, err, plan)


def check_sign(what, words, ybits, owned_words=None):
    """Every sign word the launch owns says (stored y > 0) bit by bit; the others keep their poison."""
    want = ic.sign_words(ybits.view(np.float32)).view(np.uint32)
    if owned_words is None:
        assert np.array_equal(words, want), what
    else:
        assert np.array_equal(words[owned_words], want[owned_words]) and (words[~owned_words] == 0xFFFFFFFF).all(), what


def weights(conv, dev, c, w):
    """The packed weights on the device ([rows][Kpad], inside NaN bands) with the twin conv.pack_weights would attach in this mode."""
    buf, flat = guarded(w, dev)
    wt = flat.view(-1, c.kpad)
    conv._maybe_split(wt, rows=wt.shape[0], cin=c.d["Cin"], taps=c.d["kh"] * c.d["kw"])
    if c.b16:
        conv.split_weights(wt)
    return buf, wt


def st():
    return torch.cuda.current_stream().cuda_stream


def launch(conv, dev, c, o, cfg, plans):
    """One launch of case c with operands o -> (y bits, sign words or None, owned sign words or None, input buffers)."""
    d = c.d
    N, Cout = d["N"], d["Cout"]
    xb, xf = guarded(o.x, dev)
    wb, wt = weights(conv, dev, c, o.w)
    sb, scale = guarded(o.scale, dev)
    hb, shift = guarded(o.shift, dev)
    ab, add = guarded(o.add, dev)
    a2b, add2 = guarded(o.add2, dev)
    mb, mask = guarded(o.mask, dev)
    mwords = None
    if mask is not None and c.mask_bits:
        mwords = torch.from_numpy(ic.sign_words(o.mask).view(np.int32)).to(dev)
        mask._rn_sign = mwords
    bufs = (xb, wb, sb, hb, ab, a2b, mb)
    dense_y = d["os"] == 1 and d["oo_h"] == d["oo_w"] == 0 and d["Hy"] == d["Ho"] and d["Wy"] == d["Wo"]
    own_stride = d["y_batch_stride"] == d["Hy"] * d["Wy"] * Cout
    geom = (d["Ho"], d["Wo"], Cout, d["kh"], d["kw"], d["a"], d["b"], (d["p"], d["p_w"]), d["div_shift"])
    sign = swords = None
    if c.via in ("fprop", "dgrad"):
        kind, k, stride, pad = c.conv
        x4 = xf.view(N, d["Hi"], d["Wi"], d["Cin"])
        kw = dict(scale=scale, shift=shift, act=o.act, mask=mask, mask_mode=d["mask_mode"] or 2, add=add, add_mode=d["add_mode"], plans=plans)
        if c.via == "fprop":
            y = conv.fprop(x4, wt, Cout, k, stride, pad, kw_pad=d["kw"] if d["kw"] != k else None, **kw)
        else:
            y = conv.dgrad(x4, wt, (d["Ho"], d["Wo"]), Cout, k, stride, pad, **kw)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (N, d["Ho"], d["Wo"], Cout) and y.is_contiguous()
        ybits = y.cpu().numpy().reshape(-1).view(np.uint32)
    elif c.via == "igemm":
        out = Out(o.ysize, dev)
        y = out.f32().view(N, d["Ho"], d["Wo"], Cout) if (dense_y and own_stride) else out.f32()
        conv.conv_igemm(xf.view(N, d["Hi"], d["Wi"], d["Cin"]), wt, y, geom, scale=scale, shift=shift, add=add, add_mode=d["add_mode"],
                        add_hw=(d["Ha"], d["Wa"]), mask=mask, mask_mode=d["mask_mode"] or 2, act=o.act,
                        y_batch_stride=None if own_stride else d["y_batch_stride"], add_batch_stride=d["add_batch_stride"] if d["add_mode"] else None,
                        in_relu=bool(d["in_relu"]), out_map=None if dense_y else (d["os"], d["oo_h"], d["oo_w"], d["Hy"], d["Wy"]),
                        add2=None if add2 is None else add2.view(N, d["Ha2"], d["Wa2"], Cout), w_batch_stride=d["w_batch_stride"],
                        sign=c.sign, bf16_products=c.b16, plans=plans)
        ybits = out.bits()
        if c.sign:
            assert hasattr(y, "_rn_sign")
            sign = y._rn_sign.cpu().numpy().view(np.uint32)
    else:                                               # "desc": what the wrappers cannot set
        lib = conv._hip.load()
        out = Out(o.ysize, dev)
        sout = Out(o.ysize // 32, dev) if c.sign else None
        d0 = ic.desc_of(c, conv)
        wptr, fmt, wus = conv._w_operand(wt, d0)
        tables = None
        if fmt == 3:                                    # one amax table per image, each from its own pass: the gaps hold NaN
            tables = torch.zeros(N * conv.AMAX_SUB, dtype=torch.int32, device=dev)
            img = d["Hi"] * d["Wi"] * d["Cin"]
            for n in range(N):
                assert lib.rn_amax(xf.data_ptr() + 4 * n * d["x_batch_stride"], img, 1, tables.data_ptr() + 4 * n * conv.AMAX_SUB, st()) == 0
        cd = ic.desc_of(c, conv, fmt, sign_out=None if sout is None else sout.buf.data_ptr(), x_amax=None if tables is None else tables.data_ptr(),
                        w_unscale=wus)
        plans.append(conv.igemm_plan(cd, scale is not None or shift is not None, splitk=False))
        ptr = conv._hip.ptr
        mptr = None if mask is None else (mwords.data_ptr() if mwords is not None else mask.data_ptr())
        rc = lib.rn_conv_igemm(ctypes.byref(cd), xf.data_ptr(), wptr, out.buf.data_ptr(), ptr(scale), ptr(shift), ptr(add), mptr, ptr(add2), st())
        assert rc == 0, rc
        ybits = out.bits()
        if c.sign:
            sign = sout.bits()
            swords = np.zeros(o.ysize // 32, dtype=bool)
            _, _, off, _ = ref_of(c, True)
            swords[((off[..., None] + np.arange(0, Cout, 32)) // 32).reshape(-1)] = True
    torch.cuda.synchronize()
    assert bands_intact(*bufs), "an input's NaN band changed"
    return ybits, sign, swords


RUNS = [(c, cfg) for c in ic.CASES for cfg in c.runs]


@pytest.mark.parametrize("c,cfg", RUNS, ids=["%s@%s" % (c.name, cfg) for c, cfg in RUNS])
def test_single_launch(conv, dev, config, c, cfg):
    config(cfg)
    for exact in (True, False):
        o, v, off, want = ref_of(c, exact)
        plans = []
        ybits, sign, swords = launch(conv, dev, c, o, cfg, plans)
        assert len(plans) == 1 and plans[0] is not None
        plan = ic.plan_name(plans[0])
        assert plan == c.runs[cfg], (c.name, cfg, plans[0])
        what = "%s@%s %s" % (c.name, cfg, "exact" if exact else "real")
        check_result(what, plan, ybits, want, exact, wrote_all=c.via in ("fprop", "dgrad"))
        if sign is not None:
            check_sign(what, sign, ybits, swords)
        if plans[0]["family"] == 3:                                           # split-K: slabs added in slice order, the same bits every run
            again, _, _ = launch(conv, dev, c, o, cfg, [])
            assert np.array_equal(again, ybits), what + ": two split-K runs differ"


GROUP_RUNS = [(g, cfg) for g in ic.GROUPS for cfg in g.runs]


@pytest.mark.parametrize("g,cfg", GROUP_RUNS, ids=["%s@%s" % (g.name, cfg) for g, cfg in GROUP_RUNS])
def test_grouped_launch(conv, dev, config, g, cfg):
    """Groups of 1, 2 and 5 problems through conv.conv_igemm_grouped: one-tile problems at the ends and in the middle, an addend or a mask on
    some members only, one member writing with a batch stride of its own."""
    config(cfg)
    for exact in (True, False):
        first = ref_of(g.cases[0], exact)[0]
        refs = [ref_of(c, exact, w_from=None if i == 0 else first) for i, c in enumerate(g.cases)]
        wb, wt = weights(conv, dev, g.cases[0], first.w)
        sb, scale = guarded(first.scale, dev)
        hb, shift = guarded(first.shift, dev)
        problems, outs, bufs = [], [], [wb, sb, hb]
        for c, (o, v, off, want) in zip(g.cases, refs):
            d = c.d
            xb, xf = guarded(o.x, dev)
            ab, add = guarded(o.add, dev)
            mb, mask = guarded(o.mask, dev)
            bufs += [xb, ab, mb]
            out = Out(o.ysize, dev)
            own = d["y_batch_stride"] == d["Ho"] * d["Wo"] * d["Cout"]
            pr = dict(x=xf.view(d["N"], d["Hi"], d["Wi"], d["Cin"]), y=out.f32().view(d["N"], d["Ho"], d["Wo"], d["Cout"]) if own else out.f32(),
                      geom=(d["Ho"], d["Wo"], d["Cout"], d["kh"], d["kw"], d["a"], d["b"], (d["p"], d["p_w"]), 0))
            if add is not None:
                pr["add"] = add
            if mask is not None:
                pr["mask"], pr["mask_mode"] = mask, d["mask_mode"]
            if not own:
                pr["y_batch_stride"] = d["y_batch_stride"]
            problems.append(pr)
            outs.append(out)
        plans = []
        conv.conv_igemm_grouped(problems, wt, scale=scale, shift=shift, act=first.act, plans=plans)
        assert len(plans) == 1 and plans[0] is not None
        plan = ic.plan_name(plans[0])
        assert plan == g.runs[cfg], (g.name, cfg, plans[0])
        for c, out, (o, v, off, want) in zip(g.cases, outs, refs):
            check_result("%s@%s %s" % (c.name, cfg, "exact" if exact else "real"), plan, out.bits(), want, exact)
        assert bands_intact(*bufs)


S2_RUNS = [(s, cfg) for s in ic.S2 for cfg in s.runs]


@pytest.mark.parametrize("s,cfg", S2_RUNS, ids=["%s@%s" % (s.name, cfg) for s, cfg in S2_RUNS])
def test_stride2_gradient_by_parity_classes(conv, dev, config, s, cfg):
    """conv.dgrad_s2_classes for k = 1, 3 and 7 on odd and even sizes: one launch per class through the output map at the four offsets, with
    an addend, a mask before or after it and the shortcut's add2 at the even positions."""
    config(cfg)
    for exact in (True, False):
        key = (s.name, exact)
        if key not in _REF:
            _REF[key] = ic.s2_build(s, exact)
        dy4, w, classes, dx_ref = _REF[key]
        o = classes[0][1]
        db, dyf = guarded(dy4, dev)
        ab, add = guarded(o.add, dev)
        mb, mask = guarded(o.mask, dev)
        a2b, add2 = guarded(o.add2, dev)
        wbufs, cws = zip(*[weights(conv, dev, c, oc.w) for c, oc in classes])
        plans = []
        kw = dict(plans=plans)
        if add is not None:
            kw.update(add=add, add_mode=1)
        if mask is not None:
            kw.update(mask=mask, mask_mode=s.mask)
        if add2 is not None:
            kw.update(add2=add2.view(s.N, (s.Hi + 1) // 2, (s.Wi + 1) // 2, s.cin))
        dx = conv.dgrad_s2_classes(dyf.view(s.N, s.Ho, s.Wo, s.cout), list(cws), (s.Hi, s.Wi), s.cin, s.k, s.pad, **kw)
        torch.cuda.synchronize()
        names = [ic.plan_name(p) for p in plans]
        assert names == s.runs[cfg], (s.name, cfg, plans)
        what = "%s@%s %s" % (s.name, cfg, "exact" if exact else "real")
        assert tuple(dx.shape) == dx_ref.shape
        got = dx.cpu().numpy().astype(np.float64)
        if exact:
            assert np.array_equal(got, dx_ref), what
        else:
            err = float(np.abs(got - dx_ref).max()) / float(np.abs(dx_ref).max())
            print("%s %s: %.3g of max |ref|" % (what, names, err))
            worst_plan = max(names, key=tol_of)                                   # the loosest bound among the classes' plans
            for n in set(names):
                WORST[n] = max(WORST.get(n, 0.0), err)
            assert err <= tol_of(worst_plan), (what, err)
        assert bands_intact(db, ab, mb, a2b, *wbufs)

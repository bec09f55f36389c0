"""CPU: tests/igemm_cases.py is worth trusting -- its float64 reference equals torch's float64 convolutions plus the epilogue in torch
operations wherever a case is an ordinary convolution, its exact cases are exact, and the launch path every case expects is the one the
launchers' own decision code reports (rn_conv_igemm_plan / rn_conv_igemm_grouped_plan are host code: the library loads without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import igemm_cases as ic


@pytest.fixture(scope="module")
def conv():
    from retinanet_mi355x import conv
    assert conv._hip.load().rn_fp32_split_min_k() == ic.SPLIT_MIN_K
    return conv


@pytest.fixture
def config(conv):
    state = []

    def use(name):
        state.append(ic.apply_config(conv, name))
    yield use
    for s in reversed(state):
        ic.restore_config(conv, s)


WORD = ctypes.c_float(0.0)
PTR = ctypes.addressof(WORD)                      # stands for every pointer the plan query only compares with NULL


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def nchw(a):
    return t64(a).permute(0, 3, 1, 2)


def torch_epilogue(c, o, acc):
    """scale, shift, mask before, add (same geometry or nearest x2 upsample cropped), activation, mask after -- on [N, C, H, W]."""
    d = c.d
    N, Ho, Wo, Cout = d["N"], d["Ho"], d["Wo"], d["Cout"]
    v = acc
    if o.scale is not None:
        v = v * t64(o.scale).view(1, -1, 1, 1)
    if o.shift is not None:
        v = v + t64(o.shift).view(1, -1, 1, 1)
    keep = None if o.mask is None else nchw(o.mask.reshape(N, Ho, Wo, Cout)) > 0
    if d["mask_mode"] == 1:
        v = torch.where(keep, v, torch.zeros_like(v))
    if d["add_mode"] == 1:
        v = v + nchw(o.add.reshape(N, Ho, Wo, Cout))
    elif d["add_mode"] == 2:
        up = F.interpolate(nchw(o.add.reshape(N, d["Ha"], d["Wa"], Cout)), scale_factor=2, mode="nearest")
        v = v + up[:, :, :Ho, :Wo]
    if o.act == 1:
        v = torch.relu(v)
    elif o.act == 2:
        v = torch.sigmoid(v)
    if d["mask_mode"] == 2:
        v = torch.where(keep, v, torch.zeros_like(v))
    return v


def dense_output(c):
    d = c.d
    return d["os"] == 1 and d["Hy"] == d["Ho"] and d["Wy"] == d["Wo"] and d["y_batch_stride"] == d["Ho"] * d["Wo"] * d["Cout"] and \
        (d["add_mode"] == 0 or d["add_batch_stride"] == (d["y_batch_stride"] if d["add_mode"] == 1 else d["Ha"] * d["Wa"] * d["Cout"]))


ORDINARY = [c for c in ic.CASES if c.conv is not None and dense_output(c) and c.M <= 4096]


def test_enough_ordinary_convolutions():
    assert len(ORDINARY) >= 25 and {c.conv[0] for c in ORDINARY} == {"fprop", "dgrad"}
    assert {c.d["add_mode"] for c in ORDINARY} == {0, 1, 2} and {c.d["mask_mode"] for c in ORDINARY} >= {0, 2}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("c", ORDINARY, ids=lambda c: c.name)
def test_reference_equals_torch(c, exact):
    o = ic.operands(c, exact)
    got, _ = ic.reference(c, o)
    kind, k, stride, pad = c.conv
    x = nchw(o.x4)
    if c.d["in_relu"]:
        x = torch.relu(x)
    if kind == "fprop":
        w = t64(o.w5[0][:, :k, :k, :]).permute(0, 3, 1, 2)                       # [Cout][kh][kw][Cin] -> OIHW; tap columns past k are zero
        assert c.d["kw"] == k or not o.w5[0][:, :, k:, :].any()
        acc = F.conv2d(x, w, None, stride, pad)
    else:
        w = t64(o.w5[0]).permute(3, 0, 1, 2)                                     # [cin][kh][kw][cout] -> conv_transpose2d's (in = cout, out = cin)
        hi, wi = c.d["Ho"], c.d["Wo"]
        opad = (hi - ((c.d["Hi"] - 1) * stride - 2 * pad + k), wi - ((c.d["Wi"] - 1) * stride - 2 * pad + k))
        acc = F.conv_transpose2d(x, w, None, stride, pad, output_padding=opad)
    want = torch_epilogue(c, o, acc).permute(0, 2, 3, 1).numpy()
    assert got.shape == want.shape
    if exact:
        assert np.array_equal(got, want)
    else:
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("s", ic.S2, ids=lambda s: s.name)
def test_parity_classes_equal_the_transposed_convolution(s, exact):
    """The classes' descriptors (conv.s2_classes geometry, out_map, add2 at even stored positions) assemble torch's stride-2 data gradient."""
    dy4, w, classes, dx = ic.s2_build(s, exact)
    opad = (s.Hi - ((s.Ho - 1) * 2 - 2 * s.pad + s.k), s.Wi - ((s.Wo - 1) * 2 - 2 * s.pad + s.k))
    v = F.conv_transpose2d(nchw(dy4), t64(w), None, 2, s.pad, output_padding=opad)
    o = classes[0][1]
    shape = (s.N, s.Hi, s.Wi, s.cin)
    owned = torch.zeros(shape, dtype=torch.bool)
    for c, _ in classes:
        owned[:, c.d["oo_h"]::2, c.d["oo_w"]::2, :] = True
    keep = None if o.mask is None else nchw(o.mask.reshape(shape)) > 0
    if s.mask == 1:
        v = torch.where(keep, v, torch.zeros_like(v))
    if s.add:
        v = v + nchw(o.add.reshape(shape))
    if s.add2:
        a2 = nchw(o.add2.reshape(s.N, (s.Hi + 1) // 2, (s.Wi + 1) // 2, s.cin))
        v[:, :, ::2, ::2] += a2
    if s.mask == 2:
        v = torch.where(keep, v, torch.zeros_like(v))
    want = torch.where(owned, v.permute(0, 2, 3, 1), torch.zeros(shape, dtype=torch.float64)).numpy()
    assert len(classes) == (1 if s.k == 1 else 4)
    if exact:
        assert np.array_equal(dx, want)
    else:
        assert np.abs(dx - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def _integers_below_2_24(*arrays):
    for a in arrays:
        if a is not None:
            a = np.asarray(a, dtype=np.float64)
            a = a[~np.isnan(a)]
            if not (np.array_equal(a, np.round(a)) and (np.abs(a).max() if a.size else 0) < 2 ** 24):
                return False
    return True


@pytest.mark.parametrize("c", ic.CASES + [m for g in ic.GROUPS for m in g.cases], ids=lambda c: c.name)
def test_exact_cases_are_exact(c):
    """Integer operands and an integer reference, and the largest value any partial sum or epilogue step can reach stays below 2^24."""
    o = ic.operands(c, True)
    v, off = ic.reference(c, o)
    assert _integers_below_2_24(o.x, o.w, o.shift, o.mask, o.add, o.add2, v)
    assert o.act in (0, 1)
    assert o.scale is None or set(np.abs(o.scale).tolist()) <= {1.0, 2.0, 4.0}
    assert (c.K * 16 * 4 + 3 + 4 + 4) < 2 ** 24
    assert np.abs(v).max() > 0 and len(np.unique(off)) == off.size                 # something to compare, every pixel stored once
    assert np.isnan(o.x).sum() == (c.d["N"] - 1) * c.xgap                          # NaN exactly in the gaps between images


def test_exact_parity_classes_are_exact():
    for s in ic.S2:
        dy4, w, classes, dx = ic.s2_build(s, True)
        assert _integers_below_2_24(dy4, w, dx, *[getattr(classes[0][1], n) for n in ("add", "mask", "add2")])


# ---------------------------------------------------------------------------------------------- the expected plans are the launchers'
def host_plan(conv, c, cfg):
    """The plan of conv.conv_igemm's launch of c under cfg: the split-K form where the wrapper would take it, else the weight form the
    wrapper would pass (igemm_cases.w_format)."""
    ya = PTR if ic.wants_y_amax(c, cfg) else None
    sg = PTR if c.sign else None
    d0 = ic.desc_of(c, conv, 0, sign_out=sg, y_amax=ya)
    affine = c.scale or c.shift
    if not c.b16 and conv._splitk_bytes(conv._hip.load(), d0) > 0:
        return conv.igemm_plan(d0, affine, splitk=True)
    fmt = ic.w_format(c, cfg)
    d = ic.desc_of(c, conv, fmt, sign_out=sg, y_amax=ya, x_amax=PTR if fmt == 3 else None, w_unscale=PTR if fmt == 3 else None)
    return conv.igemm_plan(d, affine, splitk=False)


def _tiles(p, M, cout):
    return -(-M // p["rows"]) * -(-cout // p["cols"])


@pytest.mark.parametrize("c", ic.CASES, ids=lambda c: c.name)
def test_case_plans(conv, config, c):
    assert c.runs and set(c.runs) <= set(ic.CONFIGS)
    for cfg, want in c.runs.items():
        config(cfg)
        p = host_plan(conv, c, cfg)
        assert p is not None, (c.name, cfg)
        assert ic.plan_name(p) == want, (c.name, cfg, p)
        assert p["grid"] == _tiles(p, c.M, c.d["Cout"]), (c.name, cfg, p)
        for k, v in c.extra.get(cfg, {}).items():
            assert p[k] == v, (c.name, cfg, k, p)
        if p["family"] == 3:
            nks = (c.K + 31) // 32 * 32 // 16
            assert 2 <= p["used"] <= p["slices"] <= 32 and p["steps"] * p["used"] >= nks > p["steps"] * (p["used"] - 1), p


def test_split_k_cases_cut_taps_and_leave_slices_idle(conv, config):
    """What the split-K cases are there for: a slice border inside a filter tap, and fewer slices used than asked for."""
    config("native-sk")
    mid = [c for c in ic.CASES if "native-sk" in c.runs and c.runs["native-sk"].startswith("splitk")]
    plans = {c.name: host_plan(conv, c, "native-sk") for c in mid}
    assert sum(1 for c in mid if plans[c.name]["steps"] % (c.d["Cin"] // 16) != 0) >= 4
    assert any(p["used"] < p["slices"] for p in plans.values())


@pytest.mark.parametrize("g", ic.GROUPS, ids=lambda g: g.name)
def test_group_plans(conv, config, g):
    for cfg, want in g.runs.items():
        config(cfg)
        fmt = ic.w_format(g.cases[0], cfg)
        p = conv.igemm_grouped_plan(ic.group_of(g, conv, fmt, PTR))
        assert p is not None and ic.plan_name(p) == want, (g.name, cfg, p)
        assert p["grid"] == sum(_tiles(p, c.M, c.d["Cout"]) for c in g.cases), (g.name, cfg, p)


def test_groups_have_the_sizes_and_members_asked_for():
    assert {len(g.cases) for g in ic.GROUPS} >= {1, 2, 5}
    five = ic.GROUPS[0].cases
    assert [-(-c.M // 256) for c in five][2] == 1 and [-(-c.M // 128) for c in five] == [1, 3, 1, 3, 1]
    assert len({(c.d["add_mode"], c.d["mask_mode"]) for c in five}) >= 4


@pytest.mark.parametrize("s", ic.S2, ids=lambda s: s.name)
def test_parity_class_plans(conv, config, s):
    _, _, classes, _ = ic.s2_build(s, True)
    for cfg, wants in s.runs.items():
        config(cfg)
        assert len(wants) == len(classes)
        for (c, _), want in zip(classes, wants):
            fmt = ic.w_format(c, cfg)
            d = ic.desc_of(c, conv, fmt, y_amax=PTR if ic.CONFIGS[cfg][0] == "split3" else None, x_amax=PTR if fmt == 3 else None,
                           w_unscale=PTR if fmt == 3 else None)
            p = conv.igemm_plan(d, False, splitk=False)
            assert p is not None and ic.plan_name(p) == want, (c.name, cfg, p)


def test_the_tables_reach_every_plan_declared_reachable():
    assert ic.plan_keys() == ic.REACHABLE, (sorted(ic.REACHABLE - ic.plan_keys()), sorted(ic.plan_keys() - ic.REACHABLE))
    assert len(ic.REACHABLE) >= 55 and set(ic.UNREACHABLE) == {"RN_SPLIT_A_ONCE=0", "RN_MF16_WV8_MIN=0 or > tiles", "RN_MF16_STG_MIN_K",
                                                              "RN_FP32_SPLIT_MIN_K"}


def test_every_feature_runs_on_a_narrow_a_wide_and_an_mf16_path():
    """Per feature, the families of the plans its cases reach (mf16 only where the launcher allows the feature there)."""
    def fams(pred):
        out = set()
        for c in ic.CASES:
            if pred(c):
                for p in c.runs.values():
                    out.add("mf16" if p.startswith("mf16") else ("narrow" if " 256x64/" in p else "wide"))
        return out
    every = {"narrow", "wide", "mf16"}
    assert fams(lambda c: c.d["Cout"] % 4 != 0) == {"narrow", "wide"}                              # the 16x16x32 kernels need Cout % 4 == 0
    assert fams(lambda c: c.d["add_mode"] == 2 and (c.d["Ho"] & 1) and (c.d["Wo"] & 1)) == every
    for oo in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert fams(lambda c: c.d["os"] == 2 and (c.d["oo_h"], c.d["oo_w"]) == oo and c.d["add2_mode"] == 3) == every
    assert fams(lambda c: c.d["add_mode"] == 1 and c.d["add_batch_stride"] != c.d["y_batch_stride"]) == every
    assert fams(lambda c: c.xgap > 0) == every
    assert fams(lambda c: c.d["p"] != c.d["p_w"] and c.d["kw"] > 1) == every
    assert fams(lambda c: c.d["div_shift"] == 1 and c.d["Cin"] % 16 != 0) == {"narrow", "wide"}    # div_shift keeps a launch off the mf16 kernels
    assert fams(lambda c: c.d["Cin"] == 4 and c.d["kw"] == 8) == {"narrow"}                       # the stem has 64 output channels
    assert fams(lambda c: c.d["Ho"] * c.d["Wo"] <= 9 and c.d["N"] >= 40) == every
    assert fams(lambda c: c.M < 128) == every
    assert fams(lambda c: c.d["Cout"] == 65) == {"wide"} and fams(lambda c: c.d["Cout"] == 132) == {"wide", "mf16"}
    assert fams(lambda c: c.K < 32) == {"narrow", "wide"}
    assert fams(lambda c: c.d["kh"] == 1 and c.d["a"] == 2) == every
    assert fams(lambda c: c.d["kh"] == 7 and c.d["p"] == -3) == {"narrow", "wide"}                 # 49 taps: not the mf16 kernels'
    assert fams(lambda c: c.d["Hi"] == 1 or c.d["Wi"] == 1) == every
    assert fams(lambda c: c.d["in_relu"]) == {"wide"}                                              # the input ReLU has 128 x 128 instances only
    for mode in (1, 2):
        for bits in (False, True):
            assert fams(lambda c: c.d["mask_mode"] == mode and c.mask_bits == bits) >= {"mf16"} | ({"narrow"} if (mode, bits) != (1, True) else {"wide"})
    assert fams(lambda c: c.sign) == every
    assert fams(lambda c: c.wbatch) == every


# ---------------------------------------------------------------------------------------------- refusals
def test_the_query_refuses_what_the_launchers_refuse(conv, config):
    base = ic.BY_NAME["narrow-dense-3x3"]

    def plan(over=None, fmt=0, ask_splitk=False, **ptrs):
        c = ic.Case("refused", dict(base.d, **(over or {})), {})
        return conv.igemm_plan(ic.desc_of(c, conv, fmt, **ptrs), False, splitk=ask_splitk)

    config("native")
    assert plan() is not None
    assert plan(dict(Cin=6)) is None and plan(dict(Cin=0)) is None and plan(dict(kh=0)) is None and plan(dict(div_shift=3)) is None
    assert plan(dict(add_mode=3)) is None and plan(dict(act=3)) is None and plan(dict(mask_mode=3)) is None and plan(dict(add2_mode=1)) is None
    assert plan(dict(os=2, Hy=18, Wy=14, add_mode=2, Ha=5, Wa=4)) is None                          # no upsample-add through an output map
    assert plan(dict(Hy=8)) is None                                                              # the map leaves the tensor
    assert plan(dict(Cout=48), sign_out=PTR) is None                                             # sign bits need whole words per pixel
    assert plan(fmt=1) is None and plan(fmt=3, x_amax=PTR, w_unscale=PTR) is None                # pre-split operands in native mode
    assert plan(fmt=4) is None and plan(dict(w_batch_stride=64 * 160)) is None                   # Ho*Wo % 256 for a batch of GEMMs
    assert plan(dict(Cout=72), fmt=2) is None and plan(dict(in_relu=1), fmt=2) is None           # w_format 2: narrow instances only
    assert plan(ask_splitk=True) is None                                                         # split-K is off / not worthwhile here
    out = (ctypes.c_int32 * 16)()
    out[0] = 4
    assert conv._hip.load().rn_conv_igemm_plan(ctypes.byref(ic.desc_of(base, conv)), out) == 10001      # an ask bit nobody defined
    assert conv._hip.load().rn_conv_igemm_plan(ctypes.byref(ic.desc_of(base, conv)), None) == 10001
    config("split3")
    assert plan(fmt=3) is None and plan(fmt=3, x_amax=PTR, w_unscale=PTR) is not None
    config("native-sk")
    long_k = ic.BY_NAME["splitk-mid-tap-narrow-dense"]
    assert conv.igemm_plan(ic.desc_of(long_k, conv, 0), True, splitk=True) is not None
    assert conv.igemm_plan(ic.desc_of(long_k, conv, 1), True, splitk=True) is None                # the split-K form takes fp32 weights only

    config("native")
    g = ic.GROUPS[0]
    ok = ic.group_of(g, conv, 0, PTR)
    assert conv.igemm_grouped_plan(ok) is not None
    for spoil in ("n0", "n6", "tile_end", "in_relu", "add_ptr", "fmt2", "fmt1", "cin", "add2"):
        cg = ic.group_of(g, conv, 0, PTR)
        if spoil == "n0":
            cg.n = 0
        elif spoil == "n6":
            cg.n = 6
        elif spoil == "tile_end":
            cg.tile_end[1] += 1
        elif spoil == "in_relu":
            cg.d[2].in_relu = 1
        elif spoil == "add_ptr":
            cg.add[0] = PTR                                                                      # an addend its descriptor does not name
        elif spoil == "fmt2":
            for i in range(cg.n):
                cg.d[i].w_format = 2
        elif spoil == "fmt1":
            cg.d[1].w_format = 1
        elif spoil == "cin":
            cg.d[3].Cin = 32
        else:
            cg.d[4].add2_mode = 3
        assert conv.igemm_grouped_plan(cg) is None, spoil

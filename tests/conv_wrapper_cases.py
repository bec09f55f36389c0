"""The cases of tests/test_conv_wrappers_host.py and their recorded answers.

  DEFAULTS       what the stand-in library answers to the pure host queries, and the profiler switches; a case overrides single entries
  CASES          [(name, settings, fn)]: fn(env) calls ONE wrapper of retinanet_mi355x/conv.py or one method of engine.Layer on small CPU
                 tensors (env: test_conv_wrappers_host.Env) and returns what the wrapper returned
  EXPECTED       {name: record}: test_conv_wrappers_host.observe() on the wrappers before their fp32 / bf16 / fp8 copies were folded onto
                 shared builders (python tests/test_conv_wrappers_host.py prints it; its docstring says how a record reads)
  ENTRY_POINTS, KIND_PREFIXES, GROUPED   what the table must reach (test_the_table_reaches_every_wrapper)

No kernel runs, so a geometry only has to satisfy the Python: shapes are the smallest that take a branch.
"""
NATIVE, SPLIT, SPLIT3 = 0, 1, 2                     # rn_get_fp32_mfma
OPT_DETERMINISTIC = 1

DEFAULTS = dict(mfma=NATIVE, options={}, split_min_k=64, splitk_ws=0, wants_f16=0, tile=128128, tile_rows=128128, timer=True, by_shape=False)

ENTRY_POINTS = {"rn_conv_igemm", "rn_conv_igemm_splitk", "rn_conv_igemm_grouped", "rn_conv_igemm_bf16", "rn_conv_igemm_bf16_grouped",
                "rn_conv_igemm_fp8", "rn_conv_igemm_fp8_grouped", "rn_amax", "rn_split_weights", "rn_conv_wgrad_batched",
                "rn_conv_wgrad_batched_det", "rn_conv_wgrad_det_workspace_bytes", "rn_conv_wgrad_bf16", "rn_conv_wgrad_bf16_grouped",
                "rn_conv_bwd_1x1",
                "rn_wino_input_group", "rn_wino_input_group_list", "rn_wino_input_both_group_flags", "rn_wino_input_both_group_lists",
                "rn_wino_output_group", "rn_wino_output_group_flags", "rn_wino_output_group_list", "rn_tile_lists", "rn_wino_dw",
                "rn_conv_wgrad_batched_flags"}
KIND_PREFIXES = {"conv_igemm_4x1", "conv_igemm_2x2", "stem", "conv_igemm_bf16", "conv_igemm_bf16_p8", "conv_igemm_fp8", "conv_igemm_fp8_p8",
                 "conv_wgrad", "conv_wgrad_bf16", "conv_bwd_fused", "wino_input", "wino_output"}
GROUPED = ("rn_conv_igemm_grouped", "rn_conv_igemm_bf16_grouped", "rn_conv_igemm_fp8_grouped")

CASES = []


def case(name, **settings):
    def add(fn):
        CASES.append((name, settings, fn))
        return fn
    return add


def variants(name, **by_suffix):
    """One function under several settings: name + "/" + suffix each."""
    def add(fn):
        for suffix, settings in by_suffix.items():
            CASES.append((name + "/" + suffix, settings, fn))
        return fn
    return add


GEOM = (8, 8, 64, 3, 3, 1, 1, -1, 0)                # 3x3 / stride 1 / padding 1 on 8 x 8, 64 output channels


def kpad(k, c):
    return (k * k * c + 31) // 32 * 32


def xwy(env, cin=32, cout=64, k=3, hw=(8, 8), dtype=None, ydtype=None, wdtype=None):
    """x [2, H, W, cin], packed weights [cout, Kpad], y [2, H, W, cout] and the epilogue vectors."""
    t = env.torch
    dtype = dtype or t.float32
    x = env.t("x", (2,) + hw + (cin,), dtype)
    w = env.t("w", (cout, kpad(k, cin)), wdtype or dtype)
    y = env.t("y", (2,) + hw + (cout,), ydtype or dtype)
    return x, w, y, env.t("scale", (cout,)), env.t("shift", (cout,))


def twins(env, w, split=False, split16=False):
    t = env.torch
    if split:
        w._rn_split = t.zeros(w.numel() * 6, dtype=t.uint8)
    if split16:
        w._rn_split16 = (t.zeros(w.numel() * 4, dtype=t.uint8), t.zeros(w.shape[0], dtype=t.float32))
    return w


def with_sign(env, name, shape, dtype=None):
    """A tensor whose producer left its sign bits."""
    t = env.torch
    m = env.t(name, shape, dtype or t.float32)
    m._rn_sign = t.zeros(m.numel() // 32, dtype=t.int32)
    return m


# ------------------------------------------------------------------------------------------------------------------ conv_igemm
@variants("igemm/plain", native={}, split3=dict(mfma=SPLIT3), by_shape=dict(by_shape=True), no_timer=dict(timer=False))
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, scale=sc, shift=sh, act=env.cv.ACT_RELU, flops=1e6)


@case("igemm/wide_in_relu_kind", by_shape=True)
def _(env):
    x, w, y, sc, sh = xwy(env, cout=96)
    return env.cv.conv_igemm(x, w, y, (8, 8, 96, 3, 3, 1, 1, (-1, -2), 0), shift=sh, in_relu=True, flops=2e6)


@case("igemm/kind_given", by_shape=True)
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, kind="stem", act=env.cv.ACT_SIGMOID)


@case("igemm/add_mode1")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, scale=sc, add=env.t("add", y.shape), add_mode=1, flops=1e6)


@case("igemm/add_mode1_add_batch_stride")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, add=env.t("add", (2, 8, 8, 128)), add_mode=1, add_batch_stride=8 * 8 * 128)


@case("igemm/add_mode2")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, add=env.t("add", (2, 4, 4, 64)), add_mode=2, add_hw=(4, 4), flops=1e6)


@case("igemm/mask_fp32")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, mask=env.t("mask", y.shape), flops=1e6)


@case("igemm/mask_fp32_mode1")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, mask=env.t("mask", y.shape), mask_mode=1, add=env.t("add", y.shape), add_mode=1)


@case("igemm/mask_bits")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, mask=with_sign(env, "mask", y.shape), flops=1e6)


@case("igemm/sign", mfma=SPLIT3)
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, act=env.cv.ACT_RELU, sign=True, flops=1e6)


@case("igemm/sign_no_words")
def _(env):
    x, w, y, sc, sh = xwy(env, cout=48)
    return env.cv.conv_igemm(x, w, y, (8, 8, 48, 3, 3, 1, 1, -1, 0), act=env.cv.ACT_RELU, sign=True)


@case("igemm/reused_destination", mfma=SPLIT3)
def _(env):
    x, w, y, sc, sh = xwy(env)
    y._rn_sign = env.torch.zeros(y.numel() // 32, dtype=env.torch.int32)          # what an earlier producer left: dropped
    y._rn_amax = (env.torch.zeros(2 * 64, dtype=env.torch.int32), y._version)
    return env.cv.conv_igemm(x, w, y, GEOM)


@case("igemm/out_map", mfma=SPLIT3)
def _(env):
    x, w, _, sc, sh = xwy(env)
    y = env.t("y16", (2, 16, 16, 64))
    return env.cv.conv_igemm(x, w, y, GEOM, out_map=(2, 1, 0, 16, 16), sign=True, flops=1e6)


@case("igemm/out_map_shared_amax", mfma=SPLIT3)
def _(env):
    x, w, _, sc, sh = xwy(env)
    y = env.t("y16", (2, 16, 16, 64))
    return env.cv.conv_igemm(x, w, y, GEOM, out_map=(2, 0, 1, 16, 16), amax=env.t("slot", (2 * 64,), env.torch.int32))


@case("igemm/add2")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, add2=env.t("add2", (2, 4, 4, 64)), mask=env.t("mask", y.shape), flops=1e6)


@case("igemm/y_batch_stride", mfma=SPLIT3)
def _(env):
    x, w, _, sc, sh = xwy(env)
    buf = env.t("ybuf", (2, 3 * 8 * 8 * 64))
    return env.cv.conv_igemm(x, w, buf[:, 8 * 8 * 64:], GEOM, y_batch_stride=3 * 8 * 8 * 64, sign=True, add=env.t("add", (2, 8, 8, 64)), add_mode=1)


def tile_lists(env, tpad, grid):
    tl = env.cv.TileLists()
    tl.blocks, tl.counts, tl.grid = env.t("blocks", (tpad // 128,), env.torch.int32), env.t("counts", (4,), env.torch.int32), grid
    return tl


@variants("igemm/wino_stage", native={}, split3_f16=dict(mfma=SPLIT3, wants_f16=1, by_shape=True), split3_three_term=dict(mfma=SPLIT3, wants_f16=0))
def _(env):
    """The 36 GEMMs of a Winograd layer: per-plane weights, row amax words, tile flags and their work list."""
    i32 = env.torch.int32
    V, M = env.t("V", (36, 1, 256, 32)), env.t("M", (36, 1, 256, 64))
    U = twins(env, env.t("U", (36 * 64, 32)), split=True, split16=True)
    return env.cv.conv_igemm(V, U, M, (1, 256, 64, 1, 1, 1, 1, 0, 0), flops=3e6, w_batch_stride=64 * 32, x_amax=env.t("rows", (256,), i32),
                             x_amax_rows=True, row_active=env.t("flags", (256,), env.torch.uint8), row_list=tile_lists(env, 256, 3))


@case("igemm/bf16_products", mfma=SPLIT3, wants_f16=1)
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, twins(env, w, split=True, split16=True), y, GEOM, bf16_products=True, flops=1e6)


@case("igemm/bf16_products_twin_made")
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, bf16_products=True, sign=True, act=env.cv.ACT_RELU)


@variants("igemm/splitk", native=dict(splitk_ws=4096, by_shape=True), split3=dict(splitk_ws=4096, mfma=SPLIT3))
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, twins(env, w, split=True, split16=True), y, GEOM, scale=sc, shift=sh, add=env.t("add", y.shape), add_mode=1,
                             mask=with_sign(env, "mask", y.shape), sign=True, flops=1e6)


@variants("igemm/splitk_shared_amax", split3=dict(splitk_ws=4096, mfma=SPLIT3))
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, out_map=(1, 0, 0, 8, 8), amax=env.t("slot", (2 * 64,), env.torch.int32))


@variants("igemm/w_format", native_twins=dict(mfma=NATIVE), split_twin=dict(mfma=SPLIT), split3_f16=dict(mfma=SPLIT3, wants_f16=1),
          split3_refused=dict(mfma=SPLIT3, wants_f16=0))
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, twins(env, w, split=True, split16=True), y, GEOM, flops=1e6)


@case("igemm/w_format_no_twin", mfma=SPLIT3, wants_f16=1)
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, w, y, GEOM, flops=1e6)


@variants("igemm/w_format3_x_amax", words_given=dict(mfma=SPLIT3, wants_f16=1))
def _(env):
    x, w, y, sc, sh = xwy(env)
    return env.cv.conv_igemm(x, twins(env, w, split16=True), y, GEOM, x_amax=env.t("xam", (2 * 64,), env.torch.int32), mask=env.t("mask", y.shape),
                             add2=env.t("add2", (2, 4, 4, 64)), sign=True, flops=1e6)


# ------------------------------------------------------------------------------------------------------------------ conv_igemm_bf16 / _fp8
P8 = dict(p8_off={}, p8_single=dict(tile=256256, by_shape=True), no_timer=dict(timer=False, tile=256256))


@variants("bf16/plain", p8_persistent=dict(tile=1256256), **P8)
def _(env):
    x, w, y, sc, sh = xwy(env, dtype=env.torch.bfloat16)
    return env.cv.conv_igemm_bf16(x, w, y, GEOM, scale=sc, shift=sh, act=env.cv.ACT_RELU, sign=True, flops=1e6)


@case("bf16/fp32_result", tile=256256)
def _(env):
    x, w, y, sc, sh = xwy(env, dtype=env.torch.bfloat16, ydtype=env.torch.float32)
    return env.cv.conv_igemm_bf16(x, w, y, GEOM, shift=sh, act=env.cv.ACT_SIGMOID, sign=True, y_batch_stride=8 * 8 * 64, flops=1e6)


@case("bf16/add_mask")
def _(env):
    bf = env.torch.bfloat16
    x, w, y, sc, sh = xwy(env, dtype=bf)
    return env.cv.conv_igemm_bf16(x, w, y, GEOM, add=env.t("add", y.shape, bf), add_mode=1, mask=env.t("mask", y.shape, bf), mask_mode=1)


@case("bf16/add_mode2_mask_bits")
def _(env):
    bf = env.torch.bfloat16
    x, w, y, sc, sh = xwy(env, dtype=bf)
    y._rn_sign = env.torch.zeros(y.numel() // 32, dtype=env.torch.int32)
    return env.cv.conv_igemm_bf16(x, w, y, GEOM, add=env.t("add", (2, 4, 4, 64), bf), add_mode=2, add_hw=(4, 4), mask=with_sign(env, "mask", y.shape, bf),
                                  add_batch_stride=None)


@case("bf16/out_map")
def _(env):
    bf = env.torch.bfloat16
    x, w, _, sc, sh = xwy(env, dtype=bf)
    y = env.t("y16", (2, 16, 16, 64), bf)
    return env.cv.conv_igemm_bf16(x, w, y, GEOM, out_map=(2, 0, 0, 16, 16), add=y, add_mode=1, sign=True, flops=1e6)


@variants("fp8/plain", **P8)
def _(env):
    u8 = env.torch.uint8
    x, w, y, sc, sh = xwy(env, dtype=u8)
    return env.cv.conv_igemm_fp8(x, w, y, GEOM, sc, shift=sh, act=env.cv.ACT_RELU, out_scale=0.25, flops=1e6)


@case("fp8/fp32_result", tile=256256)
def _(env):
    u8 = env.torch.uint8
    x, w, y, sc, sh = xwy(env, dtype=u8, ydtype=env.torch.float32)
    y._rn_amax = (env.torch.zeros(2 * 64, dtype=env.torch.int32), y._version)
    return env.cv.conv_igemm_fp8(x, w, y, GEOM, sc, y_batch_stride=8 * 8 * 64, out_scale=0.25, flops=1e6)


@case("fp8/add")
def _(env):
    u8 = env.torch.uint8
    x, w, y, sc, sh = xwy(env, dtype=u8)
    add = env.t("add", y.shape, u8)
    add._rn_scale = 0.125
    return env.cv.conv_igemm_fp8(x, w, y, GEOM, sc, shift=sh, add=add, add_mode=1, out_scale=0.5, flops=1e6)


@case("fp8/add_mode2")
def _(env):
    u8 = env.torch.uint8
    x, w, y, sc, sh = xwy(env, dtype=u8)
    add = env.t("add", (2, 4, 4, 64), u8)
    add._rn_scale = 2.0
    return env.cv.conv_igemm_fp8(x, w, y, GEOM, sc, add=add, add_mode=2, add_hw=(4, 4))


# ------------------------------------------------------------------------------------------------------------------ the grouped wrappers
LEVELS = [(16, 12), (4, 4), (2, 2), (1, 1), (3, 5)]        # the first: more than one tile of every kind


def problems(env, n, cin, cout, dtype, ydtype, k=3, ybs=False, add=False, mask=None, sign=False):
    """n problems over LEVELS; ybs: results are slices of one buffer (batch stride); mask: "fp32" / "bits" / "mixed"."""
    out = []
    rows = sum(h * w for h, w in LEVELS[:n])
    buf = env.t("ybuf", (2, rows, cout), ydtype) if ybs else None
    r0 = 0
    for i, (h, w) in enumerate(LEVELS[:n]):
        pr = {"x": env.t("x%d" % i, (2, h, w, cin), dtype), "geom": (h, w, cout, k, k, 1, 1, -(k // 2), 0)}
        if ybs:
            pr["y"], pr["y_batch_stride"] = buf[:, r0:r0 + h * w], rows * cout
            r0 += h * w
        else:
            pr["y"] = env.t("y%d" % i, (2, h, w, cout), ydtype)
        if add:
            pr["add"] = env.t("add%d" % i, (2, h, w, cout), ydtype)
        if mask is not None:
            bits = mask == "bits" or (mask == "mixed" and i % 2 == 0)
            pr["mask"] = with_sign(env, "mask%d" % i, (2, h, w, cout), ydtype) if bits else env.t("mask%d" % i, (2, h, w, cout), ydtype)
            if mask == "mixed" and i == 1:
                pr["mask_mode"] = 1
        if sign:
            pr["sign"] = True
        out.append(pr)
    return out


def grouped_fp32(n, cout, twin=False, **kw):
    def fn(env):
        f32 = env.torch.float32
        probs = problems(env, n, 32, cout, f32, f32, **kw)
        w = twins(env, env.t("w", (cout, kpad(3, 32))), split=twin, split16=twin)
        return env.cv.conv_igemm_grouped(probs, w, scale=env.t("scale", (cout,)), shift=env.t("shift", (cout,)), act=env.cv.ACT_RELU, flops=5e6)
    return fn


case("grouped/n1_cout64")(grouped_fp32(1, 64, sign=True))
case("grouped/n1_cout128", mfma=SPLIT3, wants_f16=1)(grouped_fp32(1, 128, sign=True))
case("grouped/n3_cout64", mfma=SPLIT3, wants_f16=1)(grouped_fp32(3, 64, twin=True, sign=True))
case("grouped/n3_cout128", by_shape=True)(grouped_fp32(3, 128, twin=True, sign=True))
case("grouped/n5_cout64", timer=False)(grouped_fp32(5, 64))
case("grouped/n5_cout128", mfma=SPLIT3)(grouped_fp32(5, 128))
variants("grouped/ybs_add_mask", split=dict(mfma=SPLIT), split3=dict(mfma=SPLIT3, wants_f16=1))(
    grouped_fp32(3, 64, twin=True, ybs=True, add=True, mask="mixed", sign=True))
case("grouped/add_mask_bits")(grouped_fp32(2, 128, twin=True, add=True, mask="bits", sign=True))
case("grouped/no_twin", mfma=SPLIT3, wants_f16=1)(grouped_fp32(2, 64, add=True, mask="fp32"))


def grouped_bf16(n, yf32=False, cout=64, **kw):
    def fn(env):
        bf = env.torch.bfloat16
        probs = problems(env, n, 32, cout, bf, env.torch.float32 if yf32 else bf, **kw)
        return env.cv.conv_igemm_bf16_grouped(probs, env.t("w", (cout, kpad(3, 32)), bf), scale=env.t("scale", (cout,)), shift=env.t("shift", (cout,)),
                                              act=env.cv.ACT_RELU, flops=5e6)
    return fn


def grouped_fp8(n, yf32=False, cout=64, **kw):
    def fn(env):
        u8 = env.torch.uint8
        probs = problems(env, n, 32, cout, u8, env.torch.float32 if yf32 else u8, **kw)
        return env.cv.conv_igemm_fp8_grouped(probs, env.t("w", (cout, kpad(3, 32)), u8), env.t("scale", (cout,)), shift=env.t("shift", (cout,)),
                                             act=env.cv.ACT_RELU, out_scale=0.25, flops=5e6)
    return fn


for _grouped, _name in ((grouped_bf16, "grouped_bf16"), (grouped_fp8, "grouped_fp8")):
    variants(_name + "/n1", t128={}, no_timer=dict(timer=False))(_grouped(1, sign=True))
    variants(_name + "/n3", t128={}, t256=dict(tile_rows=256256, by_shape=True))(_grouped(3))
    variants(_name + "/n5", t256=dict(tile_rows=256256), t256x128=dict(tile_rows=256128))(_grouped(5, cout=160, sign=True))
    case(_name + "/fp32_results")(_grouped(3, yf32=True, ybs=True, sign=True))
    case(_name + "/ybs_add_mask", tile_rows=256256)(_grouped(3, ybs=True, add=True, mask="mixed", sign=True))
case("grouped_bf16/add_mask_bits")(grouped_bf16(2, add=True, mask="bits", sign=True))


# ------------------------------------------------------------------------------------------------------------------ fprop / dgrad / parity classes
def class_weights(env, cv, k, pad, cin, cout_pad, dtype, name="wc"):
    return [env.t("%s[%d]" % (name, i), (cin, (c[2][1] * c[2][3] * cout_pad + 31) // 32 * 32), dtype) for i, c in enumerate(cv.s2_classes(k, pad))]


@case("fprop", mfma=SPLIT3)
def _(env):
    x = env.t("x", (2, 9, 7, 32))
    return env.cv.fprop(x, env.t("w", (64, kpad(3, 32))), 64, 3, 2, 1, shift=env.t("shift", (64,)), act=env.cv.ACT_RELU, sign=True, flops=1e6)


@case("fprop/kw_pad")
def _(env):
    x = env.t("x", (2, 16, 16, 4))
    return env.cv.fprop(x, env.t("w", (64, (7 * 8 * 4 + 31) // 32 * 32)), 64, 7, 2, 3, kw_pad=8, flops=1e6)


@case("dgrad/stride1", mfma=SPLIT3)
def _(env):
    dy = env.t("dy", (2, 8, 8, 64))
    return env.cv.dgrad(dy, env.t("wd", (32, kpad(3, 64))), (8, 8), 32, 3, 1, 1, mask=with_sign(env, "mask", (2, 8, 8, 32)), add=env.t("add", (2, 8, 8, 32)),
                        add_mode=1, flops=1e6)


@case("dgrad/stride2_1x1_add2", by_shape=True)
def _(env):
    dy = env.t("dy", (2, 4, 4, 64))
    return env.cv.dgrad(dy, env.t("wd", (32, kpad(1, 64))), (8, 8), 32, 1, 2, 0, add2=env.t("add2", (2, 4, 4, 32)), flops=1e6)


@variants("s2_classes/k3", native=dict(by_shape=True), split3=dict(mfma=SPLIT3), splitk_split3=dict(mfma=SPLIT3, splitk_ws=1024))
def _(env):
    dy = env.t("dy", (2, 4, 4, 64))
    wc = class_weights(env, env.cv, 3, 1, 32, 64, env.torch.float32)
    return env.cv.dgrad_s2_classes(dy, wc, (8, 7), 32, 3, 1, flops=9e6, add=env.t("add", (2, 8, 7, 32)), add_mode=1, mask=env.t("mask", (2, 8, 7, 32)))


@case("s2_classes/k1", mfma=SPLIT3)
def _(env):
    dy = env.t("dy", (2, 4, 4, 64))
    wc = class_weights(env, env.cv, 1, 0, 32, 64, env.torch.float32)
    return env.cv.dgrad_s2_classes(dy, wc, (8, 8), 32, 1, 0, flops=1e6)


@case("s2_classes/empty_class", mfma=SPLIT3)
def _(env):
    dy = env.t("dy", (2, 1, 1, 64))
    wc = class_weights(env, env.cv, 3, 1, 32, 64, env.torch.float32)
    return env.cv.dgrad_s2_classes(dy, wc, (1, 1), 32, 3, 1, flops=9e6)


@case("fprop_bf16", tile=256256)
def _(env):
    bf = env.torch.bfloat16
    return env.cv.fprop_bf16(env.t("x", (2, 9, 7, 32), bf), env.t("w", (64, kpad(3, 32)), bf), 64, 3, 2, 1, shift=env.t("shift", (64,)), sign=True, flops=1e6)


@case("fprop_bf16/fp32_out")
def _(env):
    bf = env.torch.bfloat16
    return env.cv.fprop_bf16(env.t("x", (2, 8, 8, 32), bf), env.t("w", (64, kpad(1, 32)), bf), 64, 1, 1, 0, out_dtype=env.torch.float32, flops=1e6)


@case("dgrad_bf16", by_shape=True)
def _(env):
    bf = env.torch.bfloat16
    return env.cv.dgrad_bf16(env.t("dy", (2, 8, 8, 64), bf), env.t("wd", (32, kpad(3, 64)), bf), (8, 8), 32, 3, 1, mask=with_sign(env, "mask", (2, 8, 8, 32), bf),
                             mask_mode=2, flops=1e6)


@case("dgrad_any_bf16")
def _(env):
    bf = env.torch.bfloat16
    return env.cv.dgrad_any_bf16(env.t("dy", (2, 4, 4, 64), bf), env.t("wd", (32, kpad(1, 64)), bf), (8, 8), 32, 1, 2, 0, add=env.t("add", (2, 8, 8, 32), bf),
                                 add_mode=1, flops=1e6)


@variants("s2_classes_bf16/k3", plain={}, split3=dict(mfma=SPLIT3, by_shape=True))
def _(env):
    bf = env.torch.bfloat16
    wc = class_weights(env, env.cv, 3, 1, 32, 64, bf)
    return env.cv.dgrad_s2_classes_bf16(env.t("dy", (2, 4, 4, 64), bf), wc, (8, 7), 32, 3, 1, flops=9e6, add=env.t("add", (2, 8, 7, 32), bf), add_mode=1,
                                        mask=env.t("mask", (2, 8, 7, 32), bf))


@case("s2_classes_bf16/k1")
def _(env):
    bf = env.torch.bfloat16
    wc = class_weights(env, env.cv, 1, 0, 32, 64, bf)
    return env.cv.dgrad_s2_classes_bf16(env.t("dy", (2, 4, 4, 64), bf), wc, (8, 8), 32, 1, 0, flops=1e6)


@case("s2_classes_bf16/empty_class")
def _(env):
    bf = env.torch.bfloat16
    wc = class_weights(env, env.cv, 3, 1, 32, 64, bf)
    return env.cv.dgrad_s2_classes_bf16(env.t("dy", (2, 1, 1, 64), bf), wc, (1, 1), 32, 3, 1, flops=9e6)


# ------------------------------------------------------------------------------------------------------------------ engine.Layer
def layer(env, kind, cin=32, cout=64, k=3, stride=1, bn=True, fwd_mode=None, sign=False, twin16=False, kw_pad=None):
    """A Layer over a bare ConvSpec with this step's weight attributes set by hand (what prepare / adopt would leave).  kind: "fp32" /
    "bf16" / "fp8" (the fp8 engine's layers carry the bf16 backward's weights as well)."""
    t, cv = env.torch, env.cv
    spec = env.arch.ConvSpec("L", cin, cout, k, stride, k // 2, "L.bn" if bn else None, not bn)
    L = env.eng.Layer(spec, kw_pad=kw_pad, bf16=kind != "fp32", fp8=kind == "fp8")
    L.wf = env.t("L.wf", (cout, (k * L.kw_pad * cin + 31) // 32 * 32))
    L.scale = env.t("L.scale", (cout,)) if bn else None
    L.shift = env.t("L.shift", (cout,))
    L.sign = sign
    L.out_scale = 0.5
    if fwd_mode:
        L.fwd_mode = fwd_mode
    dt = t.float32 if kind == "fp32" else t.bfloat16
    if stride == 2 and k > 1:
        wd = class_weights(env, cv, k, k // 2, cin, L.cout_pad, dt, name="L.wd" + ("" if kind == "fp32" else "16"))
    else:
        wd = env.t("L.wd" + ("" if kind == "fp32" else "16"), (cin, kpad(k, L.cout_pad)), dt)
        if twin16:
            twins(env, wd, split=True, split16=True)
    if kind == "fp32":
        L.wd = wd
        if twin16:
            twins(env, L.wf, split=True, split16=True)
    else:
        L.wd16 = wd
        L.wf16 = env.t("L.wf16", (cout, kpad(k, cin)), t.bfloat16)
    if kind == "fp8":
        L.wq = env.t("L.wq", (cout, (kpad(k, cin) + 63) // 64 * 64), t.uint8)
        L.wscale = env.name("L.wscale", t.ones(cout))
        L._fp8_scales = {}
    env.L = L
    return L


def q8(env, name, shape, scale):
    x = env.t(name, shape, env.torch.uint8)
    x._rn_scale = scale
    return x


SPLIT3_F16 = dict(mfma=SPLIT3, wants_f16=1)


@case("layer_fp32/fwd", **SPLIT3_F16)
def _(env):
    L = layer(env, "fp32", sign=True, twin16=True)
    return L.fwd(env.t("x", (2, 8, 8, 32)), act=env.cv.ACT_RELU, add=env.t("add", (2, 8, 8, 64)), add_mode=1)


@case("layer_fp32/fwd_out_stem_products")
def _(env):
    L = layer(env, "fp32", cin=4, k=7, stride=2, sign=True, kw_pad=8)
    L.bf16_products = True
    buf = env.t("ybuf", (2, 2 * 8 * 8 * 64))
    return L.fwd(env.t("x", (2, 16, 16, 4)), act=env.cv.ACT_RELU, out=buf[:, :8 * 8 * 64], y_batch_stride=2 * 8 * 8 * 64, in_relu=True, sign=True)


@case("layer_fp32/fwd_group", **SPLIT3_F16)
def _(env):
    L = layer(env, "fp32", sign=True, twin16=True)
    return L.fwd_group([env.t("x%d" % i, (2, h, w, 32)) for i, (h, w) in enumerate(LEVELS[:3])], act=env.cv.ACT_RELU)


@case("layer_fp32/fwd_group_outs")
def _(env):
    L = layer(env, "fp32", cout=96, bn=False)
    buf = env.t("ybuf", (2, 8 * 8 + 4 * 4, 96))
    return L.fwd_group([env.t("x0", (2, 8, 8, 32)), env.t("x1", (2, 4, 4, 32))], act=env.cv.ACT_SIGMOID, outs=[buf[:, :64], buf[:, 64:]],
                       y_batch_stride=80 * 96)


@case("layer_fp32/bwd_data_group", **SPLIT3_F16)
def _(env):
    L = layer(env, "fp32", twin16=True)
    gs = [env.t("g%d" % i, (2, h, w, 64)) for i, (h, w) in enumerate(LEVELS[:3])]
    masks = [with_sign(env, "m%d" % i, (2, h, w, 32)) for i, (h, w) in enumerate(LEVELS[:3])]
    adds = [env.t("a0", (2, 16, 12, 32)), None, env.t("a2", (2, 2, 2, 32))]
    return L.bwd_data_group(gs, LEVELS[:3], adds=adds, masks=masks)


@case("layer_fp32/bwd_data_group_plain")
def _(env):
    L = layer(env, "fp32", cout=72, bn=False)                   # a padded head-output gradient: 96 channels
    return L.bwd_data_group([env.t("g0", (2, 8, 8, 96)), env.t("g1", (2, 4, 4, 96))], LEVELS[:2])


@case("layer_fp32/bwd_data_stride1")
def _(env):
    L = layer(env, "fp32", twin16=True)
    return L.bwd_data(env.t("g", (2, 8, 8, 64)), (8, 8), add=env.t("add", (2, 8, 8, 32)), mask=with_sign(env, "mask", (2, 8, 8, 32)),
                      add2=env.t("add2", (2, 4, 4, 32)))


@case("layer_fp32/bwd_data_stride2_k3", **SPLIT3_F16)
def _(env):
    L = layer(env, "fp32", stride=2)
    return L.bwd_data(env.t("g", (2, 4, 4, 64)), (8, 8), mask=env.t("mask", (2, 8, 8, 32)), mask_mode=1)


@case("layer_fp32/bwd_data_stride2_k1")
def _(env):
    L = layer(env, "fp32", k=1, stride=2)
    return L.bwd_data(env.t("g", (2, 4, 4, 64)), (8, 8), add=env.t("add", (2, 8, 8, 32)))


@variants("layer_fp32/bwd_params", native=dict(by_shape=True), split3=dict(mfma=SPLIT3), deterministic=dict(options={OPT_DETERMINISTIC: 1}))
def _(env):
    L = layer(env, "fp32")
    L.bwd_params(env.t("g", (2, 8, 8, 64)), env.t("x", (2, 8, 8, 32)), in_relu=True)
    return L.bwd_params(env.t("g2", (2, 4, 4, 64)), env.t("x2", (2, 4, 4, 32)))


@case("layer_fp32/bwd_params_group")
def _(env):
    L = layer(env, "fp32")
    return L.bwd_params_group([env.t("g%d" % i, (2, h, w, 64)) for i, (h, w) in enumerate(LEVELS[:2])],
                              [env.t("x%d" % i, (2, h, w, 32)) for i, (h, w) in enumerate(LEVELS[:2])])


@case("layer_fp32/bwd_fused", by_shape=True, **SPLIT3_F16)
def _(env):
    L = layer(env, "fp32", cin=64, cout=256, k=1, twin16=True)
    return L.bwd_fused(env.t("g", (2, 8, 8, 256)), env.t("x", (2, 8, 8, 64)), mask=with_sign(env, "mask", (2, 8, 8, 64)))


@case("layer_fp32/bwd_data_compact")
def _(env):
    L = layer(env, "fp32", k=1, stride=2)
    return L.bwd_data_compact(env.t("g", (2, 4, 4, 64)))


P8_TILES = dict(tile=256256, tile_rows=256256)


@case("layer_bf16/fwd")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16", sign=True)
    return L.fwd(env.t("x", (2, 8, 8, 32), bf), act=env.cv.ACT_RELU, add=env.t("add", (2, 8, 8, 64), bf), add_mode=1)


@case("layer_bf16/fwd_out_fp32")
def _(env):
    L = layer(env, "bf16", bn=False)
    buf = env.t("ybuf", (2, 2 * 8 * 8 * 64))
    return L.fwd(env.t("x", (2, 8, 8, 32), env.torch.bfloat16), act=env.cv.ACT_SIGMOID, out=buf[:, 8 * 8 * 64:], y_batch_stride=2 * 8 * 8 * 64)


@case("layer_bf16/fwd_group", **P8_TILES)
def _(env):
    L = layer(env, "bf16", sign=True)
    return L.fwd_group([env.t("x%d" % i, (2, h, w, 32), env.torch.bfloat16) for i, (h, w) in enumerate(LEVELS[:3])], act=env.cv.ACT_RELU)


@case("layer_bf16/fwd_group_outs")
def _(env):
    L = layer(env, "bf16", bn=False, sign=True)
    buf = env.t("ybuf", (2, 8 * 8 + 4 * 4, 64))
    return L.fwd_group([env.t("x0", (2, 8, 8, 32), env.torch.bfloat16), env.t("x1", (2, 4, 4, 32), env.torch.bfloat16)], act=env.cv.ACT_SIGMOID,
                       outs=[buf[:, :64], buf[:, 64:]], y_batch_stride=80 * 64)


@case("layer_bf16/bwd_data_group")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16")
    gs = [env.t("g%d" % i, (2, h, w, 64), bf) for i, (h, w) in enumerate(LEVELS[:3])]
    masks = [env.t("m%d" % i, (2, h, w, 32), bf) for i, (h, w) in enumerate(LEVELS[:3])]
    return L.bwd_data_group(gs, LEVELS[:3], adds=[None, env.t("a1", (2, 4, 4, 32), bf), None], masks=masks)


@case("layer_bf16/bwd_data_group_plain")
def _(env):
    L = layer(env, "bf16")
    return L.bwd_data_group([env.t("g0", (2, 8, 8, 64), env.torch.bfloat16)], LEVELS[:1])


@case("layer_bf16/bwd_data_stride1")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16")
    return L.bwd_data(env.t("g", (2, 8, 8, 64), bf), (8, 8), add=env.t("add", (2, 8, 8, 32), bf), mask=env.t("mask", (2, 8, 8, 32), bf))


@case("layer_bf16/bwd_data_stride2_k3")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16", stride=2)
    return L.bwd_data(env.t("g", (2, 4, 4, 64), bf), (8, 8), mask=env.t("mask", (2, 8, 8, 32), bf))


@case("layer_bf16/bwd_data_stride2_k1_compact")
def _(env):
    L = layer(env, "bf16", k=1, stride=2)
    return L.bwd_data(env.t("g", (2, 4, 4, 64), env.torch.bfloat16), (8, 8))


@case("layer_bf16/bwd_data_stride2_k1_compact_add")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16", k=1, stride=2)
    return L.bwd_data(env.t("g", (2, 4, 4, 64), bf), (8, 8), add=env.t("add", (2, 8, 8, 32), bf))


@case("layer_bf16/bwd_data_stride2_k1_masked")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16", k=1, stride=2)
    return L.bwd_data(env.t("g", (2, 4, 4, 64), bf), (8, 8), add=env.t("add", (2, 8, 8, 32), bf), mask=env.t("mask", (2, 8, 8, 32), bf))


@case("layer_bf16/bwd_params", by_shape=True)
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16")
    L.bwd_params(env.t("g", (2, 8, 8, 64), bf), env.t("x", (2, 8, 8, 32), bf))
    return L.bwd_params(env.t("g2", (2, 4, 4, 64), bf), env.t("x2", (2, 4, 4, 32), bf))


@case("layer_bf16/bwd_params_group", by_shape=True)
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16")
    return L.bwd_params_group([env.t("g%d" % i, (2, h, w, 64), bf) for i, (h, w) in enumerate(LEVELS[:3])],
                              [env.t("x%d" % i, (2, h, w, 32), bf) for i, (h, w) in enumerate(LEVELS[:3])])


@case("layer_bf16/bwd_params_group_per_level")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "bf16")
    return L.bwd_params_group([env.t("g0", (2, 8, 8, 64), bf)], [env.t("x0", (2, 8, 8, 32), bf)])


@case("layer_fp8/fwd_two_scales", **P8_TILES)
def _(env):
    L = layer(env, "fp8")
    a = L.fwd(q8(env, "xa", (2, 8, 8, 32), 0.5), act=env.cv.ACT_RELU)
    b = L.fwd(q8(env, "xb", (2, 8, 8, 32), 0.25), act=env.cv.ACT_RELU, add=q8(env, "add", (2, 8, 8, 64), 2.0), add_mode=1)
    c = L.fwd(q8(env, "xc", (2, 4, 4, 32), 0.5))
    return [a, b, c]


@case("layer_fp8/fwd_out_fp32")
def _(env):
    L = layer(env, "fp8", bn=False)
    buf = env.t("ybuf", (2, 2 * 8 * 8 * 64))
    return L.fwd(q8(env, "x", (2, 8, 8, 32), 0.5), act=env.cv.ACT_SIGMOID, out=buf[:, 8 * 8 * 64:], y_batch_stride=2 * 8 * 8 * 64)


@case("layer_fp8/fwd_group")
def _(env):
    L = layer(env, "fp8")
    return L.fwd_group([q8(env, "x%d" % i, (2, h, w, 32), 0.5) for i, (h, w) in enumerate(LEVELS[:3])], act=env.cv.ACT_RELU)


@case("layer_fp8/fwd_group_outs")
def _(env):
    L = layer(env, "fp8", bn=False)
    buf = env.t("ybuf", (2, 8 * 8 + 4 * 4, 64))
    L.fwd(q8(env, "x", (2, 2, 2, 32), 0.5))                      # the scale vector of this input scale exists already
    return L.fwd_group([q8(env, "x0", (2, 8, 8, 32), 0.5), q8(env, "x1", (2, 4, 4, 32), 0.5)], act=env.cv.ACT_SIGMOID, outs=[buf[:, :64], buf[:, 64:]],
                       y_batch_stride=80 * 64)


@case("layer_fp8/fwd_group_scales_differ")
def _(env):
    L = layer(env, "fp8")
    return L.fwd_group([q8(env, "x0", (2, 8, 8, 32), 0.5), q8(env, "x1", (2, 4, 4, 32), 0.25), q8(env, "x2", (2, 2, 2, 32), 0.5)], act=env.cv.ACT_RELU)


@case("layer_fp8/fwd_group_scales_differ_outs")
def _(env):
    L = layer(env, "fp8", bn=False)
    buf = env.t("ybuf", (2, 8 * 8 + 4 * 4, 64))
    return L.fwd_group([q8(env, "x0", (2, 8, 8, 32), 0.5), q8(env, "x1", (2, 4, 4, 32), 0.25)], outs=[buf[:, :64], buf[:, 64:]], y_batch_stride=80 * 64)


@case("layer_fp8_as_bf16/fwd")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "fp8", fwd_mode="bf16", sign=True)
    return L.fwd(env.t("x", (2, 8, 8, 32), bf), act=env.cv.ACT_RELU, add=env.t("add", (2, 8, 8, 64), bf), add_mode=1)


@case("layer_fp8_as_bf16/fwd_group")
def _(env):
    L = layer(env, "fp8", fwd_mode="bf16", sign=True)
    return L.fwd_group([env.t("x%d" % i, (2, h, w, 32), env.torch.bfloat16) for i, (h, w) in enumerate(LEVELS[:2])], act=env.cv.ACT_RELU)


@case("layer_fp8/bwd_data_group")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "fp8")
    return L.bwd_data_group([env.t("g%d" % i, (2, h, w, 64), bf) for i, (h, w) in enumerate(LEVELS[:2])], LEVELS[:2])


@case("layer_fp8/bwd_params_and_data")
def _(env):
    bf = env.torch.bfloat16
    L = layer(env, "fp8")
    L.bwd_params(env.t("g", (2, 8, 8, 64), bf), env.t("x", (2, 8, 8, 32), bf))
    return L.bwd_data(env.T["g"], (8, 8), mask=env.t("mask", (2, 8, 8, 32), bf))



# The Winograd wrappers themselves are not this table's subject; these cases reach the branches of Layer that hand over to them.
def wino_layer(env, **kw):
    L = layer(env, "fp32", cin=64, cout=128, **kw)
    L.uf, L.ud = env.t("L.uf", (36, 128, 64)), env.t("L.ud", (36, 64, 128))
    return L


@case("layer_wino/fwd_bwd", **SPLIT3_F16)
def _(env):
    L = wino_layer(env, sign=True)
    L.wino_active = True
    x = env.t("x", (2, 8, 8, 64))
    y = L.fwd(x, act=env.cv.ACT_RELU)
    g = env.t("g", (2, 8, 8, 128))
    L.bwd_params(g, x)
    return [y, L.bwd_data(g, (8, 8), add=env.t("add", (2, 8, 8, 64)), mask=with_sign(env, "mask", (2, 8, 8, 64)))]


@case("layer_wino/group_fwd_bwd")
def _(env):
    L = wino_layer(env, sign=True)
    xs = [env.t("x%d" % i, (2, h, w, 64)) for i, (h, w) in enumerate(LEVELS[:2])]
    gs = [env.t("g%d" % i, (2, h, w, 128)) for i, (h, w) in enumerate(LEVELS[:2])]
    ys = L.fwd_group(xs, act=env.cv.ACT_RELU, wino=True)
    L.bwd_params_group(gs, xs, wino=True)
    return ys + L.bwd_data_group(gs, LEVELS[:2], wino=True)


# ------------------------------------------------------------------------------------------------------------------ wino_conv_group / wino_wgrad_group
# ... called directly: every Winograd entry point, its list and flag forms, and a group of more than RN_MAX_GROUP problems (two launches,
# the second at a tile offset).  Records made on the wrappers before their transform helpers were folded.
WINO_LEVELS = LEVELS + [(5, 3)]
OPT_WGRAD_ONCE = 4
WINO_SPLIT3 = dict(mfma=SPLIT3, wants_f16=1, options={OPT_WGRAD_ONCE: 1})


def wino_xs(env, n, c, prefix="x"):
    return [env.t("%s%d" % (prefix, i), (2, h, w, c)) for i, (h, w) in enumerate(WINO_LEVELS[:n])]


def wino_shapes(ts):
    return tuple(tuple(t.shape) for t in ts)


def wino_lists(env, name, tpad=256):
    """The TileLists of a named flag array, built in a named buffer (the rn_tile_lists call is part of the record)."""
    i32 = env.torch.int32
    return env.cv.tile_lists(env.t(name, (tpad,), env.torch.uint8), tpad, buf=env.t(name + "_lists", (env.cv.tile_lists_numel(tpad),), i32))


@variants("wino/conv_six_problems", native={}, split3=WINO_SPLIT3, by_shape=dict(by_shape=True))
def _(env):
    xs = wino_xs(env, 6, 32)
    return env.cv.wino_conv_group(xs, env.t("U", (36, 64, 32)), scale=env.t("scale", (64,)), shift=env.t("shift", (64,)), act=env.cv.ACT_RELU, sign=True)


@variants("wino/conv_six_problems_ybs_add_mask", native={}, split3=WINO_SPLIT3)
def _(env):
    xs = wino_xs(env, 6, 32)
    rows = sum(h * w for h, w in WINO_LEVELS)
    buf, outs, r0 = env.t("ybuf", (2, rows, 64)), [], 0
    for h, w in WINO_LEVELS:
        outs.append(buf[:, r0:r0 + h * w])
        r0 += h * w
    adds = [env.t("add%d" % i, (2, h, w, 64)) for i, (h, w) in enumerate(WINO_LEVELS)]
    masks = [with_sign(env, "mask%d" % i, (2, h, w, 64)) for i, (h, w) in enumerate(WINO_LEVELS[:5])] + [env.t("mask5", (2, 5, 3, 64))]
    return env.cv.wino_conv_group(xs, env.t("U", (36, 64, 32)), outs=outs, adds=adds, masks=masks, mask_mode=1, y_batch_stride=rows * 64, sign=True)


@variants("wino/wgrad_six_problems", native={}, split3=WINO_SPLIT3, deterministic=dict(options={OPT_DETERMINISTIC: 1}))
def _(env):
    xs, gs = wino_xs(env, 6, 32), wino_xs(env, 6, 64, "g")
    return env.cv.wino_wgrad_group(gs, xs, env.t("dw", (64, kpad(3, 32))), env.t("colsum", (64,)))


def wino_need(need_in):
    def fn(env):
        xs = wino_xs(env, 2, 32)
        need = wino_lists(env, "need")
        nin = {"same": None, "dense": env.cv.DENSE}[need_in] if need_in != "own" else wino_lists(env, "need_in")
        outs, kept = env.cv.wino_conv_group(xs, env.t("U", (36, 64, 32)), shift=env.t("shift", (64,)), act=env.cv.ACT_RELU, keep_v=True, sign=True,
                                            need=need, need_in=nin, need_fill="zero")
        return outs + [kept[0]] + [w for w in kept[2] if w is not None]
    return fn


variants("wino/conv_need", native={}, split3=WINO_SPLIT3)(wino_need("same"))
case("wino/conv_need_in_own", **WINO_SPLIT3)(wino_need("own"))
variants("wino/conv_need_in_dense", native={}, split3=WINO_SPLIT3)(wino_need("dense"))


@case("wino/conv_need_workspace_v")
def _(env):
    """Without keep_v: V in the shared workspace, nothing filled."""
    return env.cv.wino_conv_group(wino_xs(env, 2, 32), env.t("U", (36, 64, 32)), need=wino_lists(env, "need"))


@variants("wino/conv_flags_out", native={}, split3=WINO_SPLIT3)
def _(env):
    xs = wino_xs(env, 2, 32)
    adds = [env.t("add%d" % i, (2, h, w, 64)) for i, (h, w) in enumerate(WINO_LEVELS[:2])]
    masks = [with_sign(env, "mask%d" % i, (2, h, w, 64)) for i, (h, w) in enumerate(WINO_LEVELS[:2])]
    return env.cv.wino_conv_group(xs, env.t("U", (36, 64, 32)), adds=adds, masks=masks, flags_out=env.t("flags_out", (256,), env.torch.uint8))


def wino_v_ready(with_lists):
    def fn(env):
        gs = wino_xs(env, 2, 128, "g")
        lists = wino_lists(env, "flags")
        ready = (env.t("Vd", (36 * 256 * 128,)), wino_shapes(gs), (env.t("rows", (256,), env.torch.int32), None), lists.flags) + ((lists,) if with_lists else ())
        masks = [env.t("mask%d" % i, (2, h, w, 96)) for i, (h, w) in enumerate(WINO_LEVELS[:2])]
        return env.cv.wino_conv_group(gs, env.t("U", (36, 96, 128)), masks=masks, V_ready=ready, flags_out=env.t("flags_out", (256,), env.torch.uint8))
    return fn


case("wino/conv_v_ready_flags", **WINO_SPLIT3)(wino_v_ready(False))
case("wino/conv_v_ready_lists", **WINO_SPLIT3)(wino_v_ready(True))


def wino_wgrad_fused(lists):
    def fn(env):
        i32 = env.torch.int32
        xs, gs = wino_xs(env, 2, 96), wino_xs(env, 2, 128, "g")
        kept = (env.t("V", (36 * 256 * 96,)), wino_shapes(xs), (None, env.t("v_word", (1,), i32)))
        flags = env.t("flags", (256,), env.torch.uint8)
        how = {"none": None, "here": True, "buffer": env.t("list_buf", (env.cv.tile_lists_numel(256),), i32) if lists == "buffer" else None}[lists]
        v_dy = env.cv.wino_wgrad_group(gs, xs, env.t("dw", (128, kpad(3, 96))), env.t("colsum", (128,)), V=kept, fuse_dgrad_input=True, flags=flags, lists=how)
        return [v_dy[0]] + [w for w in v_dy[2] if w is not None] + [t if isinstance(t, env.torch.Tensor) else t.buf for t in v_dy[3:]]
    return fn


variants("wino/wgrad_fused_flags", split3=WINO_SPLIT3, native_runs_dense=dict(options={OPT_WGRAD_ONCE: 1}), no_once_runs_dense=dict(mfma=SPLIT3, wants_f16=1))(
    wino_wgrad_fused("none"))
variants("wino/wgrad_fused_lists", built_here=WINO_SPLIT3, native_runs_dense=dict(options={OPT_WGRAD_ONCE: 1}))(wino_wgrad_fused("here"))
case("wino/wgrad_fused_lists_buffer", **WINO_SPLIT3)(wino_wgrad_fused("buffer"))


EXPECTED = {
    'igemm/plain/native': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', 'scale',
        'shift', None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/plain/split3': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0, None, None,
        'y._rn_amax'), 'x', 'w', 'y', 'scale', 'shift', None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_amax': 128}}},
    'igemm/plain/by_shape': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y',
        'scale', 'shift', None, None, None, 'stream'], ('conv_igemm_4x1 2x8x8 32->64 k3 a1 b1 ds0', 1000000.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/plain/no_timer': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y',
        'scale', 'shift', None, None, None, 'stream'], None)], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/wide_in_relu_kind': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 96, 3, 3, 1, 1, -1, -2, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 6144), 'x', 'w', 'y',
        None, 'shift', None, None, None, 'stream'], ('conv_igemm_2x2 2x8x8 32->96 k3 a1 b1 ds0', 2000000.0, 176128.0))], 'returned': ('torch.float32', (2, 8, 8, 96), 'y'), 'carried': {}},
    'igemm/kind_given': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', None, None,
        None, None, None, 'stream'], ('stem 2x8x8 32->64 k3 a1 b1 ds0', 0.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/add_mode1': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096), 'x', 'w', 'y',
        'scale', None, 'add', None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 155648.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/add_mode1_add_batch_stride': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 8192), 'x',
        'w', 'y', None, None, 'add', None, None, 'stream'], ('conv_igemm_4x1', 0.0, 155648.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/add_mode2': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 2, 4, 4, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 1024), 'x', 'w', 'y', None,
        None, 'add', None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 155648.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/mask_fp32': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 2, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', None, None,
        None, 'mask', None, 'stream'], ('conv_igemm_4x1', 1000000.0, 155648.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/mask_fp32_mode1': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096), 'x', 'w', 'y',
        None, None, 'add', 'mask', None, 'stream'], ('conv_igemm_4x1', 0.0, 188416.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/mask_bits': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 6, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', None, None,
        None, 'mask._rn_sign', None, 'stream'], ('conv_igemm_4x1', 1000000.0, 123904.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {'mask': {'_rn_sign': 256}}},
    'igemm/sign': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0, 'y._rn_sign', None,
        'y._rn_amax'), 'x', 'w', 'y', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 123904.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_sign': 256, '_rn_amax': 128}}},
    'igemm/sign_no_words': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 48, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 3072), 'x', 'w', 'y', None,
        None, None, None, None, 'stream'], ('conv_igemm_4x1', 0.0, 96256.0))], 'returned': ('torch.float32', (2, 8, 8, 48), 'y'), 'carried': {}},
    'igemm/reused_destination': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0, None,
        None, 'y._rn_amax'), 'x', 'w', 'y', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 0.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_amax': 128}}},
    'igemm/out_map': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 2, 1, 0, 16, 16, 0, 0, 0, 0, 2048, 16384), 'x', 'w', 'y16', None,
        None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 122880.0))], 'returned': ('torch.float32', (2, 16, 16, 64), 'y16'), 'carried': {}},
    'igemm/out_map_shared_amax': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 1, 16, 16, 0, 0, 0, 0, 2048, 16384, 0, 0, 0, None,
        None, 'slot'), 'x', 'w', 'y16', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 0.0, 122880.0))], 'returned': ('torch.float32', (2, 16, 16, 64), 'y16'), 'carried': {}},
    'igemm/add2': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 2, 0, 1, 0, 0, 8, 8, 3, 4, 4, 1024, 2048, 4096), 'x', 'w', 'y', None, None,
        None, 'mask', 'add2', 'stream'], ('conv_igemm_4x1', 1000000.0, 163840.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/y_batch_stride': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 12288, 12288), 'x', 'w',
        'ybuf+16384', None, None, 'add', None, None, 'stream'], ('conv_igemm_4x1', 0.0, 155648.0))], 'returned': ('torch.float32', (2, 8192), 'ret'), 'carried': {}},
    'igemm/wino_stage/native': {'calls': [('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048, 0,
        None, None, None, None, 0, 0, 'flags', 'blocks', 'counts+8', 3), 'V', 'U', 'M', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3000000.0, 3833856.0))],
        'returned': ('torch.float32', (36, 1, 256, 64), 'M'), 'carried': {}},
    'igemm/wino_stage/split3_f16': {'calls': [('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048,
        3, None, 'rows', None, 'U._rn_split16[1]', 0, 1, 'flags', 'blocks', 'counts+8', 3), 'V', 'U._rn_split16[0]', 'M', None, None, None, None, None, 'stream'],
        ('conv_igemm_4x1 36x1x256 32->64 k1 a1 b1 ds0 x36', 3000000.0, 3833856.0))], 'returned': ('torch.float32', (36, 1, 256, 64), 'M'), 'carried': {}},
    'igemm/wino_stage/split3_three_term': {'calls': [('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0,
        2048, 1, None, None, None, None, 0, 0, 'flags', 'blocks', 'counts+8', 3), 'V', 'U._rn_split', 'M', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3000000.0,
        3981312.0))], 'returned': ('torch.float32', (36, 1, 256, 64), 'M'), 'carried': {}},
    'igemm/bf16_products': {'calls': [('rn_amax', ['x', 2048, 2, 'x._rn_amax', 'stream'], None), ('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1,
        0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 2, None, 'x._rn_amax', 'y._rn_amax', 'w._rn_split16[1]', 1), 'x', 'w._rn_split', 'y', None, None, None, None, None, 'stream'],
        ('conv_igemm_4x1', 1000000.0, 159744.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {'x': {'_rn_amax': 128}, 'y': {'_rn_amax': 128}}},
    'igemm/bf16_products_twin_made': {'calls': [('rn_split_weights', ['w', 'w._rn_split', 64, 288, 'stream'], None), ('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1,
        0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 2, 'y._rn_sign'), 'x', 'w._rn_split', 'y', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 0.0, 160768.0))],
        'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_sign': 256}}},
    'igemm/splitk/native': {'calls': [('rn_conv_igemm_splitk', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 6, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096, 0, 0,
        'y._rn_sign'), 'x', 'w', 'y', 'scale', 'shift', 'add', 'mask._rn_sign', None, 'other', 'stream'], ('conv_igemm_4x1 2x8x8 32->64 k3 a1 b1 ds0', 1000000.0, 0.0))],
        'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_sign': 256}, 'mask': {'_rn_sign': 256}}},
    'igemm/splitk/split3': {'calls': [('rn_conv_igemm_splitk', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 6, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096, 0, 0,
        'y._rn_sign', None, 'y._rn_amax'), 'x', 'w', 'y', 'scale', 'shift', 'add', 'mask._rn_sign', None, 'other', 'stream'], ('conv_igemm_4x1', 1000000.0, 0.0))],
        'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_sign': 256, '_rn_amax': 128}, 'mask': {'_rn_sign': 256}}},
    'igemm/splitk_shared_amax/split3': {'calls': [('rn_conv_igemm_splitk', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0,
        0, None, None, 'slot'), 'x', 'w', 'y', None, None, None, None, None, 'other', 'stream'], ('conv_igemm_4x1', 0.0, 0.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'),
        'carried': {}},
    'igemm/w_format/native_twins': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y',
        None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/w_format/split_twin': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 1), 'x',
        'w._rn_split', 'y', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 159744.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'igemm/w_format/split3_f16': {'calls': [('rn_amax', ['x', 2048, 2, 'x._rn_amax', 'stream'], None), ('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0,
        0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 3, None, 'x._rn_amax', 'y._rn_amax', 'w._rn_split16[1]', 1), 'x', 'w._rn_split16[0]', 'y', None, None, None, None, None, 'stream'],
        ('conv_igemm_4x1', 1000000.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {'x': {'_rn_amax': 128}, 'y': {'_rn_amax': 128}}},
    'igemm/w_format/split3_refused': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 1, None,
        None, 'y._rn_amax'), 'x', 'w._rn_split', 'y', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 159744.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_amax': 128}}},
    'igemm/w_format_no_twin': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0, None, None,
        'y._rn_amax'), 'x', 'w', 'y', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 122880.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_amax': 128}}},
    'igemm/w_format3_x_amax/words_given': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 2, 0, 1, 0, 0, 8, 8, 3, 4, 4, 1024, 2048, 4096, 0, 0,
        3, 'y._rn_sign', 'xam', 'y._rn_amax', 'w._rn_split16[1]', 1), 'x', 'w._rn_split16[0]', 'y', None, None, None, 'mask', 'add2', 'stream'], ('conv_igemm_4x1', 1000000.0, 164864.0))],
        'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_sign': 256, '_rn_amax': 128}}},
    'bf16/plain/p8_persistent': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0,
        'y._rn_sign'), 'x', 'w', 'y', 0, 'scale', 'shift', None, None, 'stream'], ('conv_igemm_bf16_p8', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_sign': 256}}},
    'bf16/plain/p8_off': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0,
        'y._rn_sign'), 'x', 'w', 'y', 0, 'scale', 'shift', None, None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_sign': 256}}},
    'bf16/plain/p8_single': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0,
        'y._rn_sign'), 'x', 'w', 'y', 0, 'scale', 'shift', None, None, 'stream'], ('conv_igemm_bf16 2x8x8 32->64 k3 a1 b1 ds0', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8,
        64), 'y'), 'carried': {'y': {'_rn_sign': 256}}},
    'bf16/plain/no_timer': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 0, 0, 0,
        'y._rn_sign'), 'x', 'w', 'y', 0, 'scale', 'shift', None, None, 'stream'], None)], 'returned': ('torch.bfloat16', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_sign': 256}}},
    'bf16/fp32_result': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', 1,
        None, 'shift', None, None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'bf16/add_mask': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096), 'x', 'w', 'y', 0,
        None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16', 0.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 64), 'y'), 'carried': {}},
    'bf16/add_mode2_mask_bits': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 2, 4, 4, 6, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 1024), 'x',
        'w', 'y', 0, None, None, 'add', 'mask._rn_sign', 'stream'], ('conv_igemm_bf16', 0.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 64), 'y'),
        'carried': {'mask': {'_rn_sign': 256}}},
    'bf16/out_map': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 0, 0, 2, 0, 0, 16, 16, 0, 0, 0, 0, 2048, 16384, 16384), 'x', 'w',
        'y16', 0, None, None, 'y16', None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 16, 16, 64), 'y16'), 'carried': {}},
    'fp8/plain/p8_off': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', 0,
        'scale', 'shift', None, 1.0, 4.0, 'stream'], ('conv_igemm_fp8', 1000000.0, 0.0))], 'returned': ('torch.uint8', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_scale': 0.25}}},
    'fp8/plain/p8_single': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', 0,
        'scale', 'shift', None, 1.0, 4.0, 'stream'], ('conv_igemm_fp8_p8 2x8x8 32->64 k3', 1000000.0, 0.0))], 'returned': ('torch.uint8', (2, 8, 8, 64), 'y'),
        'carried': {'y': {'_rn_scale': 0.25}}},
    'fp8/plain/no_timer': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', 0,
        'scale', 'shift', None, 1.0, 4.0, 'stream'], None)], 'returned': ('torch.uint8', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_scale': 0.25}}},
    'fp8/fp32_result': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'y', 1,
        'scale', None, None, 1.0, 4.0, 'stream'], ('conv_igemm_fp8_p8', 1000000.0, 0.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'y'), 'carried': {}},
    'fp8/add': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096), 'x', 'w', 'y', 0,
        'scale', 'shift', 'add', 0.125, 2.0, 'stream'], ('conv_igemm_fp8', 1000000.0, 0.0))], 'returned': ('torch.uint8', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_scale': 0.5},
        'add': {'_rn_scale': 0.125}}},
    'fp8/add_mode2': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 2, 4, 4, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 1024), 'x', 'w', 'y', 0,
        'scale', None, 'add', 2.0, 1.0, 'stream'], ('conv_igemm_fp8', 0.0, 0.0))], 'returned': ('torch.uint8', (2, 8, 8, 64), 'y'), 'carried': {'y': {'_rn_scale': 1.0},
        'add': {'_rn_scale': 2.0}}},
    'grouped/n1_cout64': {'calls': [('rn_conv_igemm_grouped', [{'n': 1, 'tile_end': [2], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 16, 12, 0,
        0, 0, 0, 6144, 12288, 0, 0, 0, 'y0._rn_sign')], 'x': ['x0'], 'y': ['y0']}, 'w', 'scale', 'shift', 'stream'], ('conv_igemm_4x1', 5000000.0, 221184.0))], 'returned': None,
        'carried': {'y0': {'_rn_sign': 768}}},
    'grouped/n1_cout128': {'calls': [('rn_conv_igemm_grouped', [{'n': 1, 'tile_end': [3], 'd': [('D', 2, 16, 12, 32, 16, 12, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 16, 12, 0,
        0, 0, 0, 6144, 24576, 0, 0, 0, 'y0._rn_sign', None, 'y0._rn_amax')], 'x': ['x0'], 'y': ['y0']}, 'w', 'scale', 'shift', 'stream'], ('conv_igemm_2x2', 5000000.0, 393216.0))],
        'returned': None, 'carried': {'y0': {'_rn_sign': 1536, '_rn_amax': 128}}},
    'grouped/n3_cout64': {'calls': [('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_amax', ['x2', 128, 2,
        'x2._rn_amax', 'stream'], None), ('rn_conv_igemm_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288, 0, 0, 3, 'y0._rn_sign', 'x0._rn_amax', 'y0._rn_amax', 'w._rn_split16[1]', 1), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0,
        1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024, 0, 0, 3, 'y1._rn_sign', 'x1._rn_amax', 'y1._rn_amax', 'w._rn_split16[1]', 1), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0,
        0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256, 0, 0, 3, 'y2._rn_sign', 'x2._rn_amax', 'y2._rn_amax', 'w._rn_split16[1]', 1)], 'x': ['x0', 'x1', 'x2'], 'y': ['y0', 'y1', 'y2']},
        'w._rn_split16[0]', 'scale', 'shift', 'stream'], ('conv_igemm_4x1', 5000000.0, 236544.0))], 'returned': None, 'carried': {'x0': {'_rn_amax': 128}, 'y0': {'_rn_sign': 768,
        '_rn_amax': 128}, 'x1': {'_rn_amax': 128}, 'y1': {'_rn_sign': 64, '_rn_amax': 128}, 'x2': {'_rn_amax': 128}, 'y2': {'_rn_sign': 16, '_rn_amax': 128}}},
    'grouped/n3_cout128': {'calls': [('rn_conv_igemm_grouped', [{'n': 3, 'tile_end': [3, 4, 5], 'd': [('D', 2, 16, 12, 32, 16, 12, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 16,
        12, 0, 0, 0, 0, 6144, 24576, 0, 0, 0, 'y0._rn_sign'), ('D', 2, 4, 4, 32, 4, 4, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 2048, 0, 0, 0,
        'y1._rn_sign'), ('D', 2, 2, 2, 32, 2, 2, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 512, 0, 0, 0, 'y2._rn_sign')], 'x': ['x0', 'x1', 'x2'],
        'y': ['y0', 'y1', 'y2']}, 'w', 'scale', 'shift', 'stream'], ('conv_igemm_2x2 grouped 32->128 k3', 5000000.0, 418816.0))], 'returned': None, 'carried': {'y0': {'_rn_sign': 1536},
        'y1': {'_rn_sign': 128}, 'y2': {'_rn_sign': 32}}},
    'grouped/n5_cout64': {'calls': [('rn_conv_igemm_grouped', [{'n': 5, 'tile_end': [2, 3, 4, 5, 6], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1,
        1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256), ('D', 2, 1, 1, 32, 1, 1, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 32, 64), ('D',
        2, 3, 5, 32, 3, 5, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 3, 5, 0, 0, 0, 0, 480, 960)], 'x': ['x0', 'x1', 'x2', 'x3', 'x4'], 'y': ['y0', 'y1', 'y2', 'y3', 'y4']}, 'w',
        'scale', 'shift', 'stream'], None)], 'returned': None, 'carried': {}},
    'grouped/n5_cout128': {'calls': [('rn_conv_igemm_grouped', [{'n': 5, 'tile_end': [3, 4, 5, 6, 7], 'd': [('D', 2, 16, 12, 32, 16, 12, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 6144, 24576, 0, 0, 0, None, None, 'y0._rn_amax'), ('D', 2, 4, 4, 32, 4, 4, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 2048,
        0, 0, 0, None, None, 'y1._rn_amax'), ('D', 2, 2, 2, 32, 2, 2, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 512, 0, 0, 0, None, None, 'y2._rn_amax'),
        ('D', 2, 1, 1, 32, 1, 1, 128, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 32, 128, 0, 0, 0, None, None, 'y3._rn_amax'), ('D', 2, 3, 5, 32, 3, 5, 128, 3, 3, 1,
        1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 3, 5, 0, 0, 0, 0, 480, 1920, 0, 0, 0, None, None, 'y4._rn_amax')], 'x': ['x0', 'x1', 'x2', 'x3', 'x4'], 'y': ['y0', 'y1', 'y2', 'y3', 'y4']},
        'w', 'scale', 'shift', 'stream'], ('conv_igemm_2x2', 5000000.0, 439296.0))], 'returned': None, 'carried': {'y0': {'_rn_amax': 128}, 'y1': {'_rn_amax': 128}, 'y2': {'_rn_amax': 128},
        'y3': {'_rn_amax': 128}, 'y4': {'_rn_amax': 128}}},
    'grouped/ybs_add_mask/split': {'calls': [('rn_conv_igemm_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 6144, 13568, 13568, 0, 1), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 13568, 13568, 0, 1), ('D', 2,
        2, 2, 32, 2, 2, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 13568, 13568, 0, 1)], 'x': ['x0', 'x1', 'x2'], 'y': ['ybuf', 'ybuf+49152', 'ybuf+53248'],
        'add': ['add0', 'add1', 'add2'], 'mask': ['mask0._rn_sign', 'mask1', 'mask2._rn_sign']}, 'w._rn_split', 'scale', 'shift', 'stream'], ('conv_igemm_4x1', 5000000.0, 490496.0))],
        'returned': None, 'carried': {'mask0': {'_rn_sign': 768}, 'mask2': {'_rn_sign': 16}}},
    'grouped/ybs_add_mask/split3': {'calls': [('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_amax', ['x2', 128,
        2, 'x2._rn_amax', 'stream'], None), ('rn_conv_igemm_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 6144, 13568, 13568, 0, 3, None, 'x0._rn_amax', None, 'w._rn_split16[1]', 1), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 4,
        4, 0, 0, 0, 0, 512, 13568, 13568, 0, 3, None, 'x1._rn_amax', None, 'w._rn_split16[1]', 1), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0, 0, 2, 2, 0, 0,
        0, 0, 128, 13568, 13568, 0, 3, None, 'x2._rn_amax', None, 'w._rn_split16[1]', 1)], 'x': ['x0', 'x1', 'x2'], 'y': ['ybuf', 'ybuf+49152', 'ybuf+53248'], 'add': ['add0', 'add1',
        'add2'], 'mask': ['mask0._rn_sign', 'mask1', 'mask2._rn_sign']}, 'w._rn_split16[0]', 'scale', 'shift', 'stream'], ('conv_igemm_4x1', 5000000.0, 453632.0))], 'returned': None,
        'carried': {'x0': {'_rn_amax': 128}, 'mask0': {'_rn_sign': 768}, 'x1': {'_rn_amax': 128}, 'x2': {'_rn_amax': 128}, 'mask2': {'_rn_sign': 16}}},
    'grouped/add_mask_bits': {'calls': [('rn_conv_igemm_grouped', [{'n': 2, 'tile_end': [3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 128, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0, 0, 16,
        12, 0, 0, 0, 0, 6144, 24576, 24576, 0, 0, 'y0._rn_sign'), ('D', 2, 4, 4, 32, 4, 4, 128, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 2048, 2048, 0, 0,
        'y1._rn_sign')], 'x': ['x0', 'x1'], 'y': ['y0', 'y1'], 'add': ['add0', 'add1'], 'mask': ['mask0._rn_sign', 'mask1._rn_sign']}, 'w', 'scale', 'shift', 'stream'], ('conv_igemm_2x2',
        5000000.0, 839680.0))], 'returned': None, 'carried': {'y0': {'_rn_sign': 1536}, 'mask0': {'_rn_sign': 1536}, 'y1': {'_rn_sign': 128}, 'mask1': {'_rn_sign': 128}}},
    'grouped/no_twin': {'calls': [('rn_conv_igemm_grouped', [{'n': 2, 'tile_end': [2, 3], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 2, 0, 1, 0, 0, 16, 12, 0,
        0, 0, 0, 6144, 12288, 12288, 0, 0, None, None, 'y0._rn_amax'), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 2, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024, 1024, 0, 0,
        None, None, 'y1._rn_amax')], 'x': ['x0', 'x1'], 'y': ['y0', 'y1'], 'add': ['add0', 'add1'], 'mask': ['mask0', 'mask1']}, 'w', 'scale', 'shift', 'stream'], ('conv_igemm_4x1',
        5000000.0, 446464.0))], 'returned': None, 'carried': {'y0': {'_rn_amax': 128}, 'y1': {'_rn_amax': 128}}},
    'grouped_bf16/n1/t128': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 1, 'tile_end': [3], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 16,
        12, 0, 0, 0, 0, 6144, 12288, 0, 0, 0, 'y0._rn_sign')], 'x': ['x0'], 'y': ['y0']}, 'w', 0, 'scale', 'shift', 'stream'], ('conv_igemm_bf16', 5000000.0, 0.0))], 'returned': None,
        'carried': {'y0': {'_rn_sign': 768}}},
    'grouped_bf16/n1/no_timer': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 1, 'tile_end': [3], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288, 0, 0, 0, 'y0._rn_sign')], 'x': ['x0'], 'y': ['y0']}, 'w', 0, 'scale', 'shift', 'stream'], None)], 'returned': None,
        'carried': {'y0': {'_rn_sign': 768}}},
    'grouped_bf16/n3/t128': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 3, 'tile_end': [3, 4, 5], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 6144, 12288), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3,
        1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256)], 'x': ['x0', 'x1', 'x2'], 'y': ['y0', 'y1', 'y2']}, 'w', 0, 'scale', 'shift', 'stream'], ('conv_igemm_bf16',
        5000000.0, 0.0))], 'returned': None, 'carried': {}},
    'grouped_bf16/n3/t256': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 6144, 12288), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3,
        1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256)], 'x': ['x0', 'x1', 'x2'], 'y': ['y0', 'y1', 'y2']}, 'w', 0, 'scale', 'shift', 'stream'],
        ('conv_igemm_bf16_p8 grouped 32->64 k3', 5000000.0, 0.0))], 'returned': None, 'carried': {}},
    'grouped_bf16/n5/t256': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 5, 'tile_end': [2, 3, 4, 5, 6], 'd': [('D', 2, 16, 12, 32, 16, 12, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0,
        1, 0, 0, 16, 12, 0, 0, 0, 0, 6144, 30720, 0, 0, 0, 'y0._rn_sign'), ('D', 2, 4, 4, 32, 4, 4, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 2560, 0, 0,
        0, 'y1._rn_sign'), ('D', 2, 2, 2, 32, 2, 2, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 640, 0, 0, 0, 'y2._rn_sign'), ('D', 2, 1, 1, 32, 1, 1, 160,
        3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 32, 160, 0, 0, 0, 'y3._rn_sign'), ('D', 2, 3, 5, 32, 3, 5, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        3, 5, 0, 0, 0, 0, 480, 2400, 0, 0, 0, 'y4._rn_sign')], 'x': ['x0', 'x1', 'x2', 'x3', 'x4'], 'y': ['y0', 'y1', 'y2', 'y3', 'y4']}, 'w', 0, 'scale', 'shift', 'stream'],
        ('conv_igemm_bf16_p8', 5000000.0, 0.0))], 'returned': None, 'carried': {'y0': {'_rn_sign': 1920}, 'y1': {'_rn_sign': 160}, 'y2': {'_rn_sign': 40}, 'y3': {'_rn_sign': 10},
        'y4': {'_rn_sign': 150}}},
    'grouped_bf16/n5/t256x128': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 5, 'tile_end': [4, 6, 8, 10, 12], 'd': [('D', 2, 16, 12, 32, 16, 12, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0,
        0, 0, 1, 0, 0, 16, 12, 0, 0, 0, 0, 6144, 30720, 0, 0, 0, 'y0._rn_sign'), ('D', 2, 4, 4, 32, 4, 4, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 2560,
        0, 0, 0, 'y1._rn_sign'), ('D', 2, 2, 2, 32, 2, 2, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 640, 0, 0, 0, 'y2._rn_sign'), ('D', 2, 1, 1, 32, 1, 1,
        160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 32, 160, 0, 0, 0, 'y3._rn_sign'), ('D', 2, 3, 5, 32, 3, 5, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1,
        0, 0, 3, 5, 0, 0, 0, 0, 480, 2400, 0, 0, 0, 'y4._rn_sign')], 'x': ['x0', 'x1', 'x2', 'x3', 'x4'], 'y': ['y0', 'y1', 'y2', 'y3', 'y4']}, 'w', 0, 'scale', 'shift', 'stream'],
        ('conv_igemm_bf16', 5000000.0, 0.0))], 'returned': None, 'carried': {'y0': {'_rn_sign': 1920}, 'y1': {'_rn_sign': 160}, 'y2': {'_rn_sign': 40}, 'y3': {'_rn_sign': 10},
        'y4': {'_rn_sign': 150}}},
    'grouped_bf16/fp32_results': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 3, 'tile_end': [3, 4, 5], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 6144, 13568), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 13568), ('D', 2, 2, 2, 32, 2, 2, 64, 3,
        3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 13568)], 'x': ['x0', 'x1', 'x2'], 'y': ['ybuf', 'ybuf+49152', 'ybuf+53248']}, 'w', 1, 'scale', 'shift',
        'stream'], ('conv_igemm_bf16', 5000000.0, 0.0))], 'returned': None, 'carried': {}},
    'grouped_bf16/ybs_add_mask': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 6144, 13568, 13568), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 13568, 13568), ('D', 2, 2, 2, 32,
        2, 2, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 13568, 13568)], 'x': ['x0', 'x1', 'x2'], 'y': ['ybuf', 'ybuf+24576', 'ybuf+26624'], 'add': ['add0',
        'add1', 'add2'], 'mask': ['mask0._rn_sign', 'mask1', 'mask2._rn_sign']}, 'w', 0, 'scale', 'shift', 'stream'], ('conv_igemm_bf16_p8', 5000000.0, 0.0))], 'returned': None,
        'carried': {'mask0': {'_rn_sign': 768}, 'mask2': {'_rn_sign': 16}}},
    'grouped_fp8/n1/t128': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 1, 'tile_end': [3], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 16,
        12, 0, 0, 0, 0, 6144, 12288)], 'x': ['x0'], 'y': ['y0']}, 'w', 0, 'scale', 'shift', 1.0, 4.0, 'stream'], ('conv_igemm_fp8', 5000000.0, 0.0))], 'returned': None,
        'carried': {'y0': {'_rn_scale': 0.25}}},
    'grouped_fp8/n1/no_timer': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 1, 'tile_end': [3], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288)], 'x': ['x0'], 'y': ['y0']}, 'w', 0, 'scale', 'shift', 1.0, 4.0, 'stream'], None)], 'returned': None, 'carried': {'y0': {'_rn_scale': 0.25}}},
    'grouped_fp8/n3/t128': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 3, 'tile_end': [3, 4, 5], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1,
        1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256)], 'x': ['x0', 'x1', 'x2'], 'y': ['y0', 'y1', 'y2']}, 'w', 0, 'scale', 'shift', 1.0, 4.0, 'stream'],
        ('conv_igemm_fp8', 5000000.0, 0.0))], 'returned': None, 'carried': {'y0': {'_rn_scale': 0.25}, 'y1': {'_rn_scale': 0.25}, 'y2': {'_rn_scale': 0.25}}},
    'grouped_fp8/n3/t256': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1,
        1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256)], 'x': ['x0', 'x1', 'x2'], 'y': ['y0', 'y1', 'y2']}, 'w', 0, 'scale', 'shift', 1.0, 4.0, 'stream'],
        ('conv_igemm_fp8_p8 grouped 32->64 k3', 5000000.0, 0.0))], 'returned': None, 'carried': {'y0': {'_rn_scale': 0.25}, 'y1': {'_rn_scale': 0.25}, 'y2': {'_rn_scale': 0.25}}},
    'grouped_fp8/n5/t256': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 5, 'tile_end': [2, 3, 4, 5, 6], 'd': [('D', 2, 16, 12, 32, 16, 12, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 6144, 30720), ('D', 2, 4, 4, 32, 4, 4, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 2560), ('D', 2, 2, 2, 32, 2, 2, 160, 3,
        3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 640), ('D', 2, 1, 1, 32, 1, 1, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 32,
        160), ('D', 2, 3, 5, 32, 3, 5, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 3, 5, 0, 0, 0, 0, 480, 2400)], 'x': ['x0', 'x1', 'x2', 'x3', 'x4'], 'y': ['y0', 'y1', 'y2',
        'y3', 'y4']}, 'w', 0, 'scale', 'shift', 1.0, 4.0, 'stream'], ('conv_igemm_fp8_p8', 5000000.0, 0.0))], 'returned': None, 'carried': {'y0': {'_rn_scale': 0.25},
        'y1': {'_rn_scale': 0.25}, 'y2': {'_rn_scale': 0.25}, 'y3': {'_rn_scale': 0.25}, 'y4': {'_rn_scale': 0.25}}},
    'grouped_fp8/n5/t256x128': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 5, 'tile_end': [4, 6, 8, 10, 12], 'd': [('D', 2, 16, 12, 32, 16, 12, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0,
        0, 1, 0, 0, 16, 12, 0, 0, 0, 0, 6144, 30720), ('D', 2, 4, 4, 32, 4, 4, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 2560), ('D', 2, 2, 2, 32, 2, 2,
        160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 640), ('D', 2, 1, 1, 32, 1, 1, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0,
        32, 160), ('D', 2, 3, 5, 32, 3, 5, 160, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 3, 5, 0, 0, 0, 0, 480, 2400)], 'x': ['x0', 'x1', 'x2', 'x3', 'x4'], 'y': ['y0', 'y1', 'y2',
        'y3', 'y4']}, 'w', 0, 'scale', 'shift', 1.0, 4.0, 'stream'], ('conv_igemm_fp8', 5000000.0, 0.0))], 'returned': None, 'carried': {'y0': {'_rn_scale': 0.25}, 'y1': {'_rn_scale': 0.25},
        'y2': {'_rn_scale': 0.25}, 'y3': {'_rn_scale': 0.25}, 'y4': {'_rn_scale': 0.25}}},
    'grouped_fp8/fp32_results': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 3, 'tile_end': [3, 4, 5], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 6144, 13568), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 13568), ('D', 2, 2, 2, 32, 2, 2, 64, 3,
        3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 13568)], 'x': ['x0', 'x1', 'x2'], 'y': ['ybuf', 'ybuf+49152', 'ybuf+53248']}, 'w', 1, 'scale', 'shift', 1.0,
        4.0, 'stream'], ('conv_igemm_fp8', 5000000.0, 0.0))], 'returned': None, 'carried': {}},
    'grouped_fp8/ybs_add_mask': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 6144, 13568), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 13568), ('D', 2, 2, 2, 32, 2, 2, 64, 3,
        3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 13568)], 'x': ['x0', 'x1', 'x2'], 'y': ['ybuf', 'ybuf+12288', 'ybuf+13312']}, 'w', 0, 'scale', 'shift', 1.0,
        4.0, 'stream'], ('conv_igemm_fp8_p8', 5000000.0, 0.0))], 'returned': None, 'carried': {'mask0': {'_rn_sign': 768}, 'mask2': {'_rn_sign': 16}}},
    'grouped_bf16/add_mask_bits': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 2, 'tile_end': [3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 6144, 12288, 12288, 0, 0, 'y0._rn_sign'), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 6, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024, 1024,
        0, 0, 'y1._rn_sign')], 'x': ['x0', 'x1'], 'y': ['y0', 'y1'], 'add': ['add0', 'add1'], 'mask': ['mask0._rn_sign', 'mask1._rn_sign']}, 'w', 0, 'scale', 'shift', 'stream'],
        ('conv_igemm_bf16', 5000000.0, 0.0))], 'returned': None, 'carried': {'y0': {'_rn_sign': 768}, 'mask0': {'_rn_sign': 768}, 'y1': {'_rn_sign': 64}, 'mask1': {'_rn_sign': 64}}},
    'fprop': {'calls': [('rn_conv_igemm', [('D', 2, 9, 7, 32, 5, 4, 64, 3, 3, 2, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 5, 4, 0, 0, 0, 0, 2016, 1280, 0, 0, 0, 'ret._rn_sign', None,
        'ret._rn_amax'), 'x', 'w', 'ret', None, 'shift', None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 100416.0))], 'returned': ('torch.float32', (2, 5, 4, 64), 'ret'),
        'carried': {'ret': {'_rn_sign': 80, '_rn_amax': 128}}},
    'fprop/kw_pad': {'calls': [('rn_conv_igemm', [('D', 2, 16, 16, 4, 8, 8, 64, 7, 8, 2, 1, -3, -3, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 4096), 'x', 'w', 'ret', None, None,
        None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 98304.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'ret'), 'carried': {}},
    'dgrad/stride1': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 64, 8, 8, 32, 3, 3, 1, -1, 1, 1, 0, 0, 1, 0, 0, 6, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 4096, 2048, 2048, 0, 0, None, None,
        'ret._rn_amax'), 'dy', 'wd', 'ret', None, None, 'add', 'mask._rn_sign', None, 'stream'], ('conv_igemm_4x1', 1000000.0, 139776.0))], 'returned': ('torch.float32', (2, 8, 8, 32),
        'ret'), 'carried': {'mask': {'_rn_sign': 128}, 'ret': {'_rn_amax': 128}}},
    'dgrad/stride2_1x1_add2': {'calls': [('rn_conv_igemm', [('D', 2, 4, 4, 64, 8, 8, 32, 1, 1, 1, -1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 3, 4, 4, 512, 1024, 2048), 'dy', 'wd', 'ret',
        None, None, None, None, 'add2', 'stream'], ('conv_igemm_4x1 2x8x8 64->32 k1 a1 b-1 ds1', 1000000.0, 36864.0))], 'returned': ('torch.float32', (2, 8, 8, 32), 'ret'), 'carried': {}},
    's2_classes/k3/native': {'calls': [('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 1, 0, 0, 2, 0, 2, 0, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[0]',
        'ret', None, None, 'add', 'mask', None, 'stream'], ('conv_igemm_4x1 2x4x4 64->32 k1 a1 b-1 ds0', 1000000.0, 28672.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 3, 32, 1, 2, 1, -1, 0,
        1, 0, 0, 1, 0, 0, 2, 0, 2, 0, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[1]', 'ret', None, None, 'add', 'mask', None, 'stream'], ('conv_igemm_4x1 2x4x3 64->32 k1 a1 b-1 ds0',
        2000000.0, 33792.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 2, 1, 1, -1, 1, 0, 0, 0, 1, 0, 0, 2, 0, 2, 1, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[2]', 'ret',
        None, None, 'add', 'mask', None, 'stream'], ('conv_igemm_4x1 2x4x4 64->32 k2 a1 b-1 ds0', 2000000.0, 36864.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 3, 32, 2, 2, 1, -1, 1, 1, 0,
        0, 1, 0, 0, 2, 0, 2, 1, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[3]', 'ret', None, None, 'add', 'mask', None, 'stream'], ('conv_igemm_4x1 2x4x3 64->32 k2 a1 b-1 ds0',
        4000000.0, 50176.0))], 'returned': ('torch.float32', (2, 8, 7, 32), 'ret'), 'carried': {}},
    's2_classes/k3/split3': {'calls': [('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 1, 0, 0, 2, 0, 2, 0, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792, 0, 0, None, None,
        'ret._rn_amax'), 'dy', 'wc[0]', 'ret', None, None, 'add', 'mask', None, 'stream'], ('conv_igemm_4x1', 1000000.0, 28672.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 3, 32, 1, 2, 1,
        -1, 0, 1, 0, 0, 1, 0, 0, 2, 0, 2, 0, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792, 0, 0, None, None, 'ret._rn_amax'), 'dy', 'wc[1]', 'ret', None, None, 'add', 'mask', None, 'stream'],
        ('conv_igemm_4x1', 2000000.0, 33792.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 2, 1, 1, -1, 1, 0, 0, 0, 1, 0, 0, 2, 0, 2, 1, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792, 0, 0,
        None, None, 'ret._rn_amax'), 'dy', 'wc[2]', 'ret', None, None, 'add', 'mask', None, 'stream'], ('conv_igemm_4x1', 2000000.0, 36864.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 3,
        32, 2, 2, 1, -1, 1, 1, 0, 0, 1, 0, 0, 2, 0, 2, 1, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792, 0, 0, None, None, 'ret._rn_amax'), 'dy', 'wc[3]', 'ret', None, None, 'add', 'mask', None,
        'stream'], ('conv_igemm_4x1', 4000000.0, 50176.0))], 'returned': ('torch.float32', (2, 8, 7, 32), 'ret'), 'carried': {'ret': {'_rn_amax': 128}}},
    's2_classes/k3/splitk_split3': {'calls': [('rn_conv_igemm_splitk', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 1, 0, 0, 2, 0, 2, 0, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792, 0,
        0, None, None, 'ret._rn_amax'), 'dy', 'wc[0]', 'ret', None, None, 'add', 'mask', None, 'other', 'stream'], ('conv_igemm_4x1', 1000000.0, 0.0)), ('rn_conv_igemm_splitk', [('D', 2, 4,
        4, 64, 4, 3, 32, 1, 2, 1, -1, 0, 1, 0, 0, 1, 0, 0, 2, 0, 2, 0, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792, 0, 0, None, None, 'ret._rn_amax'), 'dy', 'wc[1]', 'ret', None, None, 'add',
        'mask', None, 'other', 'stream'], ('conv_igemm_4x1', 2000000.0, 0.0)), ('rn_conv_igemm_splitk', [('D', 2, 4, 4, 64, 4, 4, 32, 2, 1, 1, -1, 1, 0, 0, 0, 1, 0, 0, 2, 0, 2, 1, 0, 8, 7,
        0, 0, 0, 0, 1024, 1792, 1792, 0, 0, None, None, 'ret._rn_amax'), 'dy', 'wc[2]', 'ret', None, None, 'add', 'mask', None, 'other', 'stream'], ('conv_igemm_4x1', 2000000.0, 0.0)),
        ('rn_conv_igemm_splitk', [('D', 2, 4, 4, 64, 4, 3, 32, 2, 2, 1, -1, 1, 1, 0, 0, 1, 0, 0, 2, 0, 2, 1, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792, 0, 0, None, None, 'ret._rn_amax'), 'dy',
        'wc[3]', 'ret', None, None, 'add', 'mask', None, 'other', 'stream'], ('conv_igemm_4x1', 4000000.0, 0.0))], 'returned': ('torch.float32', (2, 8, 7, 32), 'ret'),
        'carried': {'ret': {'_rn_amax': 128}}},
    's2_classes/k1': {'calls': [('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048, 0, 0, 0, None, None,
        'ret._rn_amax'), 'dy', 'wc[0]', 'ret', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 20480.0))], 'returned': ('torch.float32', (2, 8, 8, 32), 'ret'),
        'carried': {'ret': {'_rn_amax': 128}}},
    's2_classes/empty_class': {'calls': [('rn_conv_igemm', [('D', 2, 1, 1, 64, 1, 1, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 1, 1, 0, 0, 0, 0, 64, 32, 0, 0, 0, None, None,
        'ret._rn_amax'), 'dy', 'wc[0]', 'ret', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 1000000.0, 8960.0))], 'returned': ('torch.float32', (2, 1, 1, 32), 'ret'),
        'carried': {'ret': {'_rn_amax': 128}}},
    'fprop_bf16': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 9, 7, 32, 5, 4, 64, 3, 3, 2, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 5, 4, 0, 0, 0, 0, 2016, 1280, 0, 0, 0, 'ret._rn_sign'),
        'x', 'w', 'ret', 0, None, 'shift', None, None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 5, 4, 64), 'ret'),
        'carried': {'ret': {'_rn_sign': 80}}},
    'fprop_bf16/fp32_out': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x', 'w', 'ret', 1,
        None, None, None, None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'ret'), 'carried': {}},
    'dgrad_bf16': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 64, 8, 8, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 6, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 4096, 2048), 'dy', 'wd', 'ret', 0, None,
        None, None, 'mask._rn_sign', 'stream'], ('conv_igemm_bf16 2x8x8 64->32 k3 a1 b-1 ds0', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'),
        'carried': {'mask': {'_rn_sign': 128}}},
    'dgrad_any_bf16': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 8, 8, 32, 1, 1, 1, -1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048, 2048), 'dy', 'wd', 'ret',
        0, None, None, 'add', None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'), 'carried': {}},
    's2_classes_bf16/k3/plain': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 1, 0, 0, 2, 0, 2, 0, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy',
        'wc[0]', 'ret', 0, None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0)), ('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 3, 32, 1, 2, 1, -1, 0, 1, 0, 0, 1, 0, 0,
        2, 0, 2, 0, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[1]', 'ret', 0, None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16', 2000000.0, 0.0)), ('rn_conv_igemm_bf16', [('D',
        2, 4, 4, 64, 4, 4, 32, 2, 1, 1, -1, 1, 0, 0, 0, 1, 0, 0, 2, 0, 2, 1, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[2]', 'ret', 0, None, None, 'add', 'mask', 'stream'],
        ('conv_igemm_bf16', 2000000.0, 0.0)), ('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 3, 32, 2, 2, 1, -1, 1, 1, 0, 0, 1, 0, 0, 2, 0, 2, 1, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy',
        'wc[3]', 'ret', 0, None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16', 4000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 7, 32), 'ret'), 'carried': {}},
    's2_classes_bf16/k3/split3': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 1, 0, 0, 2, 0, 2, 0, 0, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy',
        'wc[0]', 'ret', 0, None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16 2x4x4 64->32 k1 a1 b-1 ds0', 1000000.0, 0.0)), ('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 3, 32, 1, 2,
        1, -1, 0, 1, 0, 0, 1, 0, 0, 2, 0, 2, 0, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[1]', 'ret', 0, None, None, 'add', 'mask', 'stream'],
        ('conv_igemm_bf16 2x4x3 64->32 k1 a1 b-1 ds0', 2000000.0, 0.0)), ('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 2, 1, 1, -1, 1, 0, 0, 0, 1, 0, 0, 2, 0, 2, 1, 0, 8, 7, 0, 0, 0,
        0, 1024, 1792, 1792), 'dy', 'wc[2]', 'ret', 0, None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16 2x4x4 64->32 k2 a1 b-1 ds0', 2000000.0, 0.0)), ('rn_conv_igemm_bf16', [('D', 2,
        4, 4, 64, 4, 3, 32, 2, 2, 1, -1, 1, 1, 0, 0, 1, 0, 0, 2, 0, 2, 1, 1, 8, 7, 0, 0, 0, 0, 1024, 1792, 1792), 'dy', 'wc[3]', 'ret', 0, None, None, 'add', 'mask', 'stream'],
        ('conv_igemm_bf16 2x4x3 64->32 k2 a1 b-1 ds0', 4000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 7, 32), 'ret'), 'carried': {}},
    's2_classes_bf16/k1': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048), 'dy', 'wc[0]',
        'ret', 0, None, None, None, None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'), 'carried': {}},
    's2_classes_bf16/empty_class': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 1, 1, 64, 1, 1, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 1, 1, 0, 0, 0, 0, 64, 32), 'dy', 'wc[0]',
        'ret', 0, None, None, None, None, 'stream'], ('conv_igemm_bf16', 1000000.0, 0.0))], 'returned': ('torch.bfloat16', (2, 1, 1, 32), 'ret'), 'carried': {}},
    'layer_fp32/fwd': {'calls': [('rn_amax', ['x', 2048, 2, 'x._rn_amax', 'stream'], None), ('rn_conv_igemm', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0,
        8, 8, 0, 0, 0, 0, 2048, 4096, 4096, 0, 3, 'ret._rn_sign', 'x._rn_amax', 'ret._rn_amax', 'L.wf._rn_split16[1]', 1), 'x', 'L.wf._rn_split16[0]', 'ret', 'L.scale', 'L.shift', 'add',
        None, None, 'stream'], ('conv_igemm_4x1', 4718592.0, 156672.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'ret'), 'carried': {'x': {'_rn_amax': 128}, 'ret': {'_rn_sign': 256,
        '_rn_amax': 128, '_rn_qscale': 0.5}}},
    'layer_fp32/fwd_out_stem_products': {'calls': [('rn_split_weights', ['L.wf', 'L.wf._rn_split', 64, 224, 'stream'], None), ('rn_conv_igemm', [('D', 2, 16, 16, 4, 8, 8, 64, 7, 8, 2, 1, -3,
        -3, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 8192, 0, 0, 2), 'x', 'L.wf._rn_split', 'ybuf', 'L.scale', 'L.shift', None, None, None, 'stream'], ('conv_igemm_4x1',
        3211264.0, 126976.0))], 'returned': ('torch.float32', (2, 4096), 'ret'), 'carried': {'ret': {'_rn_qscale': 0.5}}},
    'layer_fp32/fwd_group': {'calls': [('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_amax', ['x2', 128, 2,
        'x2._rn_amax', 'stream'], None), ('rn_conv_igemm_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288, 0, 0, 3, 'ret[0]._rn_sign', 'x0._rn_amax', 'ret[0]._rn_amax', 'L.wf._rn_split16[1]', 1), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0,
        0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024, 0, 0, 3, 'ret[1]._rn_sign', 'x1._rn_amax', 'ret[1]._rn_amax', 'L.wf._rn_split16[1]', 1), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1, 1, -1,
        -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256, 0, 0, 3, 'ret[2]._rn_sign', 'x2._rn_amax', 'ret[2]._rn_amax', 'L.wf._rn_split16[1]', 1)], 'x': ['x0', 'x1', 'x2'],
        'y': ['ret[0]', 'ret[1]', 'ret[2]']}, 'L.wf._rn_split16[0]', 'L.scale', 'L.shift', 'stream'], ('conv_igemm_4x1', 15630336.0, 236544.0))], 'returned': [('torch.float32', (2, 16, 12,
        64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]'), ('torch.float32', (2, 2, 2, 64), 'ret[2]')], 'carried': {'x0': {'_rn_amax': 128}, 'x1': {'_rn_amax': 128},
        'x2': {'_rn_amax': 128}, 'ret[0]': {'_rn_sign': 768, '_rn_amax': 128, '_rn_qscale': 0.5}, 'ret[1]': {'_rn_sign': 64, '_rn_amax': 128, '_rn_qscale': 0.5}, 'ret[2]': {'_rn_sign': 16,
        '_rn_amax': 128, '_rn_qscale': 0.5}}},
    'layer_fp32/fwd_group_outs': {'calls': [('rn_conv_igemm_grouped', [{'n': 2, 'tile_end': [1, 2], 'd': [('D', 2, 8, 8, 32, 8, 8, 96, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8,
        0, 0, 0, 0, 2048, 7680), ('D', 2, 4, 4, 32, 4, 4, 96, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 7680)], 'x': ['x0', 'x1'], 'y': ['ybuf',
        'ybuf+24576']}, 'L.wf', None, 'L.shift', 'stream'], ('conv_igemm_2x2', 8847360.0, 192512.0))], 'returned': [('torch.float32', (2, 64, 96), 'ret[0]'), ('torch.float32', (2, 16, 96),
        'ret[1]')], 'carried': {}},
    'layer_fp32/bwd_data_group': {'calls': [('rn_amax', ['g0', 12288, 2, 'g0._rn_amax', 'stream'], None), ('rn_amax', ['g1', 1024, 2, 'g1._rn_amax', 'stream'], None), ('rn_amax', ['g2', 256,
        2, 'g2._rn_amax', 'stream'], None), ('rn_conv_igemm_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 64, 16, 12, 32, 3, 3, 1, -1, 1, 1, 0, 0, 1, 0, 0, 6, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 12288, 6144, 6144, 0, 3, None, 'g0._rn_amax', 'ret[0]._rn_amax', 'L.wd._rn_split16[1]', 1), ('D', 2, 4, 4, 64, 4, 4, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 6, 0,
        1, 0, 0, 4, 4, 0, 0, 0, 0, 1024, 512, 0, 0, 3, None, 'g1._rn_amax', 'ret[1]._rn_amax', 'L.wd._rn_split16[1]', 1), ('D', 2, 2, 2, 64, 2, 2, 32, 3, 3, 1, -1, 1, 1, 0, 0, 1, 0, 0, 6, 0,
        1, 0, 0, 2, 2, 0, 0, 0, 0, 256, 128, 128, 0, 3, None, 'g2._rn_amax', 'ret[2]._rn_amax', 'L.wd._rn_split16[1]', 1)], 'x': ['g0', 'g1', 'g2'], 'y': ['ret[0]', 'ret[1]', 'ret[2]'],
        'add': ['a0', None, 'a2'], 'mask': ['m0._rn_sign', 'm1._rn_sign', 'm2._rn_sign']}, 'L.wd._rn_split16[0]', None, None, 'stream'], ('conv_igemm_4x1', 15630336.0, 340992.0))],
        'returned': [('torch.float32', (2, 16, 12, 32), 'ret[0]'), ('torch.float32', (2, 4, 4, 32), 'ret[1]'), ('torch.float32', (2, 2, 2, 32), 'ret[2]')],
        'carried': {'g0': {'_rn_amax': 128}, 'g1': {'_rn_amax': 128}, 'g2': {'_rn_amax': 128}, 'm0': {'_rn_sign': 384}, 'm1': {'_rn_sign': 32}, 'm2': {'_rn_sign': 8},
        'ret[0]': {'_rn_amax': 128}, 'ret[1]': {'_rn_amax': 128}, 'ret[2]': {'_rn_amax': 128}}},
    'layer_fp32/bwd_data_group_plain': {'calls': [('rn_conv_igemm_grouped', [{'n': 2, 'tile_end': [2, 3], 'd': [('D', 2, 8, 8, 96, 16, 12, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 6144, 6144), ('D', 2, 4, 4, 96, 4, 4, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 1536, 512)], 'x': ['g0', 'g1'], 'y': ['ret[0]',
        'ret[1]']}, 'L.wd', None, None, 'stream'], ('conv_igemm_4x1', 6635520.0, 200704.0))], 'returned': [('torch.float32', (2, 16, 12, 32), 'ret[0]'), ('torch.float32', (2, 4, 4, 32),
        'ret[1]')], 'carried': {}},
    'layer_fp32/bwd_data_stride1': {'calls': [('rn_conv_igemm', [('D', 2, 8, 8, 64, 8, 8, 32, 3, 3, 1, -1, 1, 1, 0, 0, 1, 0, 0, 6, 0, 1, 0, 0, 8, 8, 3, 4, 4, 512, 4096, 2048, 2048), 'g',
        'L.wd', 'ret', None, None, 'add', 'mask._rn_sign', 'add2', 'stream'], ('conv_igemm_4x1', 4718592.0, 143872.0))], 'returned': ('torch.float32', (2, 8, 8, 32), 'ret'),
        'carried': {'mask': {'_rn_sign': 128}}},
    'layer_fp32/bwd_data_stride2_k3': {'calls': [('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048, 0, 0, 0, None,
        None, 'ret._rn_amax'), 'g', 'L.wd[0]', 'ret', None, None, None, 'mask', None, 'stream'], ('conv_igemm_4x1', 131072.0, 24576.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 2,
        1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 2, 0, 1, 8, 8, 0, 0, 0, 0, 1024, 2048, 0, 0, 0, None, None, 'ret._rn_amax'), 'g', 'L.wd[1]', 'ret', None, None, None, 'mask', None, 'stream'],
        ('conv_igemm_4x1', 262144.0, 32768.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 2, 1, 1, -1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 2, 1, 0, 8, 8, 0, 0, 0, 0, 1024, 2048, 0, 0, 0, None,
        None, 'ret._rn_amax'), 'g', 'L.wd[2]', 'ret', None, None, None, 'mask', None, 'stream'], ('conv_igemm_4x1', 262144.0, 32768.0)), ('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 2, 2,
        1, -1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 2, 1, 1, 8, 8, 0, 0, 0, 0, 1024, 2048, 0, 0, 0, None, None, 'ret._rn_amax'), 'g', 'L.wd[3]', 'ret', None, None, None, 'mask', None, 'stream'],
        ('conv_igemm_4x1', 524288.0, 49152.0))], 'returned': ('torch.float32', (2, 8, 8, 32), 'ret'), 'carried': {'ret': {'_rn_amax': 128}}},
    'layer_fp32/bwd_data_stride2_k1': {'calls': [('rn_conv_igemm', [('D', 2, 4, 4, 64, 8, 8, 32, 1, 1, 1, -1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048, 2048), 'g',
        'L.wd', 'ret', None, None, 'add', None, None, 'stream'], ('conv_igemm_4x1', 131072.0, 49152.0))], 'returned': ('torch.float32', (2, 8, 8, 32), 'ret'), 'carried': {}},
    'layer_fp32/bwd_params/native': {'calls': [('rn_conv_wgrad_batched', ['g', 64, 'x', 'L.dw', 'L.cs', 1, 0, 0, 0, 0, 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 1, None, 0, None, 0, 'stream'],
        ('conv_wgrad 2x8x8 32->64 k3 s1', 4718592.0, 0.0)), ('rn_conv_wgrad_batched', ['g2', 64, 'x2', 'L.dw', 'L.cs', 1, 0, 0, 0, 0, 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, 0, None, 0, None, 0,
        'stream'], ('conv_wgrad 2x4x4 32->64 k3 s1', 1179648.0, 0.0))], 'returned': None, 'carried': {}},
    'layer_fp32/bwd_params/split3': {'calls': [('rn_amax', ['g', 4096, 2, 'g._rn_amax', 'stream'], None), ('rn_amax', ['x', 2048, 2, 'x._rn_amax', 'stream'], None), ('rn_conv_wgrad_batched',
        ['g', 64, 'x', 'L.dw', 'L.cs', 1, 0, 0, 0, 0, 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 1, 'g._rn_amax', 2, 'x._rn_amax', 2, 'stream'], ('conv_wgrad', 4718592.0, 0.0)), ('rn_amax', ['g2',
        1024, 2, 'g2._rn_amax', 'stream'], None), ('rn_amax', ['x2', 512, 2, 'x2._rn_amax', 'stream'], None), ('rn_conv_wgrad_batched', ['g2', 64, 'x2', 'L.dw', 'L.cs', 1, 0, 0, 0, 0, 2, 4,
        4, 32, 4, 4, 64, 3, 3, 1, 1, 0, 'g2._rn_amax', 2, 'x2._rn_amax', 2, 'stream'], ('conv_wgrad', 1179648.0, 0.0))], 'returned': None, 'carried': {'g': {'_rn_amax': 128},
        'x': {'_rn_amax': 128}, 'g2': {'_rn_amax': 128}, 'x2': {'_rn_amax': 128}}},
    'layer_fp32/bwd_params/deterministic': {'calls': [('rn_conv_wgrad_det_workspace_bytes', [64, 1, 0, 2, 8, 8, 32, 8, 8, 64, 3, 3], ('conv_wgrad', 4718592.0, 0.0)),
        ('rn_conv_wgrad_batched_det', ['g', 64, 'x', 'L.dw', 'L.cs', 1, 0, 0, 0, 0, 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 1, None, 0, None, 0, None, 0, 'stream'], ('conv_wgrad', 4718592.0,
        0.0)), ('rn_conv_wgrad_det_workspace_bytes', [64, 1, 0, 2, 4, 4, 32, 4, 4, 64, 3, 3], ('conv_wgrad', 1179648.0, 0.0)), ('rn_conv_wgrad_batched_det', ['g2', 64, 'x2', 'L.dw', 'L.cs',
        1, 0, 0, 0, 0, 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, 0, None, 0, None, 0, None, 0, 'stream'], ('conv_wgrad', 1179648.0, 0.0))], 'returned': None, 'carried': {}},
    'layer_fp32/bwd_params_group': {'calls': [('rn_conv_wgrad_batched', ['g0', 64, 'x0', 'L.dw', 'L.cs', 1, 0, 0, 0, 0, 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, 0, None, 0, None, 0, 'stream'],
        ('conv_wgrad', 14155776.0, 0.0)), ('rn_conv_wgrad_batched', ['g1', 64, 'x1', 'L.dw', 'L.cs', 1, 0, 0, 0, 0, 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, 0, None, 0, None, 0, 'stream'],
        ('conv_wgrad', 1179648.0, 0.0))], 'returned': None, 'carried': {}},
    'layer_fp32/bwd_fused': {'calls': [('rn_amax', ['g', 16384, 2, 'g._rn_amax', 'stream'], None), ('rn_amax', ['x', 4096, 2, 'x._rn_amax', 'stream'], None), ('rn_conv_bwd_1x1', ['g', 'x',
        'L.wd._rn_split16[0]', 'L.wd._rn_split16[1]', 'ret', 'L.dw', 'L.cs', 'mask._rn_sign', 2, None, None, 'g._rn_amax', 'x._rn_amax', 'ret._rn_amax', 2, 8, 8, 64, 256, 1, 'stream'],
        ('conv_bwd_fused 2x8x8 64->256', 8388608.0, 329728.0))], 'returned': ('torch.float32', (2, 8, 8, 64), 'ret'), 'carried': {'g': {'_rn_amax': 128}, 'x': {'_rn_amax': 128},
        'mask': {'_rn_sign': 256}, 'ret': {'_rn_amax': 128}}},
    'layer_fp32/bwd_data_compact': {'calls': [('rn_conv_igemm', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 1024, 512), 'g', 'L.wd',
        'ret', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 131072.0, 20480.0))], 'returned': ('torch.float32', (2, 4, 4, 32), 'ret'), 'carried': {}},
    'layer_bf16/fwd': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096, 0, 0,
        'ret._rn_sign'), 'x', 'L.wf16', 'ret', 0, 'L.scale', 'L.shift', 'add', None, 'stream'], ('conv_igemm_bf16', 4718592.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 64), 'ret'),
        'carried': {'ret': {'_rn_sign': 256, '_rn_qscale': 0.5}}},
    'layer_bf16/fwd_out_fp32': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 8192), 'x', 'L.wf16',
        'ybuf+16384', 1, None, 'L.shift', None, None, 'stream'], ('conv_igemm_bf16', 4718592.0, 0.0))], 'returned': ('torch.float32', (2, 4096), 'ret'),
        'carried': {'ret': {'_rn_qscale': 0.5}}},
    'layer_bf16/fwd_group': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 3, 'tile_end': [2, 3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 6144, 12288, 0, 0, 0, 'ret[0]._rn_sign'), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024, 0, 0, 0,
        'ret[1]._rn_sign'), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256, 0, 0, 0, 'ret[2]._rn_sign')], 'x': ['x0', 'x1', 'x2'],
        'y': ['ret[0]', 'ret[1]', 'ret[2]']}, 'L.wf16', 0, 'L.scale', 'L.shift', 'stream'], ('conv_igemm_bf16_p8', 15630336.0, 0.0))], 'returned': [('torch.bfloat16', (2, 16, 12, 64),
        'ret[0]'), ('torch.bfloat16', (2, 4, 4, 64), 'ret[1]'), ('torch.bfloat16', (2, 2, 2, 64), 'ret[2]')], 'carried': {'ret[0]': {'_rn_sign': 768, '_rn_qscale': 0.5},
        'ret[1]': {'_rn_sign': 64, '_rn_qscale': 0.5}, 'ret[2]': {'_rn_sign': 16, '_rn_qscale': 0.5}}},
    'layer_bf16/fwd_group_outs': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 2, 'tile_end': [1, 2], 'd': [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0,
        8, 8, 0, 0, 0, 0, 2048, 5120), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 5120)], 'x': ['x0', 'x1'], 'y': ['ybuf',
        'ybuf+16384']}, 'L.wf16', 1, None, 'L.shift', 'stream'], ('conv_igemm_bf16', 5898240.0, 0.0))], 'returned': [('torch.float32', (2, 64, 64), 'ret[0]'), ('torch.float32', (2, 16, 64),
        'ret[1]')], 'carried': {'ret[0]': {'_rn_qscale': 0.5}, 'ret[1]': {'_rn_qscale': 0.5}}},
    'layer_bf16/bwd_data_group': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 3, 'tile_end': [3, 4, 5], 'd': [('D', 2, 16, 12, 64, 16, 12, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 2, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 12288, 6144), ('D', 2, 4, 4, 64, 4, 4, 32, 3, 3, 1, -1, 1, 1, 0, 0, 1, 0, 0, 2, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 1024, 512, 512), ('D', 2, 2, 2, 64, 2, 2, 32,
        3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 2, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 256, 128)], 'x': ['g0', 'g1', 'g2'], 'y': ['ret[0]', 'ret[1]', 'ret[2]'], 'add': [None, 'a1', None], 'mask': ['m0',
        'm1', 'm2']}, 'L.wd16', 0, None, None, 'stream'], ('conv_igemm_bf16', 15630336.0, 0.0))], 'returned': [('torch.bfloat16', (2, 16, 12, 32), 'ret[0]'), ('torch.bfloat16', (2, 4, 4,
        32), 'ret[1]'), ('torch.bfloat16', (2, 2, 2, 32), 'ret[2]')], 'carried': {}},
    'layer_bf16/bwd_data_group_plain': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 1, 'tile_end': [3], 'd': [('D', 2, 8, 8, 64, 16, 12, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 4096, 6144)], 'x': ['g0'], 'y': ['ret']}, 'L.wd16', 0, None, None, 'stream'], ('conv_igemm_bf16', 4718592.0, 0.0))], 'returned': [('torch.bfloat16', (2, 16,
        12, 32), 'ret')], 'carried': {}},
    'layer_bf16/bwd_data_stride1': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 64, 8, 8, 32, 3, 3, 1, -1, 1, 1, 0, 0, 1, 0, 0, 2, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 4096, 2048, 2048), 'g',
        'L.wd16', 'ret', 0, None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16', 4718592.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'), 'carried': {}},
    'layer_bf16/bwd_data_stride2_k3': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 2, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048), 'g',
        'L.wd16[0]', 'ret', 0, None, None, None, 'mask', 'stream'], ('conv_igemm_bf16', 131072.0, 0.0)), ('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 2, 1, -1, 0, 1, 0, 0, 0, 0,
        0, 2, 0, 2, 0, 1, 8, 8, 0, 0, 0, 0, 1024, 2048), 'g', 'L.wd16[1]', 'ret', 0, None, None, None, 'mask', 'stream'], ('conv_igemm_bf16', 262144.0, 0.0)), ('rn_conv_igemm_bf16', [('D',
        2, 4, 4, 64, 4, 4, 32, 2, 1, 1, -1, 1, 0, 0, 0, 0, 0, 0, 2, 0, 2, 1, 0, 8, 8, 0, 0, 0, 0, 1024, 2048), 'g', 'L.wd16[2]', 'ret', 0, None, None, None, 'mask', 'stream'],
        ('conv_igemm_bf16', 262144.0, 0.0)), ('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 2, 2, 1, -1, 1, 1, 0, 0, 0, 0, 0, 2, 0, 2, 1, 1, 8, 8, 0, 0, 0, 0, 1024, 2048), 'g',
        'L.wd16[3]', 'ret', 0, None, None, None, 'mask', 'stream'], ('conv_igemm_bf16', 524288.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'), 'carried': {}},
    'layer_bf16/bwd_data_stride2_k1_compact': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048),
        'g', 'L.wd16', 'ret', 0, None, None, None, None, 'stream'], ('conv_igemm_bf16', 131072.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'), 'carried': {}},
    'layer_bf16/bwd_data_stride2_k1_compact_add': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 4, 4, 32, 1, 1, 1, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 0, 8, 8, 0, 0, 0, 0, 1024,
        2048, 2048), 'g', 'L.wd16', 'add', 0, None, None, 'add', None, 'stream'], ('conv_igemm_bf16', 131072.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'add'), 'carried': {}},
    'layer_bf16/bwd_data_stride2_k1_masked': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 4, 4, 64, 8, 8, 32, 1, 1, 1, -1, 0, 0, 1, 0, 1, 0, 0, 2, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 1024, 2048,
        2048), 'g', 'L.wd16', 'ret', 0, None, None, 'add', 'mask', 'stream'], ('conv_igemm_bf16', 131072.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'), 'carried': {}},
    'layer_bf16/bwd_params': {'calls': [('rn_conv_wgrad_bf16', ['g', 64, 'x', 'L.dw', 'L.cs', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 'stream'], ('conv_wgrad_bf16 2x8x8 32->64 k3 s1', 4718592.0,
        0.0)), ('rn_conv_wgrad_bf16', ['g2', 64, 'x2', 'L.dw', 'L.cs', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, 'stream'], ('conv_wgrad_bf16 2x4x4 32->64 k3 s1', 1179648.0, 0.0))],
        'returned': None, 'carried': {}},
    'layer_bf16/bwd_params_group': {'calls': [('rn_conv_wgrad_bf16_grouped', [3, ['g0', 'g1', 'g2'], 64, ['x0', 'x1', 'x2'], 'L.dw', 'L.cs', 2, [16, 4, 2], [12, 4, 2], 32, 64, 3, 3, 1, 1,
        'stream'], ('conv_wgrad_bf16 grouped 32->64 k3', 15630336.0, 0.0))], 'returned': None, 'carried': {}},
    'layer_bf16/bwd_params_group_per_level': {'calls': [('rn_conv_wgrad_bf16', ['g0', 64, 'x0', 'L.dw', 'L.cs', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 'stream'], ('conv_wgrad_bf16', 4718592.0,
        0.0))], 'returned': None, 'carried': {}},
    'layer_fp8/fwd_two_scales': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'xa', 'L.wq',
        'ret[0]', 0, 'L._fp8_scales[0.5]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8_p8', 4718592.0, 0.0)), ('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1,
        -1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096), 'xb', 'L.wq', 'ret[1]', 0, 'L._fp8_scales[0.25]', 'L.shift', 'add', 2.0, 2.0, 'stream'], ('conv_igemm_fp8_p8',
        4718592.0, 0.0)), ('rn_conv_igemm_fp8', [('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), 'xc', 'L.wq', 'ret[2]', 0,
        'L._fp8_scales[0.5]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8_p8', 1179648.0, 0.0))], 'returned': [('torch.uint8', (2, 8, 8, 64), 'ret[0]'), ('torch.uint8', (2, 8, 8,
        64), 'ret[1]'), ('torch.uint8', (2, 4, 4, 64), 'ret[2]')], 'carried': {'xa': {'_rn_scale': 0.5}, 'xb': {'_rn_scale': 0.25}, 'add': {'_rn_scale': 2.0}, 'xc': {'_rn_scale': 0.5},
        'ret[0]': {'_rn_scale': 0.5}, 'ret[1]': {'_rn_scale': 0.5}, 'ret[2]': {'_rn_scale': 0.5}}},
    'layer_fp8/fwd_out_fp32': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 8192), 'x', 'L.wq',
        'ybuf+16384', 1, 'L._fp8_scales[0.5]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8', 4718592.0, 0.0))], 'returned': ('torch.float32', (2, 4096), 'ret'),
        'carried': {'x': {'_rn_scale': 0.5}}},
    'layer_fp8/fwd_group': {'calls': [('rn_conv_igemm_fp8_grouped', [{'n': 3, 'tile_end': [3, 4, 5], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0,
        16, 12, 0, 0, 0, 0, 6144, 12288), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), ('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1,
        1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256)], 'x': ['x0', 'x1', 'x2'], 'y': ['ret[0]', 'ret[1]', 'ret[2]']}, 'L.wq', 0, 'L._fp8_scales[0.5]', 'L.shift', 1.0,
        2.0, 'stream'], ('conv_igemm_fp8', 15630336.0, 0.0))], 'returned': [('torch.uint8', (2, 16, 12, 64), 'ret[0]'), ('torch.uint8', (2, 4, 4, 64), 'ret[1]'), ('torch.uint8', (2, 2, 2,
        64), 'ret[2]')], 'carried': {'x0': {'_rn_scale': 0.5}, 'x1': {'_rn_scale': 0.5}, 'x2': {'_rn_scale': 0.5}, 'ret[0]': {'_rn_scale': 0.5}, 'ret[1]': {'_rn_scale': 0.5},
        'ret[2]': {'_rn_scale': 0.5}}},
    'layer_fp8/fwd_group_outs': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256), 'x', 'L.wq',
        'other', 0, 'L._fp8_scales[0.5]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8', 294912.0, 0.0)), ('rn_conv_igemm_fp8_grouped', [{'n': 2, 'tile_end': [1, 2], 'd': [('D', 2,
        8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 5120), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 4,
        4, 0, 0, 0, 0, 512, 5120)], 'x': ['x0', 'x1'], 'y': ['ybuf', 'ybuf+16384']}, 'L.wq', 1, 'L._fp8_scales[0.5]', 'L.shift', 1.0, 2.0, 'stream'], ('conv_igemm_fp8', 5898240.0, 0.0))],
        'returned': [('torch.float32', (2, 64, 64), 'ret[0]'), ('torch.float32', (2, 16, 64), 'ret[1]')], 'carried': {'x': {'_rn_scale': 0.5}, 'x0': {'_rn_scale': 0.5},
        'x1': {'_rn_scale': 0.5}}},
    'layer_fp8/fwd_group_scales_differ': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096), 'x0',
        'L.wq', 'ret[0]', 0, 'L._fp8_scales[0.5]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8', 4718592.0, 0.0)), ('rn_conv_igemm_fp8', [('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1,
        -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024), 'x1', 'L.wq', 'ret[1]', 0, 'L._fp8_scales[0.25]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8',
        1179648.0, 0.0)), ('rn_conv_igemm_fp8', [('D', 2, 2, 2, 32, 2, 2, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 128, 256), 'x2', 'L.wq', 'ret[2]', 0,
        'L._fp8_scales[0.5]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8', 294912.0, 0.0))], 'returned': [('torch.uint8', (2, 8, 8, 64), 'ret[0]'), ('torch.uint8', (2, 4, 4, 64),
        'ret[1]'), ('torch.uint8', (2, 2, 2, 64), 'ret[2]')], 'carried': {'x0': {'_rn_scale': 0.5}, 'x1': {'_rn_scale': 0.25}, 'x2': {'_rn_scale': 0.5}, 'ret[0]': {'_rn_scale': 0.5},
        'ret[1]': {'_rn_scale': 0.5}, 'ret[2]': {'_rn_scale': 0.5}}},
    'layer_fp8/fwd_group_scales_differ_outs': {'calls': [('rn_conv_igemm_fp8', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 5120),
        'x0', 'L.wq', 'ybuf', 1, 'L._fp8_scales[0.5]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8', 4718592.0, 0.0)), ('rn_conv_igemm_fp8', [('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1,
        1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 5120), 'x1', 'L.wq', 'ybuf+16384', 1, 'L._fp8_scales[0.25]', 'L.shift', None, 1.0, 2.0, 'stream'], ('conv_igemm_fp8',
        1179648.0, 0.0))], 'returned': [('torch.float32', (2, 64, 64), 'ret[0]'), ('torch.float32', (2, 16, 64), 'ret[1]')], 'carried': {'x0': {'_rn_scale': 0.5},
        'x1': {'_rn_scale': 0.25}}},
    'layer_fp8_as_bf16/fwd': {'calls': [('rn_conv_igemm_bf16', [('D', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, -1, -1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 2048, 4096, 4096, 0, 0,
        'ret._rn_sign'), 'x', 'L.wf16', 'ret', 0, 'L.scale', 'L.shift', 'add', None, 'stream'], ('conv_igemm_bf16', 4718592.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 64), 'ret'),
        'carried': {'ret': {'_rn_sign': 256, '_rn_qscale': 0.5}}},
    'layer_fp8_as_bf16/fwd_group': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 2, 'tile_end': [3, 4], 'd': [('D', 2, 16, 12, 32, 16, 12, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1,
        0, 0, 16, 12, 0, 0, 0, 0, 6144, 12288, 0, 0, 0, 'ret[0]._rn_sign'), ('D', 2, 4, 4, 32, 4, 4, 64, 3, 3, 1, 1, -1, -1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 512, 1024, 0, 0,
        0, 'ret[1]._rn_sign')], 'x': ['x0', 'x1'], 'y': ['ret[0]', 'ret[1]']}, 'L.wf16', 0, 'L.scale', 'L.shift', 'stream'], ('conv_igemm_bf16', 15335424.0, 0.0))],
        'returned': [('torch.bfloat16', (2, 16, 12, 64), 'ret[0]'), ('torch.bfloat16', (2, 4, 4, 64), 'ret[1]')], 'carried': {'ret[0]': {'_rn_sign': 768, '_rn_qscale': 0.5},
        'ret[1]': {'_rn_sign': 64, '_rn_qscale': 0.5}}},
    'layer_fp8/bwd_data_group': {'calls': [('rn_conv_igemm_bf16_grouped', [{'n': 2, 'tile_end': [3, 4], 'd': [('D', 2, 16, 12, 64, 16, 12, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0,
        0, 16, 12, 0, 0, 0, 0, 12288, 6144), ('D', 2, 4, 4, 64, 4, 4, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 4, 4, 0, 0, 0, 0, 1024, 512)], 'x': ['g0', 'g1'], 'y': ['ret[0]',
        'ret[1]']}, 'L.wd16', 0, None, None, 'stream'], ('conv_igemm_bf16', 15335424.0, 0.0))], 'returned': [('torch.bfloat16', (2, 16, 12, 32), 'ret[0]'), ('torch.bfloat16', (2, 4, 4, 32),
        'ret[1]')], 'carried': {}},
    'layer_fp8/bwd_params_and_data': {'calls': [('rn_conv_wgrad_bf16', ['g', 64, 'x', 'L.dw', 'L.cs', 2, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 'stream'], ('conv_wgrad_bf16', 4718592.0, 0.0)),
        ('rn_conv_igemm_bf16', [('D', 2, 8, 8, 64, 8, 8, 32, 3, 3, 1, -1, 1, 1, 0, 0, 0, 0, 0, 2, 0, 1, 0, 0, 8, 8, 0, 0, 0, 0, 4096, 2048), 'g', 'L.wd16', 'ret', 0, None, None, None,
        'mask', 'stream'], ('conv_igemm_bf16', 4718592.0, 0.0))], 'returned': ('torch.bfloat16', (2, 8, 8, 32), 'ret'), 'carried': {}},
    'layer_wino/fwd_bwd': {'calls': [('rn_amax', ['x', 4096, 2, 'x._rn_amax', 'stream'], None), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [8], 'W': [8], 'src': ['x'],
        'amax': ['x._rn_amax']}, 'other', 64, 0, 256, 0, 'other', 'other', 'stream'], ('wino_input', 106496.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 64, 1, 256, 128, 1, 1, 1, 1, 0, 0,
        0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 16384, 32768, 0, 8192), 'other', 'L.uf', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_2x2', 4718592.0,
        8257536.0)), ('rn_wino_output_group', [{'n': 1, 'N': [2], 'H': [8], 'W': [8], 'dst': ['ret[0]'], 'sign': ['ret[0]._rn_sign'], 'amax': ['ret[0]._rn_amax']}, 'other', 128, 0, 256,
        'L.scale', 'L.shift', 0, 1, 0, 'stream'], ('wino_output', 215040.0, 0.0)), ('rn_amax', ['g', 8192, 2, 'g._rn_amax', 'stream'], None), ('rn_wino_input_both_group_flags', [{'n': 1,
        'N': [2], 'H': [8], 'W': [8], 'src': ['g'], 'amax': ['g._rn_amax']}, 'other', 'other', 128, 0, 256, 'other', 'other', None, 'stream'], ('wino_input', 360448.0, 0.0)),
        ('rn_conv_wgrad_batched', ['other', 128, 'other', 'other', 'L.cs', 36, 32768, 16384, 8192, 7, 1, 1, 8, 64, 1, 8, 128, 1, 1, 1, 0, 0, 'other', -1, 'other', -1, 'stream'],
        ('conv_wgrad', 4718592.0, 0.0)), ('rn_wino_dw', ['other', 'L.dw', 128, 64, 'stream'], None), ('rn_conv_igemm', [('D', 36, 1, 256, 128, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 32768, 16384, 0, 8192), 'other', 'L.ud', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 4718592.0, 8257536.0)),
        ('rn_wino_output_group', [{'n': 1, 'N': [2], 'H': [8], 'W': [8], 'dst': ['ret[1]'], 'add': ['add'], 'mask': ['mask._rn_sign'], 'amax': ['ret[1]._rn_amax']}, 'other', 64, 0, 256,
        None, None, 6, 0, 0, 'stream'], ('wino_output', 140288.0, 0.0))], 'returned': [('torch.float32', (2, 8, 8, 128), 'ret[0]'), ('torch.float32', (2, 8, 8, 64), 'ret[1]')],
        'carried': {'x': {'_rn_amax': 128}, 'g': {'_rn_amax': 128}, 'mask': {'_rn_sign': 256}, 'ret[0]': {'_rn_sign': 512, '_rn_amax': 128}, 'ret[1]': {'_rn_amax': 128}}},
    'layer_wino/group_fwd_bwd': {'calls': [('rn_wino_input_group', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['x0', 'x1']}, 'other', 64, 0, 256, 0, None, None, 'stream'],
        ('wino_input', 346112.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 64, 1, 256, 128, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 16384, 32768, 0, 8192),
        'other', 'L.uf', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_2x2', 15335424.0, 8257536.0)), ('rn_wino_output_group', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12,
        4], 'dst': ['ret[0]', 'ret[1]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign']}, 'other', 128, 0, 256, 'L.scale', 'L.shift', 0, 1, 0, 'stream'], ('wino_output', 698880.0, 0.0)),
        ('rn_wino_input_both_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['g0', 'g1']}, 'other', 'other', 128, 0, 256, None, None, None, 'stream'], ('wino_input',
        1171456.0, 0.0)), ('rn_conv_wgrad_batched', ['other', 128, 'other', 'other', 'L.cs', 36, 32768, 16384, 8192, 7, 1, 1, 26, 64, 1, 26, 128, 1, 1, 1, 0, 0, None, 0, None, 0, 'stream'],
        ('conv_wgrad', 15335424.0, 0.0)), ('rn_wino_dw', ['other', 'L.dw', 128, 64, 'stream'], None), ('rn_conv_igemm', [('D', 36, 1, 256, 128, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
        0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 32768, 16384, 0, 8192), 'other', 'L.ud', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 15335424.0, 8257536.0)),
        ('rn_wino_output_group', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'dst': ['ret[2]', 'ret[3]']}, 'other', 64, 0, 256, None, None, 0, 0, 0, 'stream'], ('wino_output',
        346112.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 128), 'ret[0]'), ('torch.float32', (2, 4, 4, 128), 'ret[1]'), ('torch.float32', (2, 16, 12, 64), 'ret[2]'),
        ('torch.float32', (2, 4, 4, 64), 'ret[3]')], 'carried': {'ret[0]': {'_rn_sign': 1536}, 'ret[1]': {'_rn_sign': 128}}},
    'wino/conv_six_problems/native': {'calls': [('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2', 'x3', 'x4']},
        'other', 32, 0, 256, 0, None, None, 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5']}, 'other', 32, 34, 256,
        0, None, None, 'stream'], ('wino_input', 22272.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0,
        8192, 16384, 0, 2048), 'other', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 5603328.0, 3833856.0)), ('rn_wino_output_group', [{'n': 5, 'N': [2, 2, 2, 2,
        2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'dst': ['ret[0]', 'ret[1]', 'ret[2]', 'ret[3]', 'ret[4]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign', 'ret[2]._rn_sign',
        'ret[3]._rn_sign', 'ret[4]._rn_sign']}, 'other', 64, 0, 256, 'scale', 'shift', 0, 1, 0, 'stream'], ('wino_output', 433728.0, 0.0)), ('rn_wino_output_group', [{'n': 1, 'N': [2],
        'H': [5], 'W': [3], 'dst': ['ret[5]'], 'sign': ['ret[5]._rn_sign']}, 'other', 64, 34, 256, 'scale', 'shift', 0, 1, 0, 'stream'], ('wino_output', 44784.0, 0.0))],
        'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]'), ('torch.float32', (2, 2, 2, 64), 'ret[2]'), ('torch.float32', (2, 1, 1, 64),
        'ret[3]'), ('torch.float32', (2, 3, 5, 64), 'ret[4]'), ('torch.float32', (2, 5, 3, 64), 'ret[5]')], 'carried': {'ret[0]': {'_rn_sign': 768}, 'ret[1]': {'_rn_sign': 64},
        'ret[2]': {'_rn_sign': 16}, 'ret[3]': {'_rn_sign': 4}, 'ret[4]': {'_rn_sign': 60}, 'ret[5]': {'_rn_sign': 60}}},
    'wino/conv_six_problems/split3': {'calls': [('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_amax', ['x2',
        128, 2, 'x2._rn_amax', 'stream'], None), ('rn_amax', ['x3', 32, 2, 'x3._rn_amax', 'stream'], None), ('rn_amax', ['x4', 480, 2, 'x4._rn_amax', 'stream'], None),
        ('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2', 'x3', 'x4'], 'amax': ['x0._rn_amax', 'x1._rn_amax',
        'x2._rn_amax', 'x3._rn_amax', 'x4._rn_amax']}, 'other', 32, 0, 256, 0, 'other', None, 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_amax', ['x5', 480, 2, 'x5._rn_amax', 'stream'],
        None), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5'], 'amax': ['x5._rn_amax']}, 'other', 32, 34, 256, 0, 'other', None, 'stream'], ('wino_input',
        22272.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048), 'other', 'U', 'other',
        None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 5603328.0, 3833856.0)), ('rn_wino_output_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1,
        5], 'dst': ['ret[0]', 'ret[1]', 'ret[2]', 'ret[3]', 'ret[4]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign', 'ret[2]._rn_sign', 'ret[3]._rn_sign', 'ret[4]._rn_sign'],
        'amax': ['ret[0]._rn_amax', 'ret[1]._rn_amax', 'ret[2]._rn_amax', 'ret[3]._rn_amax', 'ret[4]._rn_amax']}, 'other', 64, 0, 256, 'scale', 'shift', 0, 1, 0, 'stream'], ('wino_output',
        433728.0, 0.0)), ('rn_wino_output_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'dst': ['ret[5]'], 'sign': ['ret[5]._rn_sign'], 'amax': ['ret[5]._rn_amax']}, 'other', 64, 34, 256,
        'scale', 'shift', 0, 1, 0, 'stream'], ('wino_output', 44784.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]'),
        ('torch.float32', (2, 2, 2, 64), 'ret[2]'), ('torch.float32', (2, 1, 1, 64), 'ret[3]'), ('torch.float32', (2, 3, 5, 64), 'ret[4]'), ('torch.float32', (2, 5, 3, 64), 'ret[5]')],
        'carried': {'x0': {'_rn_amax': 128}, 'x1': {'_rn_amax': 128}, 'x2': {'_rn_amax': 128}, 'x3': {'_rn_amax': 128}, 'x4': {'_rn_amax': 128}, 'x5': {'_rn_amax': 128},
        'ret[0]': {'_rn_sign': 768, '_rn_amax': 128}, 'ret[1]': {'_rn_sign': 64, '_rn_amax': 128}, 'ret[2]': {'_rn_sign': 16, '_rn_amax': 128}, 'ret[3]': {'_rn_sign': 4, '_rn_amax': 128},
        'ret[4]': {'_rn_sign': 60, '_rn_amax': 128}, 'ret[5]': {'_rn_sign': 60, '_rn_amax': 128}}},
    'wino/conv_six_problems/by_shape': {'calls': [('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2', 'x3',
        'x4']}, 'other', 32, 0, 256, 0, None, None, 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5']}, 'other', 32,
        34, 256, 0, None, None, 'stream'], ('wino_input', 22272.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0,
        0, 0, 8192, 16384, 0, 2048), 'other', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1 36x1x256 32->64 k1 a1 b1 ds0 x36', 5603328.0, 3833856.0)),
        ('rn_wino_output_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'dst': ['ret[0]', 'ret[1]', 'ret[2]', 'ret[3]', 'ret[4]'],
        'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign', 'ret[2]._rn_sign', 'ret[3]._rn_sign', 'ret[4]._rn_sign']}, 'other', 64, 0, 256, 'scale', 'shift', 0, 1, 0, 'stream'], ('wino_output',
        433728.0, 0.0)), ('rn_wino_output_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'dst': ['ret[5]'], 'sign': ['ret[5]._rn_sign']}, 'other', 64, 34, 256, 'scale', 'shift', 0, 1, 0,
        'stream'], ('wino_output', 44784.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]'), ('torch.float32', (2, 2, 2, 64),
        'ret[2]'), ('torch.float32', (2, 1, 1, 64), 'ret[3]'), ('torch.float32', (2, 3, 5, 64), 'ret[4]'), ('torch.float32', (2, 5, 3, 64), 'ret[5]')],
        'carried': {'ret[0]': {'_rn_sign': 768}, 'ret[1]': {'_rn_sign': 64}, 'ret[2]': {'_rn_sign': 16}, 'ret[3]': {'_rn_sign': 4}, 'ret[4]': {'_rn_sign': 60}, 'ret[5]': {'_rn_sign': 60}}},
    'wino/conv_six_problems_ybs_add_mask/native': {'calls': [('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2',
        'x3', 'x4']}, 'other', 32, 0, 256, 0, None, None, 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5']}, 'other',
        32, 34, 256, 0, None, None, 'stream'], ('wino_input', 22272.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0,
        0, 0, 0, 8192, 16384, 0, 2048), 'other', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 5603328.0, 3833856.0)), ('rn_wino_output_group', [{'n': 5, 'N': [2,
        2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'dst': ['ybuf', 'ybuf+49152', 'ybuf+53248', 'ybuf+54272', 'ybuf+54528'], 'add': ['add0', 'add1', 'add2', 'add3', 'add4'],
        'mask': ['mask0._rn_sign', 'mask1._rn_sign', 'mask2._rn_sign', 'mask3._rn_sign', 'mask4._rn_sign']}, 'other', 64, 0, 256, None, None, 5, 0, 15552, 'stream'], ('wino_output',
        550464.0, 0.0)), ('rn_wino_output_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'dst': ['ybuf+58368'], 'add': ['add5'], 'mask': ['mask5']}, 'other', 64, 34, 256, None, None, 1, 0,
        15552, 'stream'], ('wino_output', 59904.0, 0.0))], 'returned': [('torch.float32', (2, 192, 64), 'ret[0]'), ('torch.float32', (2, 16, 64), 'ret[1]'), ('torch.float32', (2, 4, 64),
        'ret[2]'), ('torch.float32', (2, 1, 64), 'ret[3]'), ('torch.float32', (2, 15, 64), 'ret[4]'), ('torch.float32', (2, 15, 64), 'ret[5]')], 'carried': {'mask0': {'_rn_sign': 768},
        'mask1': {'_rn_sign': 64}, 'mask2': {'_rn_sign': 16}, 'mask3': {'_rn_sign': 4}, 'mask4': {'_rn_sign': 60}}},
    'wino/conv_six_problems_ybs_add_mask/split3': {'calls': [('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None),
        ('rn_amax', ['x2', 128, 2, 'x2._rn_amax', 'stream'], None), ('rn_amax', ['x3', 32, 2, 'x3._rn_amax', 'stream'], None), ('rn_amax', ['x4', 480, 2, 'x4._rn_amax', 'stream'], None),
        ('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2', 'x3', 'x4'], 'amax': ['x0._rn_amax', 'x1._rn_amax',
        'x2._rn_amax', 'x3._rn_amax', 'x4._rn_amax']}, 'other', 32, 0, 256, 0, 'other', None, 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_amax', ['x5', 480, 2, 'x5._rn_amax', 'stream'],
        None), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5'], 'amax': ['x5._rn_amax']}, 'other', 32, 34, 256, 0, 'other', None, 'stream'], ('wino_input',
        22272.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048), 'other', 'U', 'other',
        None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 5603328.0, 3833856.0)), ('rn_wino_output_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1,
        5], 'dst': ['ybuf', 'ybuf+49152', 'ybuf+53248', 'ybuf+54272', 'ybuf+54528'], 'add': ['add0', 'add1', 'add2', 'add3', 'add4'], 'mask': ['mask0._rn_sign', 'mask1._rn_sign',
        'mask2._rn_sign', 'mask3._rn_sign', 'mask4._rn_sign']}, 'other', 64, 0, 256, None, None, 5, 0, 15552, 'stream'], ('wino_output', 550464.0, 0.0)), ('rn_wino_output_group', [{'n': 1,
        'N': [2], 'H': [5], 'W': [3], 'dst': ['ybuf+58368'], 'add': ['add5'], 'mask': ['mask5']}, 'other', 64, 34, 256, None, None, 1, 0, 15552, 'stream'], ('wino_output', 59904.0, 0.0))],
        'returned': [('torch.float32', (2, 192, 64), 'ret[0]'), ('torch.float32', (2, 16, 64), 'ret[1]'), ('torch.float32', (2, 4, 64), 'ret[2]'), ('torch.float32', (2, 1, 64), 'ret[3]'),
        ('torch.float32', (2, 15, 64), 'ret[4]'), ('torch.float32', (2, 15, 64), 'ret[5]')], 'carried': {'x0': {'_rn_amax': 128}, 'x1': {'_rn_amax': 128}, 'x2': {'_rn_amax': 128},
        'x3': {'_rn_amax': 128}, 'x4': {'_rn_amax': 128}, 'x5': {'_rn_amax': 128}, 'mask0': {'_rn_sign': 768}, 'mask1': {'_rn_sign': 64}, 'mask2': {'_rn_sign': 16}, 'mask3': {'_rn_sign': 4},
        'mask4': {'_rn_sign': 60}}},
    'wino/wgrad_six_problems/native': {'calls': [('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2', 'x3', 'x4']},
        'other', 32, 0, 256, 0, None, None, 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5']}, 'other', 32, 34, 256,
        0, None, None, 'stream'], ('wino_input', 22272.0, 0.0)), ('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['g0', 'g1',
        'g2', 'g3', 'g4']}, 'other', 64, 0, 256, 1, None, None, 'stream'], ('wino_input', 430080.0, 0.0)), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['g5']},
        'other', 64, 34, 256, 1, None, None, 'stream'], ('wino_input', 44544.0, 0.0)), ('rn_conv_wgrad_batched', ['other', 64, 'other', 'other', 'colsum', 36, 16384, 8192, 2048, 7, 1, 1, 38,
        32, 1, 38, 64, 1, 1, 1, 0, 0, None, 0, None, 0, 'stream'], ('conv_wgrad', 5603328.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 64, 32, 'stream'], None)], 'returned': None,
        'carried': {}},
    'wino/wgrad_six_problems/split3': {'calls': [('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_amax', ['x2',
        128, 2, 'x2._rn_amax', 'stream'], None), ('rn_amax', ['x3', 32, 2, 'x3._rn_amax', 'stream'], None), ('rn_amax', ['x4', 480, 2, 'x4._rn_amax', 'stream'], None),
        ('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2', 'x3', 'x4'], 'amax': ['x0._rn_amax', 'x1._rn_amax',
        'x2._rn_amax', 'x3._rn_amax', 'x4._rn_amax']}, 'other', 32, 0, 256, 0, None, 'other', 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_amax', ['x5', 480, 2, 'x5._rn_amax', 'stream'],
        None), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5'], 'amax': ['x5._rn_amax']}, 'other', 32, 34, 256, 0, None, 'other', 'stream'], ('wino_input',
        22272.0, 0.0)), ('rn_amax', ['g0', 12288, 2, 'g0._rn_amax', 'stream'], None), ('rn_amax', ['g1', 1024, 2, 'g1._rn_amax', 'stream'], None), ('rn_amax', ['g2', 256, 2, 'g2._rn_amax',
        'stream'], None), ('rn_amax', ['g3', 64, 2, 'g3._rn_amax', 'stream'], None), ('rn_amax', ['g4', 960, 2, 'g4._rn_amax', 'stream'], None), ('rn_wino_input_group', [{'n': 5, 'N': [2, 2,
        2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['g0', 'g1', 'g2', 'g3', 'g4'], 'amax': ['g0._rn_amax', 'g1._rn_amax', 'g2._rn_amax', 'g3._rn_amax', 'g4._rn_amax']},
        'other', 64, 0, 256, 1, None, 'other', 'stream'], ('wino_input', 430080.0, 0.0)), ('rn_amax', ['g5', 960, 2, 'g5._rn_amax', 'stream'], None), ('rn_wino_input_group', [{'n': 1,
        'N': [2], 'H': [5], 'W': [3], 'src': ['g5'], 'amax': ['g5._rn_amax']}, 'other', 64, 34, 256, 1, None, 'other', 'stream'], ('wino_input', 44544.0, 0.0)), ('rn_conv_wgrad_batched',
        ['other', 64, 'other', 'other', 'colsum', 36, 16384, 8192, 2048, 7, 1, 1, 38, 32, 1, 38, 64, 1, 1, 1, 0, 0, 'other', -1, 'other', -1, 'stream'], ('conv_wgrad', 5603328.0, 0.0)),
        ('rn_wino_dw', ['other', 'dw', 64, 32, 'stream'], None)], 'returned': None, 'carried': {'x0': {'_rn_amax': 128}, 'x1': {'_rn_amax': 128}, 'x2': {'_rn_amax': 128},
        'x3': {'_rn_amax': 128}, 'x4': {'_rn_amax': 128}, 'x5': {'_rn_amax': 128}, 'g0': {'_rn_amax': 128}, 'g1': {'_rn_amax': 128}, 'g2': {'_rn_amax': 128}, 'g3': {'_rn_amax': 128},
        'g4': {'_rn_amax': 128}, 'g5': {'_rn_amax': 128}}},
    'wino/wgrad_six_problems/deterministic': {'calls': [('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['x0', 'x1', 'x2', 'x3',
        'x4']}, 'other', 32, 0, 256, 0, None, None, 'stream'], ('wino_input', 215040.0, 0.0)), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3], 'src': ['x5']}, 'other', 32,
        34, 256, 0, None, None, 'stream'], ('wino_input', 22272.0, 0.0)), ('rn_wino_input_group', [{'n': 5, 'N': [2, 2, 2, 2, 2], 'H': [16, 4, 2, 1, 3], 'W': [12, 4, 2, 1, 5], 'src': ['g0',
        'g1', 'g2', 'g3', 'g4']}, 'other', 64, 0, 256, 1, None, None, 'stream'], ('wino_input', 430080.0, 0.0)), ('rn_wino_input_group', [{'n': 1, 'N': [2], 'H': [5], 'W': [3],
        'src': ['g5']}, 'other', 64, 34, 256, 1, None, None, 'stream'], ('wino_input', 44544.0, 0.0)), ('rn_conv_wgrad_det_workspace_bytes', [64, 36, 2048, 1, 1, 38, 32, 1, 38, 64, 1, 1],
        ('conv_wgrad', 5603328.0, 0.0)), ('rn_conv_wgrad_batched_det', ['other', 64, 'other', 'other', 'colsum', 36, 16384, 8192, 2048, 7, 1, 1, 38, 32, 1, 38, 64, 1, 1, 1, 0, 0, None, 0,
        None, 0, None, 0, 'stream'], ('conv_wgrad', 5603328.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 64, 32, 'stream'], None)], 'returned': None, 'carried': {}},
    'wino/conv_need/native': {'calls': [('rn_tile_lists', ['need', 256, 'need_lists', 'need_lists+88', 'need_lists+24', 'need_lists+16', 'stream'], None), ('rn_wino_input_group_list',
        [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['x0', 'x1']}, 'ret[2]', 32, 0, 256, None, None, 'need', 'need_lists+24', 'need_lists+4', 'stream'], ('wino_input',
        173056.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048, 0, None, None, None,
        None, 0, 0, None, 'need_lists+16', 'need_lists+8'), 'ret[2]', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)),
        ('rn_wino_output_group_list', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'dst': ['ret[0]', 'ret[1]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign']}, 'other', 64, 0, 256,
        None, 'shift', 0, 1, 0, 'need_lists+88', 'need_lists', 'stream'], ('wino_output', 349440.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2,
        4, 4, 64), 'ret[1]'), ('torch.float32', (294912,), 'ret[2]')], 'carried': {'ret[0]': {'_rn_sign': 768}, 'ret[1]': {'_rn_sign': 64}}},
    'wino/conv_need/split3': {'calls': [('rn_tile_lists', ['need', 256, 'need_lists', 'need_lists+88', 'need_lists+24', 'need_lists+16', 'stream'], None), ('rn_amax', ['x0', 6144, 2,
        'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_wino_input_group_list', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4],
        'src': ['x0', 'x1'], 'amax': ['x0._rn_amax', 'x1._rn_amax']}, 'ret[2]', 32, 0, 256, 'ret[3]', 'ret[4]', 'need', 'need_lists+24', 'need_lists+4', 'stream'], ('wino_input', 173056.0,
        0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048, 0, None, None, None, None, 0, 0,
        None, 'need_lists+16', 'need_lists+8'), 'ret[2]', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)), ('rn_wino_output_group_list',
        [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'dst': ['ret[0]', 'ret[1]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign'], 'amax': ['ret[0]._rn_amax', 'ret[1]._rn_amax']},
        'other', 64, 0, 256, None, 'shift', 0, 1, 0, 'need_lists+88', 'need_lists', 'stream'], ('wino_output', 349440.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'),
        ('torch.float32', (2, 4, 4, 64), 'ret[1]'), ('torch.float32', (294912,), 'ret[2]'), ('torch.int32', (256,), 'ret[3]'), ('torch.int32', (1,), 'ret[4]')],
        'carried': {'x0': {'_rn_amax': 128}, 'x1': {'_rn_amax': 128}, 'ret[0]': {'_rn_sign': 768, '_rn_amax': 128}, 'ret[1]': {'_rn_sign': 64, '_rn_amax': 128}}},
    'wino/conv_need_in_own': {'calls': [('rn_tile_lists', ['need', 256, 'need_lists', 'need_lists+88', 'need_lists+24', 'need_lists+16', 'stream'], None), ('rn_tile_lists', ['need_in', 256,
        'need_in_lists', 'need_in_lists+88', 'need_in_lists+24', 'need_in_lists+16', 'stream'], None), ('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2,
        'x1._rn_amax', 'stream'], None), ('rn_wino_input_group_list', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['x0', 'x1'], 'amax': ['x0._rn_amax', 'x1._rn_amax']},
        'ret[2]', 32, 0, 256, 'ret[3]', 'ret[4]', 'need_in', 'need_in_lists+24', 'need_in_lists+4', 'stream'], ('wino_input', 173056.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1,
        256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048, 0, None, None, None, None, 0, 0, None, 'need_lists+16', 'need_lists+8'), 'ret[2]',
        'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)), ('rn_wino_output_group_list', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4],
        'dst': ['ret[0]', 'ret[1]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign'], 'amax': ['ret[0]._rn_amax', 'ret[1]._rn_amax']}, 'other', 64, 0, 256, None, 'shift', 0, 1, 0,
        'need_lists+88', 'need_lists', 'stream'], ('wino_output', 349440.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]'),
        ('torch.float32', (294912,), 'ret[2]'), ('torch.int32', (256,), 'ret[3]'), ('torch.int32', (1,), 'ret[4]')], 'carried': {'x0': {'_rn_amax': 128}, 'x1': {'_rn_amax': 128},
        'ret[0]': {'_rn_sign': 768, '_rn_amax': 128}, 'ret[1]': {'_rn_sign': 64, '_rn_amax': 128}}},
    'wino/conv_need_in_dense/native': {'calls': [('rn_tile_lists', ['need', 256, 'need_lists', 'need_lists+88', 'need_lists+24', 'need_lists+16', 'stream'], None), ('rn_wino_input_group',
        [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['x0', 'x1']}, 'ret[2]', 32, 0, 256, 0, None, None, 'stream'], ('wino_input', 173056.0, 0.0)), ('rn_conv_igemm', [('D', 36,
        1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048, 0, None, None, None, None, 0, 0, None, 'need_lists+16',
        'need_lists+8'), 'ret[2]', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)), ('rn_wino_output_group_list', [{'n': 2, 'N': [2, 2],
        'H': [16, 4], 'W': [12, 4], 'dst': ['ret[0]', 'ret[1]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign']}, 'other', 64, 0, 256, None, 'shift', 0, 1, 0, 'need_lists+88', 'need_lists',
        'stream'], ('wino_output', 349440.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]'), ('torch.float32', (294912,),
        'ret[2]')], 'carried': {'ret[0]': {'_rn_sign': 768}, 'ret[1]': {'_rn_sign': 64}}},
    'wino/conv_need_in_dense/split3': {'calls': [('rn_tile_lists', ['need', 256, 'need_lists', 'need_lists+88', 'need_lists+24', 'need_lists+16', 'stream'], None), ('rn_amax', ['x0', 6144,
        2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_wino_input_group', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4],
        'src': ['x0', 'x1'], 'amax': ['x0._rn_amax', 'x1._rn_amax']}, 'ret[2]', 32, 0, 256, 0, 'ret[3]', 'ret[4]', 'stream'], ('wino_input', 173056.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1,
        256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048, 0, None, None, None, None, 0, 0, None, 'need_lists+16',
        'need_lists+8'), 'ret[2]', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)), ('rn_wino_output_group_list', [{'n': 2, 'N': [2, 2],
        'H': [16, 4], 'W': [12, 4], 'dst': ['ret[0]', 'ret[1]'], 'sign': ['ret[0]._rn_sign', 'ret[1]._rn_sign'], 'amax': ['ret[0]._rn_amax', 'ret[1]._rn_amax']}, 'other', 64, 0, 256, None,
        'shift', 0, 1, 0, 'need_lists+88', 'need_lists', 'stream'], ('wino_output', 349440.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4,
        64), 'ret[1]'), ('torch.float32', (294912,), 'ret[2]'), ('torch.int32', (256,), 'ret[3]'), ('torch.int32', (1,), 'ret[4]')], 'carried': {'x0': {'_rn_amax': 128},
        'x1': {'_rn_amax': 128}, 'ret[0]': {'_rn_sign': 768, '_rn_amax': 128}, 'ret[1]': {'_rn_sign': 64, '_rn_amax': 128}}},
    'wino/conv_need_workspace_v': {'calls': [('rn_tile_lists', ['need', 256, 'need_lists', 'need_lists+88', 'need_lists+24', 'need_lists+16', 'stream'], None), ('rn_wino_input_group_list',
        [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['x0', 'x1']}, 'other', 32, 0, 256, None, None, 'need', 'need_lists+24', 'need_lists+4', 'stream'], ('wino_input', 173056.0,
        0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048, 0, None, None, None, None, 0, 0,
        None, 'need_lists+16', 'need_lists+8'), 'other', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)), ('rn_wino_output_group_list',
        [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'dst': ['ret[0]', 'ret[1]']}, 'other', 64, 0, 256, None, None, 0, 0, 0, 'need_lists+88', 'need_lists', 'stream'], ('wino_output',
        346112.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]')], 'carried': {}},
    'wino/conv_flags_out/native': {'calls': [('rn_wino_input_group', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['x0', 'x1']}, 'other', 32, 0, 256, 0, None, None, 'stream'],
        ('wino_input', 173056.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048),
        'other', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)), ('rn_wino_output_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4],
        'W': [12, 4], 'dst': ['ret[0]', 'ret[1]'], 'add': ['add0', 'add1'], 'mask': ['mask0._rn_sign', 'mask1._rn_sign']}, 'other', 64, 0, 256, None, None, 6, 0, 0, None, 'flags_out',
        'stream'], ('wino_output', 455936.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]')],
        'carried': {'mask0': {'_rn_sign': 768}, 'mask1': {'_rn_sign': 64}}},
    'wino/conv_flags_out/split3': {'calls': [('rn_amax', ['x0', 6144, 2, 'x0._rn_amax', 'stream'], None), ('rn_amax', ['x1', 512, 2, 'x1._rn_amax', 'stream'], None), ('rn_wino_input_group',
        [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['x0', 'x1'], 'amax': ['x0._rn_amax', 'x1._rn_amax']}, 'other', 32, 0, 256, 0, 'other', None, 'stream'], ('wino_input',
        173056.0, 0.0)), ('rn_conv_igemm', [('D', 36, 1, 256, 32, 1, 256, 64, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 8192, 16384, 0, 2048), 'other', 'U',
        'other', None, None, None, None, None, 'stream'], ('conv_igemm_4x1', 3833856.0, 3833856.0)), ('rn_wino_output_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4],
        'dst': ['ret[0]', 'ret[1]'], 'add': ['add0', 'add1'], 'mask': ['mask0._rn_sign', 'mask1._rn_sign'], 'amax': ['ret[0]._rn_amax', 'ret[1]._rn_amax']}, 'other', 64, 0, 256, None, None,
        6, 0, 0, None, 'flags_out', 'stream'], ('wino_output', 455936.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 64), 'ret[0]'), ('torch.float32', (2, 4, 4, 64), 'ret[1]')],
        'carried': {'x0': {'_rn_amax': 128}, 'x1': {'_rn_amax': 128}, 'mask0': {'_rn_sign': 768}, 'mask1': {'_rn_sign': 64}, 'ret[0]': {'_rn_amax': 128}, 'ret[1]': {'_rn_amax': 128}}},
    'wino/conv_v_ready_flags': {'calls': [('rn_tile_lists', ['flags', 256, 'flags_lists', 'flags_lists+88', 'flags_lists+24', 'flags_lists+16', 'stream'], None), ('rn_conv_igemm', [('D', 36,
        1, 256, 128, 1, 256, 96, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 32768, 24576, 0, 12288, 0, None, None, None, None, 0, 0, 'flags'), 'Vd', 'U', 'other',
        None, None, None, None, None, 'stream'], ('conv_igemm_2x2', 23003136.0, 10027008.0)), ('rn_wino_output_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4],
        'dst': ['ret[0]', 'ret[1]'], 'mask': ['mask0', 'mask1'], 'amax': ['ret[0]._rn_amax', 'ret[1]._rn_amax']}, 'other', 96, 0, 256, None, None, 2, 0, 0, 'flags', 'flags_out', 'stream'],
        ('wino_output', 678912.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 96), 'ret[0]'), ('torch.float32', (2, 4, 4, 96), 'ret[1]')], 'carried': {'ret[0]': {'_rn_amax': 128},
        'ret[1]': {'_rn_amax': 128}}},
    'wino/conv_v_ready_lists': {'calls': [('rn_tile_lists', ['flags', 256, 'flags_lists', 'flags_lists+88', 'flags_lists+24', 'flags_lists+16', 'stream'], None), ('rn_conv_igemm', [('D', 36,
        1, 256, 128, 1, 256, 96, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 32768, 24576, 0, 12288, 0, None, None, None, None, 0, 0, 'flags', 'flags_lists+16',
        'flags_lists+8'), 'Vd', 'U', 'other', None, None, None, None, None, 'stream'], ('conv_igemm_2x2', 23003136.0, 10027008.0)), ('rn_wino_output_group_flags', [{'n': 2, 'N': [2, 2],
        'H': [16, 4], 'W': [12, 4], 'dst': ['ret[0]', 'ret[1]'], 'mask': ['mask0', 'mask1'], 'amax': ['ret[0]._rn_amax', 'ret[1]._rn_amax']}, 'other', 96, 0, 256, None, None, 2, 0, 0,
        'flags', 'flags_out', 'stream'], ('wino_output', 678912.0, 0.0))], 'returned': [('torch.float32', (2, 16, 12, 96), 'ret[0]'), ('torch.float32', (2, 4, 4, 96), 'ret[1]')],
        'carried': {'ret[0]': {'_rn_amax': 128}, 'ret[1]': {'_rn_amax': 128}}},
    'wino/wgrad_fused_flags/split3': {'calls': [('rn_amax', ['g0', 24576, 2, 'g0._rn_amax', 'stream'], None), ('rn_amax', ['g1', 2048, 2, 'g1._rn_amax', 'stream'], None),
        ('rn_wino_input_both_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['g0', 'g1'], 'amax': ['g0._rn_amax', 'g1._rn_amax']}, 'ret[0]', 'other', 128, 0, 256,
        'ret[1]', 'other', 'flags', 'stream'], ('wino_input', 1171456.0, 0.0)), ('rn_conv_wgrad_batched_flags', ['other', 128, 'V', 'other', 'colsum', 36, 32768, 24576, 12288, 7, 1, 1, 26,
        96, 1, 26, 128, 1, 1, 1, 0, 0, 'other', -1, 'v_word', -1, 'flags', None, 0, 'stream'], ('conv_wgrad', 23003136.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 128, 96, 'stream'], None)],
        'returned': [('torch.float32', (1179648,), 'ret[0]'), ('torch.int32', (256,), 'ret[1]'), ('torch.uint8', (256,), 'flags')], 'carried': {'g0': {'_rn_amax': 128},
        'g1': {'_rn_amax': 128}}},
    'wino/wgrad_fused_flags/native_runs_dense': {'calls': [('rn_wino_input_both_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['g0', 'g1']}, 'ret', 'other', 128, 0,
        256, None, None, None, 'stream'], ('wino_input', 1171456.0, 0.0)), ('rn_conv_wgrad_batched', ['other', 128, 'V', 'other', 'colsum', 36, 32768, 24576, 12288, 7, 1, 1, 26, 96, 1, 26,
        128, 1, 1, 1, 0, 0, None, 0, None, 0, 'stream'], ('conv_wgrad', 23003136.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 128, 96, 'stream'], None)], 'returned': [('torch.float32',
        (1179648,), 'ret')], 'carried': {}},
    'wino/wgrad_fused_flags/no_once_runs_dense': {'calls': [('rn_amax', ['g0', 24576, 2, 'g0._rn_amax', 'stream'], None), ('rn_amax', ['g1', 2048, 2, 'g1._rn_amax', 'stream'], None),
        ('rn_wino_input_both_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['g0', 'g1'], 'amax': ['g0._rn_amax', 'g1._rn_amax']}, 'ret[0]', 'other', 128, 0, 256,
        'ret[1]', 'other', None, 'stream'], ('wino_input', 1171456.0, 0.0)), ('rn_conv_wgrad_batched', ['other', 128, 'V', 'other', 'colsum', 36, 32768, 24576, 12288, 7, 1, 1, 26, 96, 1, 26,
        128, 1, 1, 1, 0, 0, 'other', -1, 'v_word', -1, 'stream'], ('conv_wgrad', 23003136.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 128, 96, 'stream'], None)], 'returned': [('torch.float32',
        (1179648,), 'ret[0]'), ('torch.int32', (256,), 'ret[1]')], 'carried': {'g0': {'_rn_amax': 128}, 'g1': {'_rn_amax': 128}}},
    'wino/wgrad_fused_lists/built_here': {'calls': [('rn_amax', ['g0', 24576, 2, 'g0._rn_amax', 'stream'], None), ('rn_amax', ['g1', 2048, 2, 'g1._rn_amax', 'stream'], None),
        ('rn_tile_lists', ['flags', 256, 'ret[3]', 'ret[3]+88', 'ret[3]+24', 'ret[3]+16', 'stream'], None), ('rn_wino_input_both_group_lists', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12,
        4], 'src': ['g0', 'g1'], 'amax': ['g0._rn_amax', 'g1._rn_amax']}, 'ret[0]', 'other', 128, 0, 256, 'ret[1]', 'other', 'flags', 'ret[3]+24', 'ret[3]+4', 'stream'], ('wino_input',
        1171456.0, 0.0)), ('rn_conv_wgrad_batched_flags', ['other', 128, 'V', 'other', 'colsum', 36, 32768, 24576, 12288, 7, 1, 1, 26, 96, 1, 26, 128, 1, 1, 1, 0, 0, 'other', -1, 'v_word',
        -1, 'flags', None, 0, 'stream'], ('conv_wgrad', 23003136.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 128, 96, 'stream'], None)], 'returned': [('torch.float32', (1179648,), 'ret[0]'),
        ('torch.int32', (256,), 'ret[1]'), ('torch.uint8', (256,), 'flags'), ('torch.int32', (278,), 'ret[3]')], 'carried': {'g0': {'_rn_amax': 128}, 'g1': {'_rn_amax': 128}}},
    'wino/wgrad_fused_lists/native_runs_dense': {'calls': [('rn_wino_input_both_group_flags', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4], 'src': ['g0', 'g1']}, 'ret', 'other', 128, 0,
        256, None, None, None, 'stream'], ('wino_input', 1171456.0, 0.0)), ('rn_conv_wgrad_batched', ['other', 128, 'V', 'other', 'colsum', 36, 32768, 24576, 12288, 7, 1, 1, 26, 96, 1, 26,
        128, 1, 1, 1, 0, 0, None, 0, None, 0, 'stream'], ('conv_wgrad', 23003136.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 128, 96, 'stream'], None)], 'returned': [('torch.float32',
        (1179648,), 'ret')], 'carried': {}},
    'wino/wgrad_fused_lists_buffer': {'calls': [('rn_amax', ['g0', 24576, 2, 'g0._rn_amax', 'stream'], None), ('rn_amax', ['g1', 2048, 2, 'g1._rn_amax', 'stream'], None), ('rn_tile_lists',
        ['flags', 256, 'list_buf', 'list_buf+88', 'list_buf+24', 'list_buf+16', 'stream'], None), ('rn_wino_input_both_group_lists', [{'n': 2, 'N': [2, 2], 'H': [16, 4], 'W': [12, 4],
        'src': ['g0', 'g1'], 'amax': ['g0._rn_amax', 'g1._rn_amax']}, 'ret[0]', 'other', 128, 0, 256, 'ret[1]', 'other', 'flags', 'list_buf+24', 'list_buf+4', 'stream'], ('wino_input',
        1171456.0, 0.0)), ('rn_conv_wgrad_batched_flags', ['other', 128, 'V', 'other', 'colsum', 36, 32768, 24576, 12288, 7, 1, 1, 26, 96, 1, 26, 128, 1, 1, 1, 0, 0, 'other', -1, 'v_word',
        -1, 'flags', None, 0, 'stream'], ('conv_wgrad', 23003136.0, 0.0)), ('rn_wino_dw', ['other', 'dw', 128, 96, 'stream'], None)], 'returned': [('torch.float32', (1179648,), 'ret[0]'),
        ('torch.int32', (256,), 'ret[1]'), ('torch.uint8', (256,), 'flags'), ('torch.int32', (278,), 'list_buf')], 'carried': {'g0': {'_rn_amax': 128}, 'g1': {'_rn_amax': 128}}},
}

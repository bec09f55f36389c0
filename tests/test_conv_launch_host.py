"""CPU: what the convolution launchers choose and refuse (csrc/conv_launch.h and the conv_*.hip launchers), host code only.

Tile choice: the pure host queries over tests/conv_launch_cases.py's table, against answers recorded before the launch helpers were
shared.  Refusals: per launcher one call per rule of its checks, legal but for that rule, which must come back RN_EINVAL -- every one is
refused before the launcher's first HIP call, so nothing here needs or touches a GPU, and no launcher is called with a legal problem.
"""
import ctypes

import pytest

import conv_launch_cases as C


@pytest.fixture(scope="module")
def lib():
    from retinanet_mi355x import _hip
    return _hip.load()


@pytest.fixture
def restore(lib):
    """Options and product mode as they were, whatever the test set."""
    opts = {o: lib.rn_get_option(o) for o in (C.RN_OPT_SPLITK, C.RN_OPT_BF16_P8, C.RN_OPT_FP8_P8)}
    mode = lib.rn_get_fp32_mfma()
    yield
    for o, v in opts.items():
        assert lib.rn_set_option(o, v) == 0
    assert lib.rn_set_fp32_mfma(mode) == 0


def _desc(d):
    from retinanet_mi355x import _hip
    return _hip.ConvDesc(**d)


def _group(ds, ps=None, n=None, tile_end=None):
    from retinanet_mi355x import _hip
    g = _hip.ConvGroup()
    g.n = len(ds) if n is None else n
    for i, d in enumerate(ds):
        g.d[i] = _desc(d)
        p = C.pointers(d, {}) if ps is None else ps[i]
        g.x[i], g.y[i], g.add[i], g.mask[i] = p["x"], p["y"], p["add"] or None, p["mask"] or None
        g.tile_end[i] = 0 if tile_end is None else tile_end[i]
    return g


def _set_p8(lib, m):
    assert lib.rn_set_option(C.RN_OPT_BF16_P8, m) == 0 and lib.rn_set_option(C.RN_OPT_FP8_P8, m) == 0


def observe_tiles(lib):
    """-> (TILE_EXPECTED, GROUP_EXPECTED) as this library answers (also how the recorded tables were made)."""
    tiles, groups = {}, {}
    assert lib.rn_set_option(C.RN_OPT_SPLITK, 1) == 0
    for name, over, yf32 in C.TILE_CASES:
        d = C.desc(**over)
        cd, g = _desc(d), _group([d])
        by_mode = []
        for m in (0, 1, 2):
            _set_p8(lib, m)
            by_mode.append((lib.rn_conv_igemm_bf16_tile(ctypes.byref(cd), yf32), lib.rn_conv_igemm_bf16_tile_rows(ctypes.byref(g), yf32),
                            lib.rn_conv_igemm_fp8_tile(ctypes.byref(cd), yf32), lib.rn_conv_igemm_fp8_tile_rows(ctypes.byref(g), yf32)))
        wants = []
        for mode in (C.FP32_NATIVE, C.FP32_SPLIT, C.FP32_SPLIT3):
            assert lib.rn_set_fp32_mfma(mode) == 0
            wants.append(lib.rn_conv_igemm_wants_f16(ctypes.byref(cd)))
        tiles[name] = (tuple(by_mode), lib.rn_conv_splitk_workspace_bytes(ctypes.byref(cd)), tuple(wants))
    for name, overs, yf32 in C.TILE_GROUPS:
        g = _group([C.desc(**o) for o in overs])
        by_mode = []
        for m in (0, 1, 2):
            _set_p8(lib, m)
            by_mode.append((lib.rn_conv_igemm_bf16_tile_rows(ctypes.byref(g), yf32), lib.rn_conv_igemm_fp8_tile_rows(ctypes.byref(g), yf32)))
        groups[name] = tuple(by_mode)
    return tiles, groups


def test_tile_choice_matches_the_record(lib, restore):
    tiles, groups = observe_tiles(lib)
    assert set(C.TILE_EXPECTED) == {n for n, _, _ in C.TILE_CASES} and set(C.GROUP_EXPECTED) == {n for n, _, _ in C.TILE_GROUPS}
    wrong = [(n, tiles[n], C.TILE_EXPECTED[n]) for n in tiles if tiles[n] != C.TILE_EXPECTED[n]]
    wrong += [(n, groups[n], C.GROUP_EXPECTED[n]) for n in groups if groups[n] != C.GROUP_EXPECTED[n]]
    assert not wrong, wrong


def test_tile_table_exercises_every_tile(lib):
    """The record is worth something only if the table reaches each answer the queries can give."""
    seen_bf16 = {v for t in C.TILE_EXPECTED.values() for m in t[0] for v in m[:2]} | {m[0] for g in C.GROUP_EXPECTED.values() for m in g}
    seen_fp8 = {v for t in C.TILE_EXPECTED.values() for m in t[0] for v in m[2:]} | {m[1] for g in C.GROUP_EXPECTED.values() for m in g}
    assert seen_bf16 == {128128, 256128, 256256, 1256256} and seen_fp8 == {128128, 256256}
    assert {t[1] > 0 for t in C.TILE_EXPECTED.values()} == {False, True}
    assert {t[2] for t in C.TILE_EXPECTED.values()} == {(0, 0, 1)}


def test_tile_rows_refuses_a_bad_group_size(lib):
    g = _group([C.desc()])
    for n in (0, -1, C.RN_MAX_GROUP + 1):
        g.n = n
        assert lib.rn_conv_igemm_bf16_tile_rows(ctypes.byref(g), 0) == 0 and lib.rn_conv_igemm_fp8_tile_rows(ctypes.byref(g), 0) == 0
    assert lib.rn_conv_splitk_workspace_bytes(ctypes.byref(_desc(C.desc(kh=0)))) == 0


def _call_single(lib, launcher, c):
    d, p = _desc(c["d"]), C.pointers(c["d"], c["ptrs"])
    v = lambda k: p[k] or None
    if launcher == "rn_conv_igemm":
        return lib.rn_conv_igemm(ctypes.byref(d), v("x"), v("w"), v("y"), None, None, v("add"), v("mask"), v("add2"), None)
    if launcher == "rn_conv_igemm_bf16":
        return lib.rn_conv_igemm_bf16(ctypes.byref(d), v("x"), v("w"), v("y"), c["yf32"], None, None, v("add"), v("mask"), None)
    return lib.rn_conv_igemm_fp8(ctypes.byref(d), v("x"), v("w"), v("y"), c["yf32"], None, None, v("add"), 1.0, 1.0, None)


def _call_grouped(lib, launcher, c):
    g = _group(c["ds"], c["ps"], c["n"], c["tile_end"])
    if launcher == "rn_conv_igemm_grouped":
        return lib.rn_conv_igemm_grouped(ctypes.byref(g), c["w"], None, None, None)
    if launcher == "rn_conv_igemm_bf16_grouped":
        return lib.rn_conv_igemm_bf16_grouped(ctypes.byref(g), c["w"], c["yf32"], None, None, None)
    return lib.rn_conv_igemm_fp8_grouped(ctypes.byref(g), c["w"], c["yf32"], None, None, 1.0, 1.0, None)


@pytest.mark.parametrize("launcher", ["rn_conv_igemm", "rn_conv_igemm_grouped", "rn_conv_igemm_bf16", "rn_conv_igemm_bf16_grouped",
                                      "rn_conv_igemm_fp8", "rn_conv_igemm_fp8_grouped"])
def test_launcher_refuses(lib, restore, launcher):
    cases = C.refusals(launcher)
    assert len({c["name"] for c in cases}) == len(cases) >= 20
    _set_p8(lib, 0)                                             # the 128 x 128 tiles: what the cases' tile_end counts
    call = _call_grouped if launcher.endswith("_grouped") else _call_single
    got = {}
    for c in cases:
        assert lib.rn_set_fp32_mfma(c["mode"]) == 0
        got[c["name"]] = call(lib, launcher, c)
    assert {n: rc for n, rc in got.items() if rc != C.RN_EINVAL} == {}

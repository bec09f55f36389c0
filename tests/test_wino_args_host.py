"""CPU: what the Winograd group entry points (csrc/conv_wino.hip) refuse.

Every call here must come back with RN_EINVAL from the host-side argument checks, before any launch, so neither a GPU nor real memory is
needed: the pointers are made-up addresses that nothing dereferences.  There is no accepted call in this file on purpose -- an accepted
call launches a kernel.  Each case starts from a set of arguments the entry point takes (GOOD) and breaks one thing.

REFUSED was made on the library before the eight entry points were folded onto one checker per side and holds unchanged after it;
TIGHTENED lists what only the shared checkers refuse (a check one entry had and its twin had merely left out).
"""
import ctypes

import pytest

RN_EINVAL = 10001
P = 0x7f0000001000                                  # a 4096-aligned address nobody reads
STREAM = None


def group(hip, n=1, N=1, H=8, W=8, src=P, dst=P, add=None, mask=None, sign=None, **arrays):
    """rn_wino_group of n equal problems (2 x 2 tiles each); arrays: per-problem overrides, e.g. H=[8, 0]."""
    g = hip.WinoGroup()
    g.n = n
    vals = dict(N=N, H=H, W=W, src=src, dst=dst, add=add, mask=mask, sign=sign)
    for i in range(min(max(n, 1), hip.RN_MAX_GROUP)):
        for name, v in vals.items():
            getattr(g, name)[i] = v[i] if isinstance(v, list) else v
    return g


# entry point -> (parameter names after the group, the arguments of a call it takes)
INPUT = dict(C=8, tile_offset=0, Tpad=256)
OUTPUT = dict(M=P, Cout=32, tile_offset=0, Tpad=256, scale=None, shift=None, mask_mode=0, act=0, y_batch_stride=0)
GOOD = {
    "rn_wino_input_group": dict(V=P, **INPUT, dy_form=0, row_amax=None, tensor_amax=None),
    "rn_wino_input_group_list": dict(V=P, **INPUT, row_amax=None, tensor_amax=None, flags=P, units=P, n_units=P),
    "rn_wino_input_both_group": dict(V=P, Z=P, **INPUT, v_row_amax=None, z_tensor_amax=None),
    "rn_wino_input_both_group_flags": dict(V=P, Z=P, **INPUT, v_row_amax=None, z_tensor_amax=None, flags=P),
    "rn_wino_input_both_group_lists": dict(V=P, Z=P, **INPUT, v_row_amax=None, z_tensor_amax=None, flags=P, units=P, n_units=P),
    "rn_wino_output_group": dict(OUTPUT),
    "rn_wino_output_group_flags": dict(OUTPUT, flags_in=P, flags_out=P),
    "rn_wino_output_group_list": dict(OUTPUT, tiles=P, n_tiles=P),
}
INPUTS = [e for e in GOOD if "input" in e]
OUTPUTS = [e for e in GOOD if "output" in e]
MASK_BITS = 4

REFUSED = []                                        # (entry point, what is wrong, group overrides, argument overrides)
TIGHTENED = []


def refuse(entries, what, g=None, table=None, **args):
    for e in entries:
        (REFUSED if table is None else table).append((e, what, g or {}, args))


# ---- the group itself, and what every entry point checks of its own arguments
refuse(GOOD, "n = 0", dict(n=0))
refuse(GOOD, "n = RN_MAX_GROUP + 1", dict(n=6))
for dim in "NHW":
    refuse(GOOD, dim + " = 0", {dim: 0})
    refuse(GOOD, dim + " < 0 in the second problem", {"n": 2, dim: [8, -1]})
refuse(GOOD, "negative tile_offset", tile_offset=-1)
refuse(GOOD, "tile_offset + tiles > Tpad", tile_offset=253)
refuse(GOOD, "tiles > Tpad", dict(n=5, N=16), Tpad=256)                       # 5 x 16 x 4 = 320 tiles
for c in (0, -4, 6, 33):
    refuse(INPUTS, "C = %d" % c, C=c)
    refuse(OUTPUTS, "Cout = %d" % c, Cout=c)
refuse(INPUTS, "NULL src", dict(src=None))
refuse(INPUTS, "NULL src in the second problem", dict(n=2, src=[P, None]))
refuse(OUTPUTS, "NULL dst", dict(dst=None))
refuse(OUTPUTS, "NULL dst in the second problem", dict(n=2, dst=[P, None]))

# ---- input side
refuse(["rn_wino_input_group"], "dy_form with row_amax", dy_form=1, row_amax=P)
refuse([e for e in INPUTS if e != "rn_wino_input_group"], "NULL V", V=None)
refuse([e for e in INPUTS if "both" in e], "NULL Z", Z=None)
refuse(["rn_wino_input_both_group_flags", "rn_wino_input_both_group_lists"], "flags not 16-byte aligned", flags=P + 8)
refuse(["rn_wino_input_both_group_flags", "rn_wino_input_both_group_lists", "rn_wino_input_group_list"], "Tpad not a multiple of 16", Tpad=248)
for e in ("rn_wino_input_group_list", "rn_wino_input_both_group_lists"):
    for a in ("flags", "units", "n_units"):
        refuse([e], "NULL " + a, **{a: None})
    refuse([e], "units not 4-byte aligned", units=P + 2)
refuse(["rn_wino_input_group_list"], "n_units not 4-byte aligned", n_units=P + 2)

# ---- output side
for mm, what in ((3, "mask mode 3"), (MASK_BITS, "RN_MASK_BITS alone"), (MASK_BITS | 3, "mask mode 3 with RN_MASK_BITS"), (8 | 2, "an unknown bit"),
                 (-1, "a negative mask mode")):
    refuse(OUTPUTS, what, dict(mask=P), mask_mode=mm)
refuse(OUTPUTS, "a mask pointer without a mode", dict(mask=P), mask_mode=0)
refuse(OUTPUTS, "a mask pointer without a mode in the second problem", dict(n=2, mask=[None, P]), mask_mode=0)
refuse(OUTPUTS, "a mode without a mask pointer", mask_mode=2)
refuse(OUTPUTS, "a mode without a mask pointer in the second problem", dict(n=2, mask=[P, None]), mask_mode=1)
refuse(OUTPUTS, "act = 3", act=3)
refuse(OUTPUTS, "act = -1", act=-1)
refuse(OUTPUTS, "y_batch_stride not a multiple of 4", y_batch_stride=8 * 8 * 32 + 2)
refuse(OUTPUTS, "y_batch_stride below H * W * Cout", y_batch_stride=8 * 8 * 32 - 4)
refuse(OUTPUTS, "negative y_batch_stride", y_batch_stride=-4)
refuse(OUTPUTS, "Cout = 16 with sign words", dict(sign=P), Cout=16)
refuse(OUTPUTS, "Cout = 16 with mask bits", dict(mask=P), Cout=16, mask_mode=MASK_BITS | 2)
for a in ("tiles", "n_tiles"):
    refuse(["rn_wino_output_group_list"], "NULL " + a, **{a: None})
    refuse(["rn_wino_output_group_list"], a + " not 4-byte aligned", **{a: P + 2})

# ---- what only the shared checkers refuse: conv.py never makes these calls (V is always a tensor; n_units is counts + 4 of an int32 tensor)
refuse(["rn_wino_input_group"], "NULL V (its list twin checked it)", table=TIGHTENED, V=None)
refuse(["rn_wino_input_group"], "NULL Z of the dy form", table=TIGHTENED, V=None, dy_form=1)
refuse(["rn_wino_input_both_group_lists"], "n_units not 4-byte aligned (rn_wino_input_group_list checked it)", table=TIGHTENED, n_units=P + 2)

# ---- rn_tile_lists(flags, Tpad, counts, tiles, units, blocks, stream)
TILE_LISTS_GOOD = dict(flags=P, Tpad=256, counts=P, tiles=P, units=P, blocks=P)
TILE_LISTS_REFUSED = [("Tpad above 256 * 128", dict(Tpad=256 * 128 + 256)), ("Tpad not a multiple of 256", dict(Tpad=384)),
                      ("Tpad = 0", dict(Tpad=0)), ("negative Tpad", dict(Tpad=-256)), ("flags not 16-byte aligned", dict(flags=P + 4))]
TILE_LISTS_REFUSED += [("NULL " + a, {a: None}) for a in ("flags", "counts", "tiles", "units", "blocks")]
TILE_LISTS_REFUSED += [(a + " not 4-byte aligned", {a: P + 2}) for a in ("counts", "tiles", "units", "blocks")]


@pytest.fixture(scope="module")
def hip():
    from retinanet_mi355x import _hip
    _hip.load()
    return _hip


def call(hip, entry, g_over, arg_over):
    args = dict(GOOD[entry], **arg_over)
    assert set(arg_over) <= set(GOOD[entry]), (entry, arg_over)
    assert len(args) + 2 == len(hip.SIGNATURES[entry][1]), entry
    g = group(hip, **g_over)
    return getattr(hip.load(), entry)(ctypes.byref(g), *args.values(), STREAM)


def ids(table):
    return ["%s: %s" % (e[0][3:], e[1]) for e in table]


@pytest.mark.parametrize("case", REFUSED, ids=ids(REFUSED))
def test_refused(hip, case):
    entry, what, g_over, arg_over = case
    assert call(hip, entry, g_over, arg_over) == RN_EINVAL, (entry, what)


@pytest.mark.parametrize("case", TIGHTENED, ids=ids(TIGHTENED))
def test_refused_since_the_checkers_are_shared(hip, case):
    entry, what, g_over, arg_over = case
    assert call(hip, entry, g_over, arg_over) == RN_EINVAL, (entry, what)


@pytest.mark.parametrize("case", TILE_LISTS_REFUSED, ids=[c[0] for c in TILE_LISTS_REFUSED])
def test_tile_lists_refused(hip, case):
    args = dict(TILE_LISTS_GOOD, **case[1])
    assert hip.load().rn_tile_lists(*args.values(), STREAM) == RN_EINVAL, case[0]


def test_null_group(hip):
    for entry in GOOD:
        assert getattr(hip.load(), entry)(None, *GOOD[entry].values(), STREAM) == RN_EINVAL, entry


def test_every_entry_point_is_covered():
    assert {e[0] for e in REFUSED} == set(GOOD) and len(GOOD) == 8
    for entry in GOOD:                                # ... with the refusals of the group, the sizes and the offsets at least
        assert len([e for e in REFUSED if e[0] == entry]) >= 15, entry

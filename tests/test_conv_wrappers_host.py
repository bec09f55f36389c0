"""CPU: what the Python convolution wrappers (retinanet_mi355x/conv.py, engine.Layer) hand the library, call by call.

A recording stand-in takes the place of the loaded library, so neither the built library nor a GPU is needed and the wrappers run on
small CPU tensors.  Each case of tests/conv_wrapper_cases.py calls one wrapper; its record is the list of library calls -- entry point,
every field of each rn_conv_desc / rn_conv_group passed by reference (copied at call time; a descriptor as ("D", values in field order),
zero / NULL fields left out at its end), every scalar, and the (kind, work, bytes) the profiler's timer was given -- plus what came back: dtype and shape of the results and the side data they carry.  The pure host
queries (product mode, options, tile choice, split-K workspace size, capture id) are answered from the case's settings and not
recorded.  Pointers are recorded by meaning (the case's name of the tensor they point into plus a byte offset; "other" for a scratch
tensor nobody can reach afterwards), never by value.  EXPECTED is observe() on the wrappers as they were before the three engines'
copies were folded onto shared builders: any change to what reaches the library shows here as a differing case.
"""
import ctypes
import functools
import types

import pytest
import torch

import conv_wrapper_cases as C

STREAM = 0x5EED                                     # the stand-in stream handle; recorded as "stream"
SIDE = ("_rn_sign", "_rn_amax", "_rn_split", "_rn_split16")
LAYER_TENSORS = ("wf", "wf16", "wq", "wscale", "scale", "shift", "wd", "wd16", "dw", "cs")
_BYREF = type(ctypes.byref(ctypes.c_int()))


def _snap(v, ctype):
    """A ctypes value copied into plain Python; pointers as ("ptr", raw integer) until the case has ended."""
    if ctype is ctypes.c_void_p:
        return ("ptr", v.value if isinstance(v, ctypes.c_void_p) else v)
    if type(v).__name__ == "ConvDesc":              # ("D", field values in order); the zero / NULL fields at the end are left out
        vals = [_snap(getattr(v, name), ft) for name, ft in v._fields_]
        while vals and vals[-1] in (0, None, ("ptr", None)):
            vals.pop()
        return ("D",) + tuple(vals)
    if isinstance(v, ctypes.Structure):
        out = {}
        n = getattr(v, "n", None)                   # rn_conv_group: the first n entries of every array
        for name, ft in v._fields_:
            f = getattr(v, name)
            if issubclass(ft, ctypes.Array):
                f = [_snap(e, ft._type_) for e in list(f)[:n]]
            else:
                f = _snap(f, ft)
            if f not in (0, None, ("ptr", None)) and f != [("ptr", None)] * len(f if isinstance(f, list) else ()):    # left out: zero / NULL
                out[name] = f
        return out
    return v


class Recorder:
    """Stands in for the loaded library: answers the pure host queries from the case's settings, records everything else and
    answers 0."""

    def __init__(self, hip, settings):
        self.hip, self.s, self.calls, self.timing = hip, settings, [], None

    def __getattr__(self, name):
        if not name.startswith("rn_"):
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _call(self, name, *args):
        s = self.s
        if name == "rn_get_fp32_mfma":
            return s["mfma"]
        if name == "rn_get_option":
            return s["options"].get(args[0], 0)
        if name == "rn_fp32_split_min_k":
            return s["split_min_k"]
        if name == "rn_conv_splitk_workspace_bytes":
            return s["splitk_ws"]
        if name == "rn_conv_igemm_wants_f16":
            return s["wants_f16"]
        if name in ("rn_conv_igemm_bf16_tile", "rn_conv_igemm_fp8_tile"):
            return s["tile"]
        if name in ("rn_conv_igemm_bf16_tile_rows", "rn_conv_igemm_fp8_tile_rows"):
            return s["tile_rows"]
        if name == "rn_stream_capture_id":
            return 0
        types_ = self.hip.SIGNATURES[name][1]
        assert len(types_) == len(args), (name, len(types_), len(args))
        rec = []
        for a, t in zip(args, types_):
            if isinstance(a, _BYREF):
                rec.append(_snap(a._obj, type(a._obj)))
            elif isinstance(a, ctypes.Array):
                rec.append([_snap(e, a._type_) for e in a])
            else:
                rec.append(_snap(a, t))
        self.calls.append((name, rec, self.timing))
        return 0


class Timer:
    """prof.ACTIVE: no events, the (kind, work, nbytes) go to the calls made inside."""

    def __init__(self, lib):
        self.lib = lib

    def launch(self, kind, work, fn, nbytes=0.0):
        self.lib.timing = (kind, work, nbytes)
        try:
            return fn()
        finally:
            self.lib.timing = None


class Env:
    """What a case works with: the modules, named CPU tensors (t / name) and a Layer built by hand (conv_wrapper_cases.layer)."""

    def __init__(self, cv, eng, arch, hip):
        self.cv, self.eng, self.arch, self.hip, self.torch = cv, eng, arch, hip, torch
        self.T = {}
        self.L = None

    def name(self, name, tensor):
        assert name not in self.T
        self.T[name] = tensor
        return tensor

    def t(self, name, shape, dtype=torch.float32):
        return self.name(name, torch.zeros(shape, dtype=dtype))


def _extent(t):
    if t.is_contiguous():
        return t.numel() * t.element_size()
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def _side(t):
    """[(suffix, tensor)] of the side tensors t carries."""
    out = []
    for a in SIDE:
        v = getattr(t, a, None)
        if a == "_rn_amax" and v is not None:
            v = v[0]
        if isinstance(v, tuple):
            out += [("%s[%d]" % (a, i), e) for i, e in enumerate(v)]
        elif v is not None:
            out.append((a, v))
    return out


def _describe(t, T):
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return [_describe(e, T) for e in t]
    same = [n for n, o in T.items() if o is t]
    return (str(t.dtype), tuple(t.shape), same[0] if same else None)       # (dtype, shape, the case's name of this very tensor)


def observe_case(settings, fn):
    from retinanet_mi355x import _hip, arch, conv, engine, prof
    s = dict(C.DEFAULTS, **settings)
    with pytest.MonkeyPatch.context() as mp:
        lib = Recorder(_hip, s)
        mp.setattr(_hip, "_lib", lib)
        mp.setattr(_hip, "need_gpu", lambda *tensors: None)
        mp.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=STREAM))
        mp.setattr(conv, "_AMAX_CHUNK", {})
        mp.setattr(conv, "_WINO_WS", {})
        mp.setattr(conv, "BITMASKS", True)
        mp.setattr(conv, "PRESPLIT", True)
        mp.setattr(conv, "BWD_FUSED_LAUNCHES", 0)
        mp.setattr(engine, "GROUPED_WGRAD_BF16", True)
        mp.setattr(engine, "FUSE_DY", True)
        mp.setattr(engine, "S2_SHORTCUT_COMPACT", True)
        mp.setattr(prof, "ACTIVE", Timer(lib) if s["timer"] else None)
        mp.setattr(prof, "BY_SHAPE", s["by_shape"])
        held = []                                   # no allocation of the case is freed before its pointers are resolved: no address twice

        def holding(make):
            def wrapped(*args, **kw):
                held.append(make(*args, **kw))
                return held[-1]
            return wrapped
        for f in ("empty", "zeros", "empty_like", "zeros_like"):
            mp.setattr(torch, f, holding(getattr(torch, f)))
        env = Env(conv, engine, arch, _hip)
        ret = fn(env)
        T = dict(env.T)
        if env.L is not None:                       # what the layer made for itself: accumulators, fp8 scale vectors
            have = {id(t) for t in T.values()}
            made = [("L." + a, getattr(env.L, a, None)) for a in LAYER_TENSORS]
            made += [("L._fp8_scales[%r]" % k, v) for k, v in getattr(env.L, "_fp8_scales", {}).items()]
            for n, v in made:
                for i, e in enumerate(v if isinstance(v, list) else [v]):
                    if e is not None and id(e) not in have:
                        T[n + ("[%d]" % i if isinstance(v, list) else "")] = e
        flat = ret if isinstance(ret, (list, tuple)) else [ret]
        for i, r in enumerate(flat):
            if isinstance(r, torch.Tensor) and not any(o is r for o in T.values()):
                T["ret[%d]" % i if len(flat) > 1 else "ret"] = r
        spans = [(n, t.data_ptr(), _extent(t)) for n, t in T.items()]
        spans += [("%s.%s" % (n, a), v.data_ptr(), _extent(v)) for n, t in T.items() for a, v in _side(t)]

        def resolve(v):
            if isinstance(v, tuple) and v[:1] == ("D",):
                return tuple(resolve(e) for e in v)
            if isinstance(v, tuple) and len(v) == 2 and v[0] == "ptr":
                if v[1] is None or v[1] == 0:
                    return None
                if v[1] == STREAM:
                    return "stream"
                for n, p, size in spans:
                    if size and p <= v[1] < p + size:
                        return "%s+%d" % (n, v[1] - p) if v[1] != p else n
                return "other"
            if isinstance(v, dict):
                return {k: resolve(e) for k, e in v.items()}
            if isinstance(v, list):
                return [resolve(e) for e in v]
            return v

        carried = {}
        for n, t in T.items():
            c = {a: getattr(t, a)[0].numel() if a == "_rn_amax" else getattr(t, a).numel() for a in ("_rn_sign", "_rn_amax") if hasattr(t, a)}
            c.update({a: getattr(t, a) for a in ("_rn_scale", "_rn_qscale") if hasattr(t, a)})
            if c:
                carried[n] = c
        return {"calls": [(name, resolve(rec), timing) for name, rec, timing in lib.calls], "returned": _describe(ret, T), "carried": carried}


def observe():
    """-> {case name: record}: EXPECTED as this code answers (also how the recorded table was made)."""
    names = [c[0] for c in C.CASES]
    assert len(set(names)) == len(names)
    return {name: observe_case(settings, fn) for name, settings, fn in C.CASES}


def _ser(v):
    """repr(v) with a NUL after every separator this function writes: where a line may end."""
    if isinstance(v, dict):
        return "{" + ", \0".join("%r: %s" % (k, _ser(e)) for k, e in v.items()) + "}"
    if isinstance(v, (list, tuple)):
        body = ", \0".join(_ser(e) for e in v)
        return "[%s]" % body if isinstance(v, list) else "(%s%s)" % (body, "," if len(v) == 1 else "")
    return repr(v)


def format_expected(obs, width=190, indent=8):
    """The text of `EXPECTED = ...` in conv_wrapper_cases.py for an observe() result (python tests/test_conv_wrappers_host.py prints it):
    one entry per case, filled to `width`."""
    out = ["EXPECTED = {"]
    for n, r in obs.items():
        cur = "    %r: " % n
        for piece in (_ser(r) + ",").split("\0"):
            if len(cur) + len(piece.rstrip()) > width and cur.strip():
                out.append(cur.rstrip())
                cur = " " * indent
            cur += piece
        out.append(cur)
    return "\n".join(out + ["}"]) + "\n"


def named(v):
    """A record with its descriptors written out as {field: value} (the non-zero ones), for reading."""
    from retinanet_mi355x import _hip
    if isinstance(v, tuple) and v[:1] == ("D",):
        return {f[0]: e for f, e in zip(_hip.ConvDesc._fields_, v[1:]) if e not in (0, None)}
    if isinstance(v, dict):
        return {k: named(e) for k, e in v.items()}
    return type(v)(named(e) for e in v) if isinstance(v, (list, tuple)) else v


@pytest.fixture(scope="module")
def observed():
    return observe()


def test_wrappers_match_the_record(observed):
    assert set(observed) == set(C.EXPECTED)
    wrong = [n for n in observed if observed[n] != C.EXPECTED[n]]
    for n in wrong:
        got, exp = observed[n], C.EXPECTED[n]
        print("---- %s: %d calls, %d expected" % (n, len(got["calls"]), len(exp["calls"])))
        for i, (a, b) in enumerate(zip(got["calls"], exp["calls"])):
            if a != b:
                print("  call %d\n    got      %r\n    expected %r" % (i, named(a), named(b)))
        for key in ("returned", "carried"):
            if got[key] != exp[key]:
                print("  %s\n    got      %r\n    expected %r" % (key, got[key], exp[key]))
    assert not wrong, wrong


def test_the_record_repeats(observed):
    """Nothing in a record may depend on an address or on what ran before it."""
    assert observe() == observed


def test_the_table_reaches_every_wrapper(observed):
    """The record is worth something only if the table reaches each entry point and each kind the wrappers can produce."""
    calls = [c for r in observed.values() for c in r["calls"]]
    assert {c[0] for c in calls} == C.ENTRY_POINTS
    kinds = {c[2][0] for c in calls if c[2] is not None}
    assert {k.split(" ")[0] for k in kinds} == C.KIND_PREFIXES
    assert {k for k in kinds if " " in k} and {k for k in kinds if " " not in k}              # prof.BY_SHAPE on and off
    assert any(c[2] is None for c in calls if c[0] == "rn_conv_igemm")                         # ... and no timer at all
    groups = [c for c in calls if c[0].endswith("_grouped") and c[0].startswith("rn_conv_igemm")]
    assert {(c[0], c[1][0]["n"]) for c in groups} >= {(e, n) for e in C.GROUPED for n in (1, 3, 5)}
    assert {named(c[1][0]).get("w_format", 0) for c in calls if c[0] == "rn_conv_igemm"} == {0, 1, 2, 3}


if __name__ == "__main__":                          # after a deliberate change to what a wrapper hands the library: prints the new table
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-playground_amd"))
    sys.stdout.write(format_expected(observe()))

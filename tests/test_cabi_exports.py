"""CPU: the C-ABI library loads and exports every symbol include/retinanet_mi355x.h declares (no compute)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(REPO, "include", "retinanet_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rn_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from retinanet_mi355x import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "missing export " + n
    assert set(names) == set(_hip.SIGNATURES), set(names) ^ set(_hip.SIGNATURES)


# ---- the binding's three hand-kept mirrors of the header: _hip.SIGNATURES, the ctypes structures, the Python constants.
# The header is regular enough for a few regular expressions; a declaration that does not fit them fails the test.
def _header():
    src = open(os.path.join(REPO, "include", "retinanet_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


_SCALARS = {"int": "int", "int64_t": "int64_t", "float": "float", "double": "double", "uint64_t": "uint64_t",
            "unsigned long long": "uint64_t"}


def _c_kind(decl, named):
    """Kind of a C parameter ('const float *a', 'int B', 'double out[180]') or, named=False, of a return type."""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if named:
        assert len(words) >= 2 and re.fullmatch(r"[A-Za-z_]\w*", words[-1]), "parameter without a name: %r" % decl
        words = words[:-1]
    kind = "void" if words == ["void"] and not named else _SCALARS.get(" ".join(words))
    assert kind, "a type this test does not know: %r" % decl
    return kind


def _c_prototypes():
    """name -> (return kind, [parameter kinds]) of every function the header declares."""
    src = re.sub(r"^\s*#.*$", "", _header(), flags=re.M)
    src = re.sub(r"typedef\s+struct\s+\w+\s*\{[^{}]*\}\s*\w+\s*;", "", src)
    src = re.sub(r'extern\s+"C"\s*\{', "", src).replace("}", "")
    protos = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(rn_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        assert m, "not a function prototype: %r" % stmt
        ret, name, params = m.groups()
        assert name not in protos, name
        params = [] if params.strip() == "void" else [_c_kind(p, True) for p in params.split(",")]
        protos[name] = (_c_kind(ret, False), params)
    return protos


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_float: "float", ctypes.c_double: "double",
            ctypes.c_uint64: "uint64_t"}[t]


def test_signatures_agree_with_the_header_in_every_parameter():
    from retinanet_mi355x import _hip
    protos = _c_prototypes()
    assert len(protos) >= 177 and sorted(protos) == _declared() == sorted(_hip.SIGNATURES)
    for name, (res, args) in _hip.SIGNATURES.items():
        assert (_ctypes_kind(res), [_ctypes_kind(a) for a in args]) == protos[name], name


def test_structure_mirrors_list_the_header_s_fields_in_order():
    from retinanet_mi355x import _hip
    mirrors = {"rn_conv_desc": _hip.ConvDesc, "rn_conv_group": _hip.ConvGroup, "rn_prep_job": _hip.PrepJob,
               "rn_unpack_job": _hip.UnpackJob, "rn_wino_group": _hip.WinoGroup}
    bodies = dict(re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", _header()))
    assert set(mirrors) <= set(bodies)
    total = 0
    for name, mirror in mirrors.items():
        fields = []
        for stmt in bodies[name].split(";"):
            for decl in stmt.split(",") if stmt.strip() else []:
                m = re.search(r"([A-Za-z_]\w*)\s*(\[[^\]]*\])?\s*$", decl)
                assert m, "%s: not a field: %r" % (name, decl)
                fields.append(m.group(1))
        assert fields == [f[0] for f in mirror._fields_], name
        total += len(fields)
    assert total >= 100, total                         # 44 + 7 + 25 + 16 + 10 fields at the time of writing


def test_python_constants_equal_the_header_s_defines():
    from retinanet_mi355x import _hip, ops
    defines = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(RN_\w+)[ \t]+(.*?)[ \t]*$", _header(), flags=re.M):
        expr = re.sub(r"RN_\w+", lambda m: str(defines[m.group(0)]), expr)
        assert re.fullmatch(r"[0-9a-fA-FxX()<>+\-*|& ]+", expr), "%s is not an integer expression: %r" % (name, expr)
        defines[name] = eval(expr)
    checked = 0
    for mod in (ops, _hip):
        for attr, value in vars(mod).items():
            define = attr if attr.startswith("RN_") else "RN_" + attr
            if type(value) is int and define in defines:
                assert value == defines[define], "%s.%s = %d, the header's %s = %d" % (mod.__name__, attr, value, define, defines[define])
                checked += 1
    assert checked >= 80, checked


def test_host_helpers_without_gpu():
    """rn_anchor_count / rn_anchor_base_boxes are host code: check them against the oracle on CPU."""
    import numpy as np
    from oracle import anchors as oanchors
    from retinanet_mi355x import _hip
    lib = _hip.load()
    assert lib.rn_anchor_count(1080, 1920) == 389205
    assert lib.rn_anchor_count(512, 512) == oanchors.num_anchors(512, 512)
    buf = (ctypes.c_double * 180)()
    lib.rn_anchor_base_boxes(ctypes.cast(buf, ctypes.c_void_p))
    got = np.frombuffer(buf, dtype=np.float64).reshape(5, 9, 4)
    for li, lvl in enumerate(oanchors.PYRAMID_LEVELS):
        assert np.array_equal(got[li], oanchors.base_boxes(2 ** (lvl + 2)))       # bit-exact fp64
    assert lib.rn_version().startswith(b"retinanet_mi355x")


def test_ops_refuse_cpu_tensors():
    import torch
    from retinanet_mi355x import ops
    with pytest.raises(RuntimeError):
        ops.decode_dir(torch.zeros(1, 4, 4), torch.zeros(1, 4, 12))
    with pytest.raises(RuntimeError):
        ops.anchors(64, 64, "cpu")

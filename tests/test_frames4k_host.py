"""CPU: the 4K frame intake's host side (tests/frames4k_cases.py, 3d-playground_amd/timestamp_utilities.py, the C entries'
argument checks).  The numpy restatement of the time stamp reader equals what the reference's own parse_frame_timestamp
returned (tests/golden/frames4k.npz) bit for bit; make_checksums reproduces the cases' tables; the drop-in and both C
entry points refuse what they must before anything is launched; the ops refuse CPU tensors."""
import numpy as np
import pytest
import torch

import frames4k_cases as fc


def test_restatement_equals_the_reference_golden(golden):
    g = golden("frames4k")
    cases = fc.golden_cases()
    assert sorted(g.files) == sorted(c["name"] + "_" + k for c in cases for k in ("frame", "geom", "keys", "table", "time", "is_int", "err", "failed"))
    read = 0
    for c in cases:
        tag, geom = c["name"] + "_", c["geom"]
        assert np.array_equal(g[tag + "frame"], c["frame"])                     # the fixture's inputs are these builders'
        assert [int(v) for v in g[tag + "geom"]] == [geom[k] for k in fc.GEOMETRY_KEYS + ("h12",)]
        assert [str(k) for k in c["table"].keys()] == list(g[tag + "keys"])
        r = fc.parse_frames([c["frame"]], [(geom, c["table"])])
        assert r["times"].view(np.int64)[0] == g[tag + "time"].reshape(1).view(np.int64)[0], c["name"]
        assert bool(g[tag + "failed"]) == (r["status"][0] == fc.FAILED)
        assert bool(g[tag + "is_int"]) == (not g[tag + "failed"] and geom["n"] <= 10)
        if g[tag + "failed"]:
            j, w = int(r["fail_cell"][0]), geom["w"]
            assert np.array_equal(r["mask"][0][:, j * w:(j + 1) * w], g[tag + "err"]), c["name"]
        else:
            read += 1
            assert r["fail_cell"][0] == -1 and not g[tag + "err"].any()
    assert read >= 13 and len(cases) - read >= 6
    by_name = dict((c["name"], c) for c in cases)
    r = fc.parse_frames([by_name["duplicate_entry"]["frame"]], [(by_name["duplicate_entry"]["geom"], by_name["duplicate_entry"]["table"])])
    assert 2 in r["digits"][0] and 5 not in r["digits"][0]                      # glyph 1 reads as entry 2, never as its copy at 5
    for name, cell in (("flip_cell3", 3), ("flip_cell12", 12), ("flip_cells_5_8", 5), ("edge_past_right", 12), ("edge_past_bottom", 0)):
        c = by_name[name]
        assert fc.parse_frames([c["frame"]], [(c["geom"], c["table"])])["fail_cell"][0] == cell


def test_value_is_the_literal_bit_for_bit():
    digits = fc.random_digits(64, 15, seed=3)
    for n in (10, 11, 13, 16):
        for row in digits:
            text = fc.stamp_text(row, n)
            idx = [int(ch) if ch != "." else -1 for ch in text]
            assert fc.value(list(range(10)), idx, n).hex() == float(text).hex()


def test_every_font_and_geometry_gives_distinct_checksums_and_make_checksums_agrees():
    import timestamp_utilities as tsu
    for w, h in ((5, 9), (7, 11), (6, 10)):
        for font in (0, 1):
            for geom in (fc.geometry(w, h, 13), fc.geometry(w, h, 13, h13=0, w12=w)):
                want = fc.table(geom, font)
                got = tsu.make_checksums([fc.glyph(d, w, h, font) for d in range(10)], geom)
                assert list(got.keys()) == list(want.keys())
                assert all(np.array_equal(got[k], want[k]) and got[k].shape == (3, 2) for k in want)
                got = tsu.make_checksums(dict((str(d), torch.from_numpy(fc.glyph(d, w, h, font).astype(np.uint8) * 255)) for d in range(10)), geom)
                assert list(got.keys()) == [str(d) for d in range(10)] and all(np.array_equal(got[str(k)], want[k]) for k in want)
    geom = fc.geometry(7, 11, 13)
    with pytest.raises(ValueError, match="same six-area"):
        tsu.make_checksums([fc.glyph(1, 7, 11)] * 2, geom)
    with pytest.raises(ValueError, match="cell"):
        tsu.make_checksums([fc.glyph(1, 5, 9)], geom)


def test_drop_in_validation():
    import timestamp_utilities as tsu
    geom = fc.geometry(7, 11, 13)
    tab = fc.table(geom)
    with pytest.raises(ValueError, match="frame_pixels"):
        tsu.parse_frame_timestamp(geom, tab)
    frame = np.zeros((16, 100, 3), np.uint8)
    for key in (10, "a", "", 1.5, -1):
        bad = dict(tab)
        bad[key] = bad.pop(9)
        with pytest.raises(ValueError, match="decimal digit"):
            tsu.parse_frame_timestamp(geom, bad, frame_pixels=frame)
        with pytest.raises(ValueError, match="decimal digit"):
            tsu.TimestampReader([(geom, bad)], 2)
    for change in (dict(n=17), dict(n=0), dict(x0=-1), dict(y0=-2), dict(h13=8), dict(h23=12), dict(w12=8), dict(w=0), dict(h=600),
                   dict(h13=-1), dict(w12=-1)):
        with pytest.raises(ValueError, match="set 0"):
            tsu.TimestampReader([(dict(geom, **change), tab)], 1)
    with pytest.raises(ValueError, match="between 1 and 4"):
        tsu.TimestampReader([(geom, tab)] * 5, 1)
    with pytest.raises(ValueError, match="between 1 and 4"):
        tsu.TimestampReader([], 1)
    with pytest.raises(ValueError, match="table entries"):
        tsu.TimestampReader([(geom, dict(((k, 0), tab[0]) for k in range(65)))], 1)


GOOD_SET = (0, 0, 7, 11, 13, 3, 7, 3, 10)          # x0 y0 w h n h13 h23 w12 K


def _ts_call(lib, buf, sets=(GOOD_SET,), G=None, B=2, H=16, W=100, frame_stride=4800, row_stride=300, null=None):
    """rn_parse_frame_timestamps on host addresses that are never dereferenced: every call here is refused before a launch."""
    geo = np.array(sets, np.int32)
    p = dict((k, buf.ctypes.data) for k in ("frames", "tables", "times", "status", "set_index", "digits", "fail_cell"))
    if null:
        p[null] = None
    return lib.rn_parse_frame_timestamps(p["frames"], B, H, W, frame_stride, row_stride, 0, None if null == "sets" else geo.ctypes.data,
                                         len(sets) if G is None else G, p["tables"], None, p["times"], p["status"], p["set_index"],
                                         p["digits"], p["fail_cell"], None, None)


def test_c_entries_refuse_bad_arguments_without_launching():
    from retinanet_mi355x import _hip
    lib = _hip.load()
    EINVAL = 10001
    buf = np.zeros(64, np.uint8)

    def edit(**kw):
        s = dict(zip(("x0", "y0", "w", "h", "n", "h13", "h23", "w12", "K"), GOOD_SET))
        s.update(kw)
        return (tuple(s.values()),)
    for null in ("frames", "sets", "tables", "times", "status", "set_index", "digits", "fail_cell"):
        assert _ts_call(lib, buf, null=null) == EINVAL, null
    assert _ts_call(lib, buf, B=0) == EINVAL and _ts_call(lib, buf, B=-3) == EINVAL
    assert _ts_call(lib, buf, H=0) == EINVAL and _ts_call(lib, buf, W=0) == EINVAL
    for kw in (dict(n=17), dict(n=0), dict(K=0), dict(K=65), dict(x0=-1), dict(y0=-1), dict(h13=8), dict(h23=12), dict(h13=-1),
               dict(w12=8), dict(w12=-1), dict(w=0), dict(h=0), dict(w=64, h=65, h23=65, w12=64), dict(x0=(1 << 24) + 1)):
        assert _ts_call(lib, buf, sets=edit(**kw)) == EINVAL, kw
    assert _ts_call(lib, buf, G=0) == EINVAL and _ts_call(lib, buf, sets=(GOOD_SET,) * 5) == EINVAL
    assert _ts_call(lib, buf, sets=(GOOD_SET,) + edit(n=17)) == EINVAL         # a bad second set
    assert _ts_call(lib, buf, row_stride=299) == EINVAL and _ts_call(lib, buf, frame_stride=4799) == EINVAL

    def half(frames=buf.ctypes.data, B=1, H2=4, W2=6, layout=0, out=buf.ctypes.data):
        return lib.rn_frame_ingest_half(frames, B, H2, W2, 0, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, layout, out, None, None)
    for kw in (dict(frames=None), dict(out=None), dict(B=0), dict(H2=0), dict(W2=0), dict(H2=5), dict(W2=7), dict(H2=-2), dict(layout=2),
               dict(H2=1 << 17, W2=1 << 17)):
        assert half(**kw) == EINVAL, kw


def test_ops_refuse_cpu_tensors_and_operators_are_registered():
    from retinanet_mi355x import ops, torch_ops
    geom = fc.geometry(7, 11, 13)
    frames = torch.zeros((1, 16, 100, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.parse_frame_timestamps(frames, [(geom, fc.table(geom))])
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.frame_ingest_half(frames)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.load_frames_4k(frames, None)
    for name in ("frame_ingest_half", "parse_frame_timestamps"):
        assert name in torch_ops.OPERATORS
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty((3, 8, 64, 3), dtype=torch.uint8, device="cuda")
        x, u = torch.ops.retinanet_mi355x.frame_ingest_half(f, False, True)
        assert tuple(x.shape) == (3, 4, 32, 4) and tuple(u.shape) == (3, 4, 32, 3) and u.dtype == torch.uint8
        r = torch.ops.retinanet_mi355x.parse_frame_timestamps(f, list(GOOD_SET), torch.empty((1, 64, 8), dtype=torch.int32, device="cuda"), None, False)
        assert tuple(r[0].shape) == (3,) and r[0].dtype == torch.float64 and tuple(r[3].shape) == (3, 16) and tuple(r[5].shape) == (3, 11, 91)

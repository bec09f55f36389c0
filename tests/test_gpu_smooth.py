"""GPU: csrc/smooth.hip (ops.smooth_filter / smooth_rts), track_smooth.smooth_tracks and Data_Reader.smooth against the restatement
of tests/smooth_cases.py.

Bit for bit (fp64, one rounding per operation on both sides, the same order): filt, nis and out; exact: flag and the status word.
Both entry points go through ops.* and through torch.ops.retinanet_mi355x.*.

Shapes: tracklets of 1, 2, 3, 7, 130 and 150 rows; 1, 2, 3, 20 and 65 tracklets (a second wave with one lane, unequal lengths
inside a wave); flagged rows directly after the first row and as the last one, every row flagged, the gate off; the first 20
tracklets of the reference's shipped tracking output (tests/golden/track_stitch.npz)."""
import os

import numpy as np
import pytest
import torch

import smooth_cases as sc

pytestmark = pytest.mark.gpu


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ns(t):
    from retinanet_mi355x import ops, torch_ops     # noqa: F401  (registers torch.ops.retinanet_mi355x.*)
    return torch.ops.retinanet_mi355x if t else ops


def device_run(dev, offsets, cols, direction, model, gate, order=None, t=False):
    """Both entry points -> numpy arrays under the restatement's names."""
    o = _ns(t)
    order = sc.sorted_order(offsets) if order is None else np.asarray(order, np.int32)
    args = [_up(dev, a) for a in (offsets, order, cols, direction, model)]
    filt, nis, flag, st_f = o.smooth_filter(*args, float(gate), sc.DT_DEFAULT)
    out, st_r = o.smooth_rts(*args, sc.DT_DEFAULT, filt)
    got = {k: v.cpu().numpy() for k, v in dict(filt=filt, nis=nis, flag=flag, out=out).items()}
    got["status"] = int(st_f) | int(st_r)
    return got


def check(got, want):
    assert got["status"] == want["status"] == 0
    for key in ("filt", "nis", "out"):
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (key, np.abs(g - w).max(), int((g != w).sum()))
    assert got["flag"].dtype == np.uint8 and np.array_equal(got["flag"], want["flag"])


@pytest.fixture(scope="module")
def scenes(golden):
    """name -> (offsets, cols, direction, model, gate) and, computed once, the restatement's result."""
    out = {"exact": sc.exact_scene() + (sc.full_model(), sc.GATE), "noisy": sc.noisy_scene()[:3] + (sc.NOISY_MODEL, sc.GATE),
           "golden20": sc.golden_scene(golden("track_stitch")) + (sc.NOISY_MODEL, sc.GATE)}
    for name, (o, c, d, gate) in sc.edge_scenes().items():
        out[name] = (o, c, d, sc.NOISY_MODEL, gate)
    return {k: (v, sc.smooth(*v[:4], gate=v[4])) for k, v in out.items()}


NAMES = ("exact", "noisy", "golden20", "short", "mixed65", "flag_ends", "all_flagged", "gate_off", "direction_zero")


@pytest.mark.parametrize("t", [False, True], ids=["ops", "torch_ops"])
@pytest.mark.parametrize("name", NAMES)
def test_both_passes_bit_for_bit(dev, scenes, name, t):
    (o, c, d, model, gate), want = scenes[name]
    got = device_run(dev, o, c, d, model, gate, t=t)
    check(got, want)
    if name == "exact":
        assert got["out"][:, :6].tobytes() == c[:, 1:7].tobytes() and not got["flag"].any() and (got["out"][:, 5] == 96.0).all()
    if name == "flag_ends":
        assert got["flag"].nonzero()[0].tolist() == [1, 17]
    if name == "all_flagged":
        assert int(got["flag"].sum()) == len(c) - (len(o) - 1)
    if name == "gate_off":
        assert not got["flag"].any() and got["nis"].max() > sc.GATE


def test_any_lane_order_gives_the_same_bytes(dev, scenes):
    (o, c, d, model, gate), want = scenes["mixed65"]
    N = len(o) - 1
    assert not np.array_equal(sc.sorted_order(o), np.arange(N))
    for order in (np.arange(N), np.arange(N)[::-1], np.random.default_rng(3).permutation(N)):
        check(device_run(dev, o, c, d, model, gate, order=order), want)


def test_noisy_scene_on_the_device(dev, scenes):
    (o, c, d, model, gate), _ = scenes["noisy"]
    sc.check_noisy(o, c, sc.noisy_scene()[3], device_run(dev, o, c, d, model, gate))


# ------------------------------------------------------------------------------------------------ refusals
def _kf(Q=sc.NOISY_Q, R=sc.NOISY_R, P=sc.NOISY_P0):
    return {"Q": torch.from_numpy(np.array(Q)), "R": torch.from_numpy(np.array(R)), "P": torch.from_numpy(np.array(P))}


def _reader(dev, tmp_path, data):
    import datareader
    import datareader_cases as dc
    import homography
    hg = homography.Homography()
    hg.correspondence = {"p1c1": {"P": dc.cameras()[1][2]}}
    hg.default_correspondence = "p1c1"
    path = os.path.join(str(tmp_path), "in.csv")
    with open(path, "w", newline="") as f:
        f.write(dc.csv_text([dc.HEADER + ["ts_bias for cameras ['p1c1']"]]))
    dr = datareader.Data_Reader(path, hg)
    assert dr.data == []
    dr.data = data
    return dr


@pytest.mark.parametrize("name", ["nan", "empty", "repeat", "indefinite"])
def test_every_status_bit_raises_and_nothing_is_replaced(dev, tmp_path, name):
    import track_smooth
    from retinanet_mi355x import ops
    o, c, d, model, bit = sc.refusal_scenes()[name]
    args = [_up(dev, a) for a in (o, sc.sorted_order(o), c, d, model)]
    filt, nis, flag, status = ops.smooth_filter(*args, sc.GATE, sc.DT_DEFAULT)
    out, status = ops.smooth_rts(*args, sc.DT_DEFAULT, filt, status=status)
    assert int(status) == bit == sc.smooth(o, c, d, model)["status"]
    with pytest.raises(RuntimeError, match=r"status %d\b" % bit):
        ops.smooth_check(status)
    with pytest.raises(RuntimeError, match="refused"):
        track_smooth.smooth_packed(o, c, d, model, track_smooth.resolve_params(), dev)
    if name in ("nan", "indefinite"):                                               # the two that ``data`` dicts can express
        data = sc.as_data(o, c, d)
        before = [{k: dict(v) for k, v in f.items()} for f in data]
        dr = _reader(dev, tmp_path, data)
        dr.d_idx = 3
        kf = _kf(Q=model[:36].reshape(6, 6).astype(np.float32))
        with pytest.raises(RuntimeError, match="refused"):
            dr.smooth(kf, save=os.path.join(str(tmp_path), "never.csv"))
        assert dr.data is data and dr.d_idx == 3 and not os.path.exists(os.path.join(str(tmp_path), "never.csv"))
        assert repr(data) == repr(before)                                           # repr: a NaN is not equal to itself


# ------------------------------------------------------------------------------------------------ end to end
def test_smooth_tracks_and_data_reader_on_the_noisy_scene(dev, tmp_path):
    import track_smooth
    import track_stitch
    import datareader_cases as dc
    o, c, d, truth = sc.noisy_scene()
    data = sc.as_data(o, c, d)
    before = [{k: dict(v) for k, v in f.items()} for f in data]
    new, report = track_smooth.smooth_tracks(data, _kf(), device=dev)
    assert data == before                                                           # the input is unmodified
    pk, pk_new = track_stitch.pack_tracklets(data), track_stitch.pack_tracklets(new)
    assert np.array_equal(pk["ids"], pk_new["ids"]) and np.array_equal(pk["offsets"], pk_new["offsets"])   # ids, rows per id
    assert pk["cols"][:, 0].tobytes() == pk_new["cols"][:, 0].tobytes() and np.array_equal(pk["frame"], pk_new["frame"])
    assert [list(f) for f in new] == [list(f) for f in data] and all(k == v["id"] for f in new for k, v in f.items())
    assert all(type(v[k]) is float for f in new for v in f.values() for k in ("x", "y", "l", "w", "h", "v"))
    assert all(a[k] == b[k] for fa, fb in zip(new, data) for a, b in zip(fa.values(), fb.values())
               for k in ("id", "timestamp", "class", "camera", "direction", "ts_bias", "frame"))
    assert report["status"] == 0 and np.array_equal(report["ids"], pk["ids"]) and np.array_equal(report["offsets"], o)
    assert report["direction"].tolist() == [1, -1] * 10 and report["var"].shape == (3000, 6) and report["filtered"].shape == (3000, 27)
    # the time stamps of ``data`` are rounded to 1e-4 s: the restatement on the packed arrays, then the scene's inequalities
    want = sc.smooth(pk["offsets"], pk["cols"], pk["direction"], sc.NOISY_MODEL)
    assert pk_new["cols"][:, 1:].tobytes() == want["out"][:, :6].tobytes() and report["var"].tobytes() == want["out"][:, 6:].tobytes()
    assert report["filtered"].tobytes() == want["filt"].tobytes() and report["nis"].tobytes() == want["nis"].tobytes()
    res = dict(status=report["status"], flag=report["flag"], filt=report["filtered"], out=np.concatenate((pk_new["cols"][:, 1:], report["var"]), axis=1))
    sc.check_noisy(pk["offsets"], pk["cols"], truth, res)
    dr = _reader(dev, tmp_path, data)
    dr.d_idx = 5
    path = os.path.join(str(tmp_path), "smoothed.csv")
    rep = dr.smooth(_kf(), save=path)
    assert dr.d_idx == 0 and dr.data is not data and dr.data == new and rep["flag"].tobytes() == report["flag"].tobytes()
    with open(path, newline="") as f:
        rows = len(dc.parse(f.read()))
    assert 1 < rows <= 1 + 3000                                                     # write_to_file ran: the header and the kept rows
    off = dr.smooth(_kf(), {"gate": 0})
    assert not off["flag"].any()
    empty, rep = track_smooth.smooth_tracks([], _kf(), device=dev)
    assert empty == [] and rep["status"] == 0 and len(rep["ids"]) == 0 and rep["var"].shape == (0, 6) and rep["filtered"].shape == (0, 27)
    with pytest.raises(ValueError):
        dr.smooth(_kf(), {"gates": 1})


def test_stitch_then_smooth(dev, tmp_path):
    data = sc.fragments()
    dr = _reader(dev, tmp_path, data)
    link = dr.stitch()
    assert len(link["links"]) == 1 and {k for f in dr.data for k in f} == {11}
    stitched = dr.data
    n = sum(len(f) for f in stitched)
    assert n >= 50 + 9                                                              # the gap of 10 frames is filled
    report = dr.smooth(_kf())
    assert report["ids"].tolist() == [11] and report["offsets"].tolist() == [0, n] and report["status"] == 0
    assert [list(f) for f in dr.data] == [list(f) for f in stitched]
    filled = [(a[11], b[11]) for a, b in zip(stitched, dr.data) if 100.0 + 19.5 / 30 < a[11]["timestamp"] < 100.0 + 29.5 / 30]
    assert len(filled) >= 9
    for a, b in filled:                                                             # the filled rows are smoothed like any other
        assert b["timestamp"] == a["timestamp"] and b["x"] != a["x"] and abs(b["x"] - a["x"]) < 2.0 and abs(b["v"] - 95.0) < 5.0
    x = np.array([f[11]["x"] for f in dr.data])
    t = np.array([f[11]["timestamp"] for f in dr.data])
    raw = np.array([f[11]["x"] for f in stitched])
    line = 300.0 + 95.0 * (t - 100.0)
    print("RMSE against the line: stitched %.3f, smoothed %.3f" % (np.sqrt(((raw - line) ** 2).mean()), np.sqrt(((x - line) ** 2).mean())))
    assert ((x - line) ** 2).mean() < ((raw - line) ** 2).mean()

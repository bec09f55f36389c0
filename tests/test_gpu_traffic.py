"""GPU: csrc/traffic.hip (ops.traffic_lanes / traffic_cells / traffic_leaders), traffic_state.traffic_fields / car_following and
Data_Reader.traffic_state against the restatement of tests/traffic_cases.py.

Exact: dir, lane, T, D, n, the counters, leader and the status word (T and D are integer sums: the order of the atomics cannot
show).  Byte for byte: spacing, gap, headway and ttc, infinities included (fp64, one rounding per operation on both sides).  Every
entry point goes through ops.* and through torch.ops.retinanet_mi355x.*.

Shapes: the closed form (12 tracklets of 513 rows: 6 156 segments, 25 workgroups); one tracklet per edge of the cell rule; 65 and
300 segments in one tracklet and 65 short tracklets; frames of 0, 1, 2, 65 and 300 rows (the last past one LDS tile); all 6 806 rows
of the reference's shipped tracking output (tests/golden/track_stitch.npz)."""
import os

import numpy as np
import pytest
import torch

import traffic_cases as tc

pytestmark = pytest.mark.gpu


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ns(t):
    from retinanet_mi355x import ops, torch_ops     # noqa: F401  (registers torch.ops.retinanet_mi355x.*)
    return torch.ops.retinanet_mi355x if t else ops


def _edges(dev, edges=tc.DEFAULT_EDGES):
    return [_up(dev, np.asarray(edges[s], np.float64)) for s in (1, -1)]


def device_cells(dev, offsets, cols, direction, grid, max_gap, t=False):
    o = _ns(t)
    d_off, d_cols, d_dir = (_up(dev, a) for a in (offsets, cols, direction))
    ep, en = _edges(dev)
    tdir, lane, st_l = o.traffic_lanes(d_off, d_cols, d_dir, ep, en)
    T, D, n, counters, st_c = o.traffic_cells(d_off, d_cols, tdir, ep, en, *grid, max_gap)
    got = {k: v.cpu().numpy() for k, v in dict(dir=tdir, lane=lane, T=T, D=D, n=n).items()}
    got["counters"] = dict(zip(tc.CELL_COUNTERS, counters.cpu().tolist()))
    assert counters.cpu().tolist()[6:] == [0, 0]
    got["status"] = int(st_l) | int(st_c)
    return got


def device_leaders(dev, offsets, cols, direction, frame_off, frame_rows, t=False):
    o = _ns(t)
    d_off, d_cols, d_dir, d_foff, d_frows = (_up(dev, a) for a in (offsets, cols, direction, frame_off, frame_rows))
    ep, en = _edges(dev)
    tdir, lane, st_l = o.traffic_lanes(d_off, d_cols, d_dir, ep, en)
    leader, spacing, gap, headway, ttc, counters, st = o.traffic_leaders(d_off, d_cols, tdir, lane, d_foff, d_frows)
    got = {k: v.cpu().numpy() for k, v in dict(dir=tdir, lane=lane, leader=leader, spacing=spacing, gap=gap, headway=headway, ttc=ttc).items()}
    got["with_leader"], got["overlaps"] = counters.cpu().tolist()[:2]
    assert counters.cpu().tolist()[2:] == [0] * 6
    got["status"] = int(st_l) | int(st)
    return got


def check_cells(got, want):
    assert got["status"] == want["status"] == 0
    for key, dtype in (("dir", np.int32), ("lane", np.int32), ("T", np.int64), ("D", np.int64), ("n", np.int32)):
        assert got[key].dtype == dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    assert got["counters"] == want["counters"]


def check_leaders(got, want):
    assert got["status"] == want["status"] == 0
    for key in ("dir", "lane", "leader"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
    for key in ("spacing", "gap", "headway", "ttc"):
        assert got[key].dtype == np.float64 and got[key].tobytes() == want[key].tobytes(), key
    assert (got["with_leader"], got["overlaps"]) == (want["with_leader"], want["overlaps"])


@pytest.fixture(scope="module")
def scenes(golden):
    """name -> dict(offsets, cols, direction, and where the scene has them: grid, max_gap, cells = the restatement's fields;
    frame_off, frame_rows, leaders = the restatement's leaders), computed once."""
    out = {}
    o, c, d, frame = tc.closed_form_scene()
    out["closed"] = dict(offsets=o, cols=c, direction=d, frame=frame, grid=tc.derive_grid(c, 64.0, 2.0), max_gap=1.0)
    o, c, d, _ = tc.cell_edge_scene()
    out["edges"] = dict(offsets=o, cols=c, direction=d, grid=tc.EDGE_GRID, max_gap=tc.EDGE_MAX_GAP)
    o, c, d, frame = tc.many_scene()
    out["many"] = dict(offsets=o, cols=c, direction=d, frame=frame, grid=tc.derive_grid(c, 50.0, 2.0), max_gap=1.0)
    o, c, d, frame = tc.golden_scene(golden("track_stitch"))
    out["golden"] = dict(offsets=o, cols=c, direction=d, frame=frame, grid=tc.derive_grid(c, 50.0, 2.0), max_gap=1.0)
    o, c, d, frame_off, frame_rows = tc.leader_edge_scene()
    out["frames"] = dict(offsets=o, cols=c, direction=d, frame_off=frame_off, frame_rows=frame_rows)
    for s in out.values():
        tdir, lane, status = tc.lanes(s["offsets"], s["cols"], s["direction"], tc.DEFAULT_EDGES)
        assert status == 0
        if "frame" in s:
            s["frame_off"], s["frame_rows"] = tc.frames_csr(s["frame"])
        if "grid" in s:
            s["cells"] = dict(tc.cells(s["offsets"], s["cols"], tdir, tc.DEFAULT_EDGES, s["grid"], s["max_gap"]), dir=tdir, lane=lane)
        if "frame_off" in s:
            s["leaders"] = dict(tc.leaders(s["offsets"], s["cols"], tdir, lane, s["frame_off"], s["frame_rows"]), dir=tdir, lane=lane)
    return out


@pytest.mark.parametrize("t", [False, True], ids=["ops", "torch_ops"])
@pytest.mark.parametrize("name", ["closed", "edges", "many", "golden"])
def test_lanes_and_cells_exact(dev, scenes, name, t):
    s = scenes[name]
    got = device_cells(dev, s["offsets"], s["cols"], s["direction"], s["grid"], s["max_gap"], t=t)
    check_cells(got, s["cells"])
    if name == "closed":
        c = tc.CLOSED
        for it, ix in tc.closed_form_interior(s["grid"]):
            T, D = int(got["T"][0, 0, it, ix]), int(got["D"][0, 0, it, ix])
            assert T / (tc.Q * c["dx"] * c["dt"]) == 1 / 128 and D / T == 64.0 and D / (tc.Q * c["dx"] * c["dt"]) == 0.5
    if name == "edges":
        assert got["counters"]["outside"] == 3 and got["counters"]["skipped_gap"] == 4 and got["counters"]["skipped_lane"] == 1
    if name == "golden":
        assert {k: got["counters"][k] for k in tc.GOLDEN_COUNTS} == tc.GOLDEN_COUNTS and int((got["n"] > 0).sum()) == 575


@pytest.mark.parametrize("t", [False, True], ids=["ops", "torch_ops"])
@pytest.mark.parametrize("name", ["closed", "many", "golden", "frames"])
def test_leaders_byte_for_byte(dev, scenes, name, t):
    s = scenes[name]
    got = device_leaders(dev, s["offsets"], s["cols"], s["direction"], s["frame_off"], s["frame_rows"], t=t)
    check_leaders(got, s["leaders"])
    has = got["leader"] >= 0
    if name == "closed":
        assert (got["spacing"][has] == 128.0).all() and (got["headway"][has] == 2.0).all() and np.isinf(got["ttc"]).all()
        assert int(has.sum()) == 11 * 449
    if name == "frames":
        assert s["leaders"]["ties"] > 0 and got["overlaps"] > 0 and np.isinf(got["spacing"][~has]).all() and np.isinf(got["gap"][~has]).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_a_nan_raises_the_status_word(dev, scenes):
    import traffic_state
    from retinanet_mi355x import ops
    s = scenes["many"]
    cols = s["cols"].copy()
    cols[70, 1] = np.nan                                                             # x of a row inside the 301-row tracklet
    got = device_cells(dev, s["offsets"], cols, s["direction"], s["grid"], s["max_gap"])
    assert got["status"] == ops.TRAFFIC_NONFINITE == tc.cells(s["offsets"], cols, got["dir"], tc.DEFAULT_EDGES, s["grid"], s["max_gap"])["status"]
    lead = device_leaders(dev, s["offsets"], cols, s["direction"], s["frame_off"], s["frame_rows"])
    assert lead["status"] == ops.TRAFFIC_NONFINITE and lead["leader"][70] == -1 and not (lead["leader"] == 70).any()
    cols[70, 1] = np.inf
    d_off, d_cols, d_dir = (_up(dev, a) for a in (s["offsets"], cols, s["direction"]))
    _, _, status = ops.traffic_lanes(d_off, d_cols, d_dir, *_edges(dev))
    with pytest.raises(RuntimeError, match=r"refused.*status 1\b"):
        ops.traffic_check(status)
    data = tc.as_data_frames(s["offsets"], cols, s["direction"], np.arange(len(s["offsets"]) - 1), s["frame"])
    for fn in (traffic_state.traffic_fields, traffic_state.car_following):
        with pytest.raises(RuntimeError, match="refused"):
            fn(data, {"dx": 50.0, "dt": 2.0}, dev)


def test_other_status_bits_equal_the_restatement(dev):
    from retinanet_mi355x import ops
    offsets, cols, direction = tc.pack([[tc.row(100, 0), tc.row(100.5, 10)], [tc.row(100, 0), tc.row(100.5, 1e7)]], [1, 1])
    tdir = np.array([1, 1], np.int32)
    ep, en = _edges(dev)

    def status(cols, tdir, grid):
        out = ops.traffic_cells(_up(dev, offsets), _up(dev, cols), _up(dev, tdir), ep, en, *grid, 1.0)
        want = tc.cells(offsets, cols, tdir, tc.DEFAULT_EDGES, grid, 1.0)
        assert out[3].cpu().tolist()[:6] == [want["counters"][k] for k in tc.CELL_COUNTERS] and np.array_equal(out[0].cpu().numpy(), want["T"])
        assert int(out[4]) == want["status"]
        return int(out[4])
    assert status(cols, tdir, tc.EDGE_GRID) == ops.TRAFFIC_RANGE
    cols[3, 1] = 1e6
    assert status(cols, tdir, (100.0, 2.0, 6, 0.0, 64.0, 6)) == ops.TRAFFIC_TOO_MANY_CUTS
    assert status(cols, np.array([1, 0], np.int32), tc.EDGE_GRID) == ops.TRAFFIC_BAD_DIR
    bad = ops.traffic_lanes(_up(dev, np.array([0, 3, 2], np.int64)), _up(dev, cols), _up(dev, direction), ep, en)
    assert int(bad[2]) & ops.TRAFFIC_BAD_OFFSETS
    tdir_d, lane_d, _ = ops.traffic_lanes(_up(dev, offsets), _up(dev, cols), _up(dev, direction), ep, en)
    out = ops.traffic_leaders(_up(dev, offsets), _up(dev, cols), tdir_d, lane_d, _up(dev, np.array([0, 2], np.int64)), _up(dev, np.array([0, 9], np.int32)))
    assert int(out[6]) == ops.TRAFFIC_BAD_FRAME and out[0].cpu().tolist() == [-1] * 4
    out = ops.traffic_leaders(_up(dev, offsets), _up(dev, cols), tdir_d, lane_d, _up(dev, np.array([0, 5], np.int64)), _up(dev, np.array([0, 1], np.int32)))
    assert int(out[6]) == ops.TRAFFIC_BAD_FRAME


# ------------------------------------------------------------------------------------------------ end to end
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


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        elif isinstance(a[k], dict) and k == "lane_edges":
            assert all(np.array_equal(a[k][s], b[k][s]) for s in (1, -1))
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("name", ["closed", "golden"])
def test_traffic_state_end_to_end(dev, tmp_path, scenes, golden, name):
    import track_stitch
    import traffic_state
    s = scenes[name]
    params = {"dx": 64.0, "dt": 2.0} if name == "closed" else dict(tc.GOLDEN_PARAMS)
    ids = np.arange(100, 112) if name == "closed" else golden("track_stitch")["ids"]
    data = tc.as_data_frames(s["offsets"], s["cols"], s["direction"], ids, s["frame"])
    before = [{k: dict(v) for k, v in f.items()} for f in data]
    pk = track_stitch.pack_tracklets(data)
    assert np.array_equal(pk["offsets"], s["offsets"]) and pk["cols"].tobytes() == s["cols"].tobytes() and np.array_equal(pk["frame"], s["frame"])
    fields = traffic_state.traffic_fields(data, params, dev)
    follow = traffic_state.car_following(data, params, dev)
    assert data == before                                                           # the input is unmodified
    want, lead = s["cells"], s["leaders"]
    g = fields["grid"]
    assert (g["t0"], g["dt"], g["nt"], g["x0"], g["dx"], g["nx"]) == s["grid"]
    for key in ("T", "D", "n"):
        assert fields[key].dtype == want[key].dtype and np.array_equal(fields[key], want[key])
    assert fields["counters"] == want["counters"]
    area = tc.Q * g["dx"] * g["dt"]
    T, D = want["T"].astype(np.float64), want["D"].astype(np.float64)
    assert fields["density"].tobytes() == (T / area).tobytes() and fields["flow"].tobytes() == (D / area).tobytes()
    assert np.array_equal(np.isnan(fields["speed"]), want["T"] == 0) and np.array_equal(fields["speed"][want["T"] > 0], (D / np.where(T > 0, T, 1))[want["T"] > 0])
    assert np.array_equal(follow["ids"], pk["ids"]) and np.array_equal(follow["offsets"], pk["offsets"]) and np.array_equal(follow["frame"], pk["frame"])
    assert np.array_equal(follow["dir"], lead["dir"]) and np.array_equal(follow["lane"], lead["lane"]) and np.array_equal(follow["leader"], lead["leader"])
    trk = np.repeat(np.arange(len(pk["ids"])), np.diff(pk["offsets"]))
    assert follow["leader_id"].dtype == np.int64
    assert np.array_equal(follow["leader_id"], np.where(lead["leader"] >= 0, pk["ids"][trk[np.maximum(lead["leader"], 0)]], -1))
    for key in ("spacing", "gap", "headway", "ttc"):
        assert follow[key].tobytes() == lead[key].tobytes(), key
    assert (follow["with_leader"], follow["overlaps"]) == (lead["with_leader"], lead["overlaps"])
    spread = max(max(v["timestamp"] for v in f.values()) - min(v["timestamp"] for v in f.values()) for f in data if f)
    assert follow["frame_spread"] == spread == 0.0
    if name == "closed":                                                            # a frame that is not one instant shows
        late = [{k: dict(v) for k, v in f.items()} for f in data[:80]]
        late[70][100]["timestamp"] += 0.25
        assert traffic_state.car_following(late, params, dev)["frame_spread"] == 0.25
    if name == "closed":
        inner = tuple(zip(*tc.closed_form_interior(s["grid"])))
        assert (fields["density"][0, 0][inner] == 1 / 128).all() and (fields["speed"][0, 0][inner] == 64.0).all() and (fields["flow"][0, 0][inner] == 0.5).all()
    dr = _reader(dev, tmp_path, data)
    dr.d_idx = 3
    first = dr.traffic_state(params)
    second = dr.traffic_state(params)
    assert dr.data is data and dr.d_idx == 3 and data == before and set(first) == {"fields", "following"}
    for part, direct in (("fields", fields), ("following", follow)):
        _same(first[part], direct)
        _same(second[part], first[part])


def test_empty_data_and_bad_parameters(dev):
    import traffic_state
    fields = traffic_state.traffic_fields([], None, dev)
    assert fields["T"].shape == (2, 5, 0, 0) and fields["counters"]["segments"] == 0 and fields["speed"].shape == (2, 5, 0, 0)
    follow = traffic_state.car_following([{}, {}], None, dev)
    assert len(follow["ids"]) == 0 and follow["leader_id"].shape == (0,) and follow["overlaps"] == 0 and follow["frame_spread"] == 0.0
    with pytest.raises(ValueError):
        traffic_state.traffic_fields([], {"dz": 1.0}, dev)
    with pytest.raises(RuntimeError):
        traffic_state.traffic_fields([], None, "cpu")

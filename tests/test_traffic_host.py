"""CPU: the restatement of tests/traffic_cases.py against the closed form, the conservation rule and the counts of the shipped
tracking output; traffic_state's parameters and grid; the operators' registration and their refusal of CPU tensors."""
import numpy as np
import pytest

import traffic_cases as tc


def _cells(offsets, cols, direction, grid, max_gap, edges=tc.DEFAULT_EDGES):
    d, lane, status = tc.lanes(offsets, cols, direction, edges)
    assert status == 0
    return d, lane, tc.cells(offsets, cols, d, edges, grid, max_gap)


def _conserved(res):
    """Without outside pieces the cells hold every used segment's time and distance, up to half a quantum per piece."""
    assert res["counters"]["outside"] == 0
    pieces = res["counters"]["pieces"]
    assert int(res["n"].sum()) == pieces
    for got, whole in zip((res["T"], res["D"]), res["whole"]):
        assert 2 * abs(sum(int(v) for v in got.reshape(-1)) - whole) <= pieces


# ------------------------------------------------------------------------------------------------ closed form
def test_closed_form_fields_and_following():
    offsets, cols, direction, frame = tc.closed_form_scene()
    c = tc.CLOSED
    grid = tc.derive_grid(cols, c["dx"], c["dt"])
    assert grid == (1024.0, 2.0, 20, 0.0, 64.0, 17)
    d, lane, res = _cells(offsets, cols, direction, grid, 1.0)
    assert res["status"] == 0 and (d == 1).all() and (lane == 0).all()
    assert res["counters"] == dict(segments=12 * 512, used=12 * 512, skipped_gap=0, skipped_lane=0, pieces=12 * 512, outside=0)
    _conserved(res)
    interior = tc.closed_form_interior(grid)
    assert len(interior) == 12 * 16
    T, D = res["T"][0, 0], res["D"][0, 0]
    for it, ix in interior:
        assert T[it, ix] / (tc.Q * c["dx"] * c["dt"]) == 1 / 128 and D[it, ix] / T[it, ix] == 64.0 and D[it, ix] / (tc.Q * c["dx"] * c["dt"]) == 0.5
        assert res["n"][0, 0, it, ix] == 32
    assert int(T.sum()) == sum(int(T[c]) for c in interior) and not res["T"][1].any() and not res["T"][0, 1:].any()
    frame_off, frame_rows = tc.frames_csr(frame)
    lead = tc.leaders(offsets, cols, d, lane, frame_off, frame_rows)
    has = lead["leader"] >= 0
    trk = np.repeat(np.arange(12), np.diff(offsets))
    assert lead["status"] == 0 and lead["with_leader"] == int(has.sum()) == 11 * (512 - 64 + 1) and lead["overlaps"] == 0 and lead["ties"] == 0
    assert (trk[lead["leader"][has]] == trk[has] - 1).all() and not has[trk == 0].any()
    assert (lead["spacing"][has] == 128.0).all() and (lead["headway"][has] == 2.0).all() and (lead["gap"][has] == 112.0).all()
    assert np.isinf(lead["ttc"]).all() and np.isinf(lead["spacing"][~has]).all()


# ------------------------------------------------------------------------------------------------ the cell rule at its edges
def test_cell_rule_edge_by_edge():
    offsets, cols, direction, names = tc.cell_edge_scene()
    d, lane, _ = tc.lanes(offsets, cols, direction, tc.DEFAULT_EDGES)
    assert d[names.index("other_direction")] == -1 and d[names.index("direction_zero")] == 1

    def one(name, max_gap=tc.EDGE_MAX_GAP):
        i = names.index(name)
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        res = tc.cells(np.array([0, hi - lo]), cols[lo:hi], d[i:i + 1], tc.DEFAULT_EDGES, tc.EDGE_GRID, max_gap)
        assert res["status"] == 0
        cells = {tuple(int(v) for v in k): (int(res["T"][tuple(k)]), int(res["D"][tuple(k)]), int(res["n"][tuple(k)])) for k in np.argwhere(res["n"])}
        return res["counters"], cells

    q = tc.Q
    assert one("one_row") == (dict(segments=0, used=0, skipped_gap=0, skipped_lane=0, pieces=0, outside=0), {})
    assert one("no_cut")[1] == {(0, 0, 0, 0): (q // 2, 10 * q, 1)}
    assert one("time_cut")[1] == {(0, 0, 0, 1): (q // 2, 15 * q, 1), (0, 0, 1, 1): (q // 2, 15 * q, 1)}
    assert one("x_cut")[1] == {(0, 0, 1, 0): (q // 5, 4 * q, 1), (0, 0, 1, 1): (3 * q // 10 + 1, 6 * q, 1)}
    c, cells = one("both_cuts_same_s")                                              # the empty piece between the two cuts is dropped
    assert c["pieces"] == 2 and cells == {(0, 0, 0, 0): (q // 2, 16 * q, 1), (0, 0, 1, 1): (q // 2, 16 * q, 1)}
    c, cells = one("eight_pieces")
    assert c["pieces"] == 8 and len(cells) == 8 and sum(v[0] for v in cells.values()) in range(7 * q - 4, 7 * q + 5)
    assert one("no_motion")[1] == {(0, 0, 1, 1): (q, 0, 1), (0, 0, 2, 1): (q, 0, 1)}
    c, cells = one("backwards")                                                     # X < 0 under direction +1: |X| is travelled
    assert c["pieces"] == 3 and set(cells) == {(0, 0, 2, 3), (0, 0, 2, 2), (0, 0, 2, 1)} and sum(v[1] for v in cells.values()) == 100 * q
    assert one("on_grid_lines") == (dict(segments=1, used=1, skipped_gap=0, skipped_lane=0, pieces=1, outside=0), {(0, 0, 1, 1): (q, 64 * q, 1)})
    assert set(one("ym_on_an_edge")[1]) == {(0, 1, 3, 0)}
    assert one("ym_on_the_last_edge")[0] == dict(segments=1, used=0, skipped_gap=0, skipped_lane=1, pieces=0, outside=0)
    c, cells = one("outside_in_x")
    assert (c["pieces"], c["outside"]) == (2, 1) and set(cells) == {(0, 0, 4, 5)}
    c, cells = one("outside_late")
    assert (c["pieces"], c["outside"]) == (2, 1) and set(cells) == {(0, 0, 5, 0)}
    c, cells = one("outside_early")
    assert (c["pieces"], c["outside"]) == (2, 1) and set(cells) == {(0, 0, 0, 0)}
    c, cells = one("bad_stamps")                                                    # -1 -> -1, -1 -> 105, 105 -> 105 are skipped
    assert (c["segments"], c["used"], c["skipped_gap"]) == (4, 1, 3) and set(cells) == {(0, 0, 2, 0)}
    assert one("too_far_apart")[0]["skipped_gap"] == 1 and one("too_far_apart", max_gap=8.5)[0]["used"] == 1
    assert set(one("other_direction")[1]) == {(1, 0, 1, 4), (1, 0, 1, 3)}
    assert set(one("direction_zero")[1]) == {(0, 0, 4, 2)}
    whole = tc.cells(offsets, cols, d, tc.DEFAULT_EDGES, tc.EDGE_GRID, tc.EDGE_MAX_GAP)
    assert whole["counters"]["outside"] == 3 and whole["counters"]["segments"] == len(cols) - len(names) and whole["max_pieces"] == 8


def test_refusals_of_the_restatement():
    offsets, cols, direction = tc.pack([[tc.row(100, 0), tc.row(100.5, float("nan"))], [tc.row(100, 0), tc.row(100.5, 1e7)]], [1, 1])
    d = np.array([1, 1], np.int32)
    assert tc.lanes(offsets, cols, direction, tc.DEFAULT_EDGES)[2] == tc.NONFINITE
    assert tc.cells(offsets, cols, d, tc.DEFAULT_EDGES, tc.EDGE_GRID, 1.0)["status"] == tc.NONFINITE | tc.RANGE
    cols[1, 1] = 10.0
    cols[3, 1] = 1e6
    assert tc.cells(offsets, cols, d, tc.DEFAULT_EDGES, (100.0, 2.0, 6, 0.0, 64.0, 6), 1.0)["status"] == tc.TOO_MANY_CUTS
    assert tc.cells(offsets, cols, np.array([1, 0], np.int32), tc.DEFAULT_EDGES, tc.EDGE_GRID, 1.0)["status"] == tc.BAD_DIR


def test_conservation_on_the_scenes_without_outside_pieces(golden):
    for offsets, cols, direction, _ in (tc.many_scene(), tc.golden_scene(golden("track_stitch"))):
        res = _cells(offsets, cols, direction, tc.derive_grid(cols, 50.0, 2.0), 1.0)[2]
        assert res["status"] == 0 and res["counters"]["used"] > 100
        _conserved(res)


def test_many_scene_reaches_past_a_wave_and_a_workgroup():
    offsets, cols, direction, frame = tc.many_scene()
    n = np.diff(offsets)
    assert len(n) == 67 and n[0] == 66 and n[1] == 301
    d, lane, res = _cells(offsets, cols, direction, tc.derive_grid(cols, 50.0, 2.0), 1.0)
    c = res["counters"]
    assert set(d.tolist()) == {1, -1} and set(lane.tolist()) >= {-1, 0, 1, 2, 3, 4} and c["skipped_gap"] > 0 and c["skipped_lane"] > 0
    assert c["pieces"] > c["used"] > 200 and int(res["n"].max()) > 1


# ------------------------------------------------------------------------------------------------ the shipped tracking output
def test_golden_counts(golden):
    offsets, cols, direction, frame = tc.golden_scene(golden("track_stitch"))
    grid = tc.derive_grid(cols, tc.GOLDEN_PARAMS["dx"], tc.GOLDEN_PARAMS["dt"])
    d, lane, res = _cells(offsets, cols, direction, grid, tc.GOLDEN_PARAMS["max_gap"])
    c = res["counters"]
    assert res["status"] == 0 and {k: c[k] for k in tc.GOLDEN_COUNTS} == tc.GOLDEN_COUNTS
    assert res["max_pieces"] == 3 and c["outside"] == 0 and int((res["n"] > 0).sum()) == 575
    assert abs(int(res["T"].sum()) / tc.Q - 240.48) < 0.01 and abs(int(res["D"].sum()) / tc.Q - 25135) < 1.0
    assert (cols[:, 0] == -1).any()                                                 # the rows the grid's t0 must leave out
    frame_off, frame_rows = tc.frames_csr(frame)
    assert int(np.diff(frame_off).max()) == 17


# ------------------------------------------------------------------------------------------------ the leaders at their edges
def test_leader_scene_holds_every_edge():
    offsets, cols, direction, frame_off, frame_rows = tc.leader_edge_scene()
    assert np.diff(frame_off).tolist() == list(tc.LEADER_FRAMES)
    d, lane, status = tc.lanes(offsets, cols, direction, tc.DEFAULT_EDGES)
    res = tc.leaders(offsets, cols, d, lane, frame_off, frame_rows)
    assert status == res["status"] == 0 and res["ties"] > 0 and res["overlaps"] > 0 and 0 < res["with_leader"] < len(cols)
    trk = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    has = res["leader"] >= 0
    assert (lane[has] >= 0).all() and (lane == -1).any() and (d[trk[res["leader"][has]]] == d[trk[has]]).all()
    assert set(lane[d[trk] == 1].tolist()) == set(lane[d[trk] == -1].tolist()) == {-1, 0, 1, 2, 3, 4}
    assert (res["spacing"][has] > 0).all() and np.isinf(res["headway"][has & (cols[:, 6] <= 0)]).all() and (has & (cols[:, 6] <= 0)).any()
    assert np.isfinite(res["ttc"]).any() and np.isinf(res["ttc"][has]).any()
    # two rows at the same x in one frame, direction and lane: neither leads the other
    big = frame_rows[int(frame_off[4]):]
    same = [(i, j) for i in big for j in big if i < j and cols[i, 1] == cols[j, 1] and lane[i] == lane[j] >= 0 and d[trk[i]] == d[trk[j]]]
    assert same and all(res["leader"][i] != j and res["leader"][j] != i for i, j in same)
    # a tie goes to the smaller tracklet index
    for i in np.nonzero(has)[0]:
        f = int(cols[i, 0]) - 100
        rivals = [j for j in frame_rows[int(frame_off[f]):int(frame_off[f + 1])] if j != i and lane[j] == lane[i] and d[trk[j]] == d[trk[i]]
                  and d[trk[i]] * (cols[j, 1] - cols[i, 1]) == res["spacing"][i]]
        assert res["leader"][i] == min(rivals, key=lambda j: trk[j])


# ------------------------------------------------------------------------------------------------ traffic_state on the host
def test_resolve_params_refusals_and_defaults():
    import traffic_state as ts
    p = ts.resolve_params()
    assert (p["dx"], p["dt"], p["max_gap"], p["x_range"], p["t_range"]) == (100.0, 5.0, 1.0, None, None)
    assert p["lane_edges"][1].tolist() == tc.DEFAULT_EDGES[1] and p["lane_edges"][-1].tolist() == tc.DEFAULT_EDGES[-1]
    assert p["lane_edges"][1].dtype == np.float64 and ts.DEFAULTS["lane_edges"][1] == [0, 12, 24, 36, 48, 60]
    assert ts.resolve_params({"dx": 50, "x_range": (0, 10)})["x_range"] == (0.0, 10.0)
    for bad in ({"dz": 1}, {"dx": 0}, {"dt": -1.0}, {"max_gap": 0}, {"dx": float("inf")}, {"dt": float("nan")},
                {"lane_edges": {1: [0, 12, 12], -1: [60, 72]}}, {"lane_edges": {1: [0, 12], -1: [72, 60]}}, {"lane_edges": {1: [0, 12]}},
                {"lane_edges": [0, 12]}, {"lane_edges": {1: [0, float("nan")], -1: [60, 72]}}, {"x_range": (5, 5)}, {"t_range": (2, 1)}):
        with pytest.raises(ValueError):
            ts.resolve_params(bad)


def test_grid_derivation(golden):
    import traffic_state as ts
    offsets, cols, direction, frame = tc.golden_scene(golden("track_stitch"))
    g = ts.grid_of(cols, ts.resolve_params(tc.GOLDEN_PARAMS))
    assert (g["t0"], g["dt"], g["nt"], g["x0"], g["dx"], g["nx"]) == tc.derive_grid(cols, 50.0, 2.0)
    t = cols[:, 0][cols[:, 0] > 0]
    assert g["t0"] <= t.min() < g["t0"] + 2.0 and g["t0"] + 2.0 * (g["nt"] - 1) <= t.max() < g["t0"] + 2.0 * g["nt"] and g["t0"] % 2.0 == 0
    assert g["x0"] <= cols[:, 1].min() < g["x0"] + 50.0 and g["x0"] + 50.0 * (g["nx"] - 1) <= cols[:, 1].max() < g["x0"] + 50.0 * g["nx"]
    rows = np.array([tc.row(-1, -30.0), tc.row(7.5, 210.0), tc.row(19.9, 99.0)])
    g = ts.grid_of(rows, ts.resolve_params({"dx": 100, "dt": 5}))
    assert (g["t0"], g["nt"], g["x0"], g["nx"]) == (5.0, 3, -100.0, 4)
    g = ts.grid_of(rows, ts.resolve_params({"dx": 64, "dt": 2, "x_range": (0, 384), "t_range": (100, 111)}))
    assert (g["t0"], g["nt"], g["x0"], g["nx"]) == (100.0, 6, 0.0, 6)
    g = ts.grid_of(np.zeros((0, 7)), ts.resolve_params())
    assert (g["nt"], g["nx"]) == (0, 0)
    off, rows = ts.frames_csr([2, 0, 2, 4], 6)
    assert off.tolist() == [0, 1, 1, 3, 3, 4, 4] and rows.tolist() == [1, 0, 2, 3] and rows.dtype == np.int32


def test_the_operators_are_registered_and_refuse_cpu_tensors():
    import torch
    from retinanet_mi355x import ops, torch_ops
    for name in ("traffic_lanes", "traffic_cells", "traffic_leaders"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    assert ops.TRAFFIC_Q == tc.Q == 1 << 20 and ops.TRAFFIC_CELL_COUNTERS == tc.CELL_COUNTERS and ops.TRAFFIC_MAX_CUTS == tc.MAX_CUTS
    assert (ops.TRAFFIC_NONFINITE, ops.TRAFFIC_TOO_MANY_CUTS, ops.TRAFFIC_RANGE, ops.TRAFFIC_BAD_DIR) == (tc.NONFINITE, tc.TOO_MANY_CUTS, tc.RANGE, tc.BAD_DIR)
    offsets, cols, direction, names = tc.cell_edge_scene()
    o, c, dr = torch.from_numpy(offsets), torch.from_numpy(cols), torch.from_numpy(direction)
    ep, en = (torch.tensor(tc.DEFAULT_EDGES[s], dtype=torch.float64) for s in (1, -1))
    d, lane = torch.ones(len(offsets) - 1, dtype=torch.int32), torch.zeros(len(cols), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.traffic_lanes(o, c, dr, ep, en)                                         # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.traffic_cells(o, c, d, ep, en, *tc.EDGE_GRID, tc.EDGE_MAX_GAP)
    with pytest.raises(RuntimeError):
        ops.traffic_leaders(o, c, d, lane, torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"status 9\b"):
        ops.traffic_check(9)
    ops.traffic_check(0)

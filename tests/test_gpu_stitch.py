"""GPU: csrc/stitch.hip (ops.stitch_*), track_stitch.stitch_tracks and Data_Reader.stitch against the restatement of
tests/stitch_cases.py and the stored arrays of tests/golden/track_stitch.npz.

Every stage goes through its own op, fed with the restatement's output of the stage before, so a stage is judged alone.  Bit for
bit (fp64, one rounding per operation on both sides, the same order): end points, the dense W, Wc, link costs, fill fields and times.
Exact: candidate lists and counts, next / prev, root, rank, new_id, fill counts, prefix, link and side.

Shapes: tracklets of 1, 2, 7, 8, 9 and 70 rows around fit_n = 8, 1 and 64; 1, 2, 65 and 130 tracklets per direction (the 64 x 64
cost tile, the wave and the 256-thread scan of the compaction), one direction empty; chains of 2, 9 and 33 (pointer jumping's last
round); links of 0, 1 and 70 new rows, 1 471 in all (more than four workgroups of the row kernel)."""
import os

import numpy as np
import pytest
import torch

import stitch_cases as sc

pytestmark = pytest.mark.gpu


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ns(t):
    from retinanet_mi355x import ops, torch_ops     # noqa: F401  (registers torch.ops.retinanet_mi355x.*)
    return torch.ops.retinanet_mi355x if t else ops


def device_stages(dev, ep, ids, params=None, fill=True, want=None, t=False):
    """Every stage after the end points through its own op -> numpy arrays under the restatement's names.  want: the restatement's
    arrays; each op then takes ITS inputs from there instead of from the op before."""
    o = _ns(t)
    p, P = sc.scales_of(params)
    P = list(P)
    N = len(ep)
    d_ep = _up(dev, ep)
    got = {"W": o.stitch_costs(d_ep, P)}
    cand, ncand = o.stitch_candidates(d_ep, P)
    got.update(cand=cand, ncand=ncand)
    if want is not None:
        cand, ncand = _up(dev, want["cand"]), _up(dev, want["ncand"])
    plus = int((ep[:, 0, sc.SGN] > 0).sum())
    cap = plus * plus + (N - plus) * (N - plus)
    Wc, st_c = o.stitch_compact(d_ep, P, cand, ncand, cap)
    n = ncand.cpu().tolist()
    used = n[0] * n[1] + n[2] * n[3]                                               # the cells behind stay unwritten
    got["Wc"] = Wc[:used]
    if want is not None:
        Wc = torch.cat((_up(dev, want["Wc"]), Wc[used:]))
    nxt, prev, link_cost, st_a = o.stitch_assign(d_ep, P, cand, ncand, Wc)
    got.update(next=nxt, prev=prev, link_cost=link_cost)
    if want is not None:
        nxt, prev = _up(dev, want["next"]), _up(dev, want["prev"])
    root, rank, new_id, st_r = o.stitch_chains(prev, _up(dev, np.asarray(ids, np.int64)))
    got.update(root=root, rank=rank, new_id=new_id)
    status = [st_c, st_a, st_r]
    if fill:
        count, prefix, st_f = o.stitch_fill_count(d_ep, nxt, p["fill_rate"])
        got.update(count=count, prefix=prefix)
        rows = (int(want["prefix"][-1]) if want is not None else int(prefix[-1])) + 3            # three rows that stay unwritten
        fields, time, link, side, st_w = o.stitch_fill_rows(d_ep, nxt, prefix, p["fill_rate"], rows)
        got.update(fields=fields[:rows - 3], time=time[:rows - 3], link=link[:rows - 3], side=side[:rows - 3])
        status += [st_f, st_w]
    assert all(int(s) == 0 for s in status), [int(s) for s in status]
    return {k: v.cpu().numpy() for k, v in got.items()}


BITS = ("W", "Wc", "link_cost", "fields", "time")


def check(got, want):
    for key, g in got.items():
        w = want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
        if key in BITS:
            assert g.tobytes() == w.tobytes(), (key, np.abs(g - w).max())
        else:
            assert np.array_equal(g, w), key


# ------------------------------------------------------------------------------------------------ end points
@pytest.fixture(scope="module")
def end_scene():
    return sc.endpoint_scene()


@pytest.mark.parametrize("fit_n", [8, 1, 64])
def test_end_points_bit_for_bit(dev, end_scene, fit_n):
    from retinanet_mi355x import ops, torch_ops     # noqa: F401  (registers torch.ops.retinanet_mi355x.*)
    ids, offsets, cols, direction = end_scene
    want = sc.endpoints(offsets, cols, direction, fit_n)
    ep, status = ops.stitch_endpoints(_up(dev, offsets), _up(dev, cols), _up(dev, direction), fit_n)
    got = ep.cpu().numpy()
    assert int(status) == 0 and got.shape == want.shape and got.tobytes() == want.tobytes(), np.abs(got - want).max()
    n = np.diff(offsets)
    assert sorted(set(n.tolist())) == [1, 2, 3, 4, 7, 8, 9, 70] and np.array_equal(got[:, 0, sc.K], np.minimum(n, fit_n))
    two = list(ids).index(500)                                                      # equal times: the slope is sgn * v of the end row
    assert got[two, 0, sc.VX] == -88.0 and got[two, 1, sc.VX] == -77.0 and got[list(ids).index(501), 0, sc.SGN] == 1.0
    assert got[list(ids).index(502), 0, sc.SGN] == -1.0
    t_ep, _ = torch.ops.retinanet_mi355x.stitch_endpoints(_up(dev, offsets), _up(dev, cols), _up(dev, direction), fit_n)
    assert t_ep.cpu().numpy().tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ costs .. fill, stage by stage
def _lane(n, seed, both=True):
    ids, offsets, cols, direction = sc.lane_scene(n, seed, both)
    return sc.endpoints(offsets, cols, direction, 8), ids


def _both_funnels():
    ep = np.concatenate((sc.funnel_ep(5, 2, 1), sc.funnel_ep(2, 5, 2, sgn=-1.0)))   # nr' > nc' one way, nr' < nc' the other
    return ep, np.arange(len(ep)) * 2 + 7


SCENES = {
    "lane1": lambda: _lane(1, 1), "lane2": lambda: _lane(2, 2), "lane65": lambda: _lane(65, 3), "lane130": lambda: _lane(130, 4),
    "one_direction": lambda: _lane(67, 5, both=False),
    "edges": lambda: (sc.edge_ep()[0], np.arange(20) + 1),
    "greedy_trap": lambda: (sc.greedy_trap_ep()[0], np.array([40, 30, 20, 10])),
    "tall_and_wide": _both_funnels,
    "tall70": lambda: (sc.funnel_ep(70, 66, 6), np.arange(136)),
    "wide70": lambda: (sc.funnel_ep(66, 70, 7), np.arange(136)[::-1].copy()),
    "no_candidates": lambda: (sc.no_candidate_ep(), np.arange(5)),
}


@pytest.fixture(scope="module")
def scene():
    cache = {}

    def get(name):
        if name not in cache:
            ep, ids = SCENES[name]()
            cache[name] = (ep, ids, sc.run_from_ep(ep, ids))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(SCENES))
def test_stages_against_the_restatement(dev, scene, name):
    ep, ids, want = scene(name)
    check(device_stages(dev, ep, ids, want=want), want)                             # each stage alone ...
    check(device_stages(dev, ep, ids), want)                                        # ... and chained
    links = {(a, int(want["next"][a])) for a in range(len(ep)) if want["next"][a] >= 0}
    if name == "edges":
        assert links == {k for k, ok in sc.edge_ep()[1].items() if ok}
    if name == "greedy_trap":
        assert links == sc.greedy_trap_ep()[1]
    if name == "tall_and_wide":
        assert want["ncand"].tolist() == [5, 2, 2, 5] and len(links) == 4
    if name == "no_candidates":
        assert want["ncand"].tolist() == [0] * 4 and not links and np.array_equal(want["root"], np.arange(5))
    if name == "one_direction":
        assert want["ncand"][2:].tolist() == [0, 0] and want["ncand"][0] > 0
    if name.startswith("lane") and name != "lane1":
        assert len(links) > 0 or name == "lane2"


def test_two_runs_and_the_torch_operators(dev, scene):
    for name in ("lane65", "tall_and_wide"):
        ep, ids, want = scene(name)
        a, b, c = device_stages(dev, ep, ids), device_stages(dev, ep, ids), device_stages(dev, ep, ids, t=True)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key
            assert a[key].tobytes() == c[key].tobytes() and a[key].dtype == c[key].dtype and a[key].shape == c[key].shape, key


@pytest.mark.parametrize("lengths,singles", [((2, 9, 33), 3), ((65, 17, 5, 3), 0), ((1,), 0), ((129,), 1)])
def test_chains_by_pointer_jumping(dev, lengths, singles):
    from retinanet_mi355x import ops
    prev, ids, root, rank = sc.chain_prev(lengths, singles)
    got = ops.stitch_chains(_up(dev, prev), _up(dev, ids))
    assert int(got[3]) == 0
    assert np.array_equal(got[0].cpu().numpy(), root) and np.array_equal(got[1].cpu().numpy(), rank)
    assert np.array_equal(got[2].cpu().numpy(), ids[root]) and rank.max() == max(lengths) - 1


def test_fill_counts_rows_and_the_half_way_row(dev):
    from retinanet_mi355x import ops
    for (ep, nxt), rate in ((sc.fill_ep(), 30.0), (sc.quarter_ep(), 4.0)):
        count, prefix = sc.fill_count(ep, nxt, rate)
        want = sc.fill_rows(ep, nxt, prefix, rate)
        g_count, g_prefix, st = ops.stitch_fill_count(_up(dev, ep), _up(dev, nxt), rate)
        assert np.array_equal(g_count.cpu().numpy(), count) and np.array_equal(g_prefix.cpu().numpy(), prefix)
        U = int(prefix[-1])
        got = ops.stitch_fill_rows(_up(dev, ep), _up(dev, nxt), g_prefix, rate, U, status=st)
        assert int(got[4]) == 0
        for g, w, bits in zip(got[:4], want, (True, True, False, False)):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and (g.tobytes() == w.tobytes() if bits else np.array_equal(g, w))
    assert count.tolist() == [1, 0] and want[1].tolist() == [1.25] and want[3].tolist() == [0]       # t_2 = t_s excluded; u = 0.5
    ep, nxt = sc.fill_ep()
    assert sorted(set(sc.fill_count(ep, nxt, 30.0)[0][nxt >= 0].tolist())) == [0, 1, 70]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev, end_scene):
    import track_stitch
    from retinanet_mi355x import ops
    ids, offsets, cols, direction = end_scene
    up = lambda a: _up(dev, a)     # noqa: E731
    bad = cols.copy()
    bad[40, 3] = np.nan
    _, status = ops.stitch_endpoints(up(offsets), up(bad), up(direction), 8)
    assert int(status) == ops.STITCH_NONFINITE
    bad[40, 3] = -np.inf
    assert int(ops.stitch_endpoints(up(offsets), up(bad), up(direction), 8)[1]) == ops.STITCH_NONFINITE
    with pytest.raises(RuntimeError, match="NaN"):
        ops.stitch_check(status)
    wrong = offsets.copy()
    wrong[3] = wrong[2]                                                             # an empty tracklet
    assert int(ops.stitch_endpoints(up(wrong), up(cols), up(direction), 8)[1]) == ops.STITCH_BAD_OFFSETS
    wrong[3] = len(cols) + 5                                                        # rows outside the packed ones
    ep, status = ops.stitch_endpoints(up(wrong), up(cols), up(direction), 8)
    assert int(status) == ops.STITCH_BAD_OFFSETS and not ep[2].cpu().numpy().any()
    for fit_n in (0, 65):
        with pytest.raises(ValueError):
            ops.stitch_endpoints(up(offsets), up(cols), up(direction), fit_n)
    ep = up(sc.no_candidate_ep())
    with pytest.raises(ValueError):
        ops.stitch_costs(ep, [3.0, 5.0, 10.0, 10.0, 0.0, 10.0, 3.0])
    with pytest.raises(ValueError):
        ops.stitch_fill_count(ep, torch.full((5,), -1, dtype=torch.int32, device=dev), 0.0)
    big = torch.zeros((ops.STITCH_MAX_TRACKLETS + 1, 2, ops.STITCH_EP), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="at most"):
        ops.stitch_candidates(big, list(sc.P0))
    with pytest.raises(RuntimeError, match="at most"):
        ops.stitch_costs(big[:ops.STITCH_DENSE_MAX + 1], list(sc.P0))
    with pytest.raises(RuntimeError):
        ops.stitch_costs(ep.float(), list(sc.P0))
    links = torch.tensor([1, 7, -1, 3, -1], dtype=torch.int32, device=dev)         # 7: outside; 3 -> 3: itself
    assert int(ops.stitch_chains(links, up(np.arange(5)))[3]) == ops.STITCH_BAD_LINK
    count, _, status = ops.stitch_fill_count(ep, links, 30.0)
    assert int(status) == ops.STITCH_BAD_LINK and count.cpu().numpy()[1] == 0 and count.cpu().numpy()[3] == 0
    # the public call: a NaN raises and nothing is replaced; too many tracklets raise before any launch
    data, _, _ = sc.highway(0)
    data[5][next(iter(data[5]))]["y"] = float("nan")
    before = [dict(f) for f in data]
    with pytest.raises(RuntimeError, match="NaN"):
        track_stitch.stitch_tracks(data, device=dev)
    assert all(a.keys() == b.keys() and all(a[k] is b[k] for k in a) for a, b in zip(data, before))
    with pytest.raises(RuntimeError, match="at most"):
        track_stitch.bounds(np.arange(ops.STITCH_MAX_TRACKLETS + 2), np.ones(ops.STITCH_MAX_TRACKLETS + 1, np.int32), sc.DEFAULTS)
    with pytest.raises(ValueError):
        track_stitch.stitch_tracks(data, {"sigma_y": -1.0}, device=dev)


def test_more_candidates_than_the_solver_takes_is_refused(dev):
    """4 097 tails that all see 4 097 heads: min(nr', nc') is above RN_LSAP_MAX_MIN.  The count exists on the device only, so the
    refusal is a status bit; no solve is started and no link is written."""
    from retinanet_mi355x import ops
    n = ops.LSAP_MAX_MIN + 1
    ep = np.zeros((2 * n, 2, sc.EP))
    ep[:, :, :14] = sc.make_ep(8.0, 10.0, 50.0, 20.0)[:, :14]
    ep[n:, 0, sc.T], ep[n:, 1, sc.T] = 11.0, 12.0
    d_ep, P = _up(dev, ep), list(sc.P0)
    cand, ncand = ops.stitch_candidates(d_ep, P)
    assert ncand.cpu().tolist() == [n, n, 0, 0]
    Wc, status = ops.stitch_compact(d_ep, P, cand, ncand, n * n)
    assert int(status) == 0 and float(Wc.max()) == -3.0 and float(Wc.min()) == -3.0
    nxt, prev, _, status = ops.stitch_assign(d_ep, P, cand, ncand, Wc)
    assert int(status) == ops.STITCH_TOO_MANY and int((nxt >= 0).sum()) == 0 and int((prev >= 0).sum()) == 0
    with pytest.raises(RuntimeError, match="%d" % ops.LSAP_MAX_MIN):
        ops.stitch_check(status)


# ------------------------------------------------------------------------------------------------ end to end
def _hg(dev):
    import homography
    import mot_cases as mc
    hg = homography.Homography(device=str(dev))
    hg.correspondence = {"cam": {"H": np.asarray(mc.SYN_H, np.float64), "P": np.asarray(mc.SYN_P, np.float64)}}
    hg.default_correspondence = "cam"
    return hg


def test_highway_is_recovered_and_scores_like_the_truth(dev):
    """The closed form of stitch_cases.highway: ``root`` reproduces the vehicle partition exactly; without the fill the stitched
    rows score exactly as the same rows under the vehicles' ids do, and IDF1 was lower before."""
    import mot_assoc_cases as ac
    import mot_evaluator as me
    import track_stitch
    data, owner, stamps = sc.highway(0)
    new_data, report = track_stitch.stitch_tracks(data, fill=False, device=dev)
    vehicle = np.array([owner[int(i)] for i in report["ids"]])
    assert np.array_equal(vehicle[report["root"]], vehicle) and len(set(report["root"].tolist())) == sc.LANES
    assert len(report["links"]) == len(vehicle) - sc.LANES and report["fill"] is None and report["status"] == 0
    assert max(l[2] for l in report["links"]) < 1e-9
    for a, b, cost in report["links"]:
        assert report["next"][a] == b and report["rank"][b] == report["rank"][a] + 1
    assert [sorted(int(report["new_id"][list(report["ids"]).index(k)]) for k in f) for f in data] == [sorted(f) for f in new_data]
    assert all(k == v["id"] for f in new_data for k, v in f.items())
    hg, scores = _hg(dev), {}
    for name, rows, label in (("before", data, lambda k: k), ("stitched", new_data, lambda k: k), ("truth", data, lambda k: owner[k] + 1)):
        gt, pred, flat = ac.scene_rows(sc.assoc_scene(stamps, rows, label))
        scores[name] = me.evaluate_association(gt, pred, hg, ious=torch.from_numpy(flat).to(dev))
    for key in me.ASSOC_SCALARS:
        assert scores["stitched"][key] == scores["truth"][key], key
    for key in ac.FIGURES:
        assert scores["stitched"]["per_alpha"][key].tobytes() == scores["truth"]["per_alpha"][key].tobytes(), key
    print("IDF1 before %.4f, stitched %.4f" % (scores["before"]["IDF1"], scores["stitched"]["IDF1"]))
    assert scores["before"]["IDF1"] < scores["stitched"]["IDF1"]
    # with the fill every vehicle is present from its first to its last row
    filled, rep = track_stitch.stitch_tracks(data, device=dev)
    want = sc.run_all(*[track_stitch.pack_tracklets(data)[k] for k in ("ids", "offsets", "cols", "direction")])
    assert np.array_equal(rep["next"], want["next"]) and rep["fill"]["fields"].tobytes() == want["fields"].tobytes()
    assert rep["fill"]["time"].tobytes() == want["time"].tobytes() and np.array_equal(rep["fill"]["side"], want["side"])
    ts = [[v["timestamp"] for v in f.values()] for f in filled]
    assert all(len(set(t)) == 1 for t in ts) and [t[0] for t in ts] == sorted(t[0] for t in ts) and len(set(t[0] for t in ts)) == len(ts)
    assert sum(len(f) for f in filled) == sum(len(f) for f in data) + len(want["time"]) - rep["fill"]["skipped"]


def test_golden_file(dev, golden):
    """The shipped tracking output of the reference: the device's links, chains and fill rows equal the stored ones."""
    import track_stitch
    g = golden("track_stitch")
    host = track_stitch.stitch_packed(g["ids"], g["offsets"], g["cols"], g["direction"], track_stitch.resolve_params(), True, dev)
    for key in ("ep", "link_cost", "fields", "time"):
        assert host[key].dtype == g[key].dtype and host[key].tobytes() == g[key].tobytes(), key
    for key in ("ncand", "next", "prev", "root", "rank", "new_id", "count", "prefix", "link", "side"):
        assert host[key].dtype == g[key].dtype and np.array_equal(host[key], g[key]), key
    assert int((host["next"] >= 0).sum()) == 28


# ------------------------------------------------------------------------------------------------ Data_Reader.stitch
def _broken_csv():
    """Two vehicles, one each way, and a third in a far lane, at 30 Hz over 60 frames; the first loses its id for 10 frames and the
    second for 25, at different times."""
    import datareader_cases as dc
    header = dc.HEADER + ["ts_bias for cameras ['p1c1']"]
    rows = []
    plan = [(1, 20.0, 1, 100.0, [(0, 20, 11), (30, 60, 12)]), (-1, 80.0, -1, 900.0, [(5, 15, 21), (40, 60, 22)]),
            (1, 44.0, 1, 300.0, [(0, 60, 31)])]
    for f in range(60):
        t = 1623877000.0 + f / 30.0
        for direction, y, sgn, x0, spans in plan:
            for lo, hi, tid in spans:
                if lo <= f < hi:
                    cells = [""] * 45
                    cells[0], cells[1], cells[2], cells[3], cells[10] = str(f), "%.6f" % t, str(tid), "sedan", "3D Detector"
                    cells[35], cells[36], cells[37], cells[38] = str(float(direction)), "p1c1", "0", repr(95.0)
                    cells[39], cells[40], cells[41] = repr(x0 + sgn * 95.0 * (f / 30.0)), repr(y), "0"
                    cells[42], cells[43], cells[44] = repr(6.0), repr(16.0), repr(5.0)
                    rows.append(cells + ["[0.0]"])
    return dc.csv_text([header] + rows)


def test_data_reader_stitch(dev, tmp_path):
    import datareader
    import datareader_cases as dc
    import homography
    hg = homography.Homography()
    hg.correspondence = {"p1c1": {"P": dc.cameras()[1][2]}}
    hg.default_correspondence = "p1c1"
    path = os.path.join(str(tmp_path), "in.csv")
    with open(path, "w", newline="") as f:
        f.write(_broken_csv())
    dr = datareader.Data_Reader(path, hg)
    n_rows = sum(len(f) for f in dr.data)
    next(dr)
    out = os.path.join(str(tmp_path), "stitched.csv")
    report = dr.stitch(save=out)
    assert dr.d_idx == 0 and report["ids"].tolist() == [11, 12, 21, 22, 31]
    assert sorted((int(report["ids"][a]), int(report["ids"][b])) for a, b, _ in report["links"]) == [(11, 12), (21, 22)]
    assert {k for f in dr.data for k in f} == {11, 21, 31} and all(k == v["id"] for f in dr.data for k, v in f.items())
    ts = [[v["timestamp"] for v in f.values()] for f in dr.data]
    assert all(len(set(t)) == 1 for t in ts) and [t[0] for t in ts] == sorted(t[0] for t in ts)
    new = len(report["fill"]["time"]) - report["fill"]["skipped"]            # skipped: a row whose rounded stamp is the next real row's
    assert new >= 9 + 23 and sum(len(f) for f in dr.data) == n_rows + new
    for vid, n in ((11, 60), (21, 55)):                                            # present from the first to the last row
        assert sum(vid in f for f in dr.data) >= n - 1
    filled = [v for f in dr.data for v in f.values() if v["id"] == 21 and 1623877000.5 < v["timestamp"] < 1623877001.3]
    # The file's x lies on the line in exact time, its stamps are rounded to 1e-4 s: a row is up to 95 * 5e-5 = 0.005 ft off the line
    # in stamp time, a slope over 7 / 30 s up to about 0.06 ft/s, the secant over the gap up to 0.011 ft/s.  The Hermite weights of
    # the two slopes sum to at most 0.3 g in x and to at most 1 in v: x within 0.005 + 0.005 + 0.3 * 0.87 * 0.06 < 0.05, v within 0.25.
    # y = (1 - u) 80 + u 80: three roundings of about 80 * 2^-53 each.
    assert len(filled) >= 23 and all(v["direction"] == -1 and abs(v["v"] - 95.0) < 0.25 and abs(v["y"] - 80.0) < 1e-12 for v in filled)
    assert all(abs(v["x"] - (900.0 - 95.0 * (v["timestamp"] - 1623877000.0))) < 0.05 for v in filled)
    with open(out, newline="") as f:
        assert len(dc.parse(f.read())) == 1 + sum(len(f) for f in dr.data)         # write_to_file succeeded: header + rows
    again = dr.stitch(fill=False)
    print("a second stitch links", again["links"])
    assert again["links"] == [] and again["ids"].tolist() == [11, 21, 31]

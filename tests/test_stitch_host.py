"""CPU: the restatement of track stitching (tests/stitch_cases.py) against the stored arrays of tests/golden/track_stitch.npz,
against scipy and against the hand-derived scenes; the host half of track_stitch.py (parameters, packing, rebuilding ``data``).
No device code runs here."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import stitch_cases as sc


@pytest.fixture(scope="module")
def gold(golden):
    g = golden("track_stitch")
    return g, sc.run_all(g["ids"], g["offsets"], g["cols"], g["direction"])


def test_restatement_reproduces_the_golden_arrays(gold):
    g, got = gold
    for key in ("ep", "cand", "ncand", "Wc", "next", "prev", "link_cost", "root", "rank", "new_id", "count", "prefix", "fields", "time",
                "link", "side"):
        assert got[key].dtype == g[key].dtype and got[key].shape == g[key].shape, key
        assert got[key].tobytes() == g[key].tobytes(), key
    assert (got["next"] >= 0).sum() == 28 and len(set(got["root"][got["next"] >= 0].tolist())) == 18


def test_golden_links_are_scipy_s_and_respect_the_gates(gold):
    g, got = gold
    ep, P = got["ep"], sc.P0
    nc, at, links = g["ncand"], 0, []
    for d in (0, 1):
        nr_, nc_ = int(nc[2 * d]), int(nc[2 * d + 1])
        Wc = g["Wc"][at:at + nr_ * nc_].reshape(nr_, nc_)
        at += nr_ * nc_
        assert np.array_equal(Wc, got["W"][np.ix_(g["cand"][d, 0, :nr_], g["cand"][d, 1, :nc_])])
        assert (Wc < 0).any(axis=1).all() and (Wc < 0).any(axis=0).all()          # every listed tail and head has a candidate
        rows, cols = linear_sum_assignment(Wc)
        links += [(int(g["cand"][d, 0, r]), int(g["cand"][d, 1, c])) for r, c in zip(rows, cols) if Wc[r, c] < 0]
    assert at == len(g["Wc"])
    assert sorted(links) == sorted((int(a), int(g["next"][a])) for a in np.nonzero(g["next"] >= 0)[0])
    tails, heads = [l[0] for l in links], [l[1] for l in links]
    assert len(set(tails)) == len(tails) and len(set(heads)) == len(heads)          # no tail or head is used twice
    for a, b in links:
        gap = ep[b, 0, sc.T] - ep[a, 1, sc.T]
        assert a != b and 0 < gap <= P[0] and ep[a, 1, sc.SGN] == ep[b, 0, sc.SGN]
        assert ep[a, 1, sc.SGN] * (ep[b, 0, sc.XH] - ep[a, 1, sc.XH]) >= -P[1]
        ok, cost = sc.pair(ep[a, 1], ep[b, 0], P)
        assert ok and cost < P[6] and cost == g["link_cost"][a] and g["prev"][b] == a
    for i in range(len(ep)):                                                        # chains follow the links, end times rise
        if g["prev"][i] >= 0:
            p = g["prev"][i]
            assert g["root"][i] == g["root"][p] and g["rank"][i] == g["rank"][p] + 1 and ep[i, 1, sc.T] > ep[p, 1, sc.T]
        else:
            assert g["root"][i] == i and g["rank"][i] == 0
    assert np.array_equal(g["new_id"], g["ids"][g["root"]])


def test_hand_derived_scenes():
    ep, want = sc.edge_ep()
    Wm = sc.costs(ep, sc.P0)
    for (a, b), ok in want.items():
        assert (Wm[a, b] < 0) == ok, (a, b)
    assert (Wm < 0).sum() == sum(want.values())                                     # and no pair across the lanes
    assert Wm[10, 11] == 5.0 / 20.0 - 3.0                                           # on back_tol: cost (5 + 5) / 2 / (10 + 10 * 1)
    ok, cost = sc.pair(ep[6, 1], ep[7, 0], sc.P0)
    assert not ok and cost == 3.0                                                   # cost == max_cost exactly: not linkable
    ep, links = sc.greedy_trap_ep()
    got = sc.run_from_ep(ep, np.arange(4), fill=False)
    assert {(a, int(got["next"][a])) for a in range(4) if got["next"][a] >= 0} == links
    assert np.allclose(got["W"][0, 2] + 3.0, 0.1) and got["W"][0, 2] == got["W"].min()  # the pair greedy would take first
    assert sc.run_from_ep(sc.no_candidate_ep(), np.arange(5))["ncand"].tolist() == [0, 0, 0, 0]
    for n_t, n_h in ((5, 2), (2, 5)):
        got = sc.run_from_ep(sc.funnel_ep(n_t, n_h, 3), np.arange(n_t + n_h), fill=False)
        assert got["ncand"].tolist() == [n_t, n_h, 0, 0] and (got["next"] >= 0).sum() == min(n_t, n_h)
    prev, ids, root, rank = sc.chain_prev()
    r, k, new_id = sc.chains(prev, ids)
    assert np.array_equal(r, root) and np.array_equal(k, rank) and np.array_equal(new_id, ids[root])


def test_fill_counts_and_the_half_way_row():
    ep, nxt = sc.quarter_ep()
    count, prefix = sc.fill_count(ep, nxt, 4.0)
    assert count.tolist() == [1, 0]                                                 # t_2 = t_s is excluded
    fields, time, link, side = sc.fill_rows(ep, nxt, prefix, 4.0)
    assert time.tolist() == [1.25] and side.tolist() == [0] and link.tolist() == [0]
    assert fields[0, 0] == 0.5 * 18.0 + 0.125 * 0.5 * 8.0 + 0.5 * 22.0 - 0.125 * 0.5 * 8.0    # Hermite at u = 0.5
    assert fields[0, 5] == abs((-1.5 * 18.0 - 0.25 * 0.5 * 8.0 + 1.5 * 22.0 - 0.25 * 0.5 * 8.0) / 0.5)
    ep, nxt = sc.fill_ep()
    count, prefix = sc.fill_count(ep, nxt, 30.0)
    assert count[nxt >= 0].tolist() == [0, 1] + [70] * 21 and prefix[-1] == 1471 > 1024


@pytest.mark.parametrize("seed", [0, 1])
def test_highway_is_recovered_exactly(seed):
    import track_stitch
    data, owner, _ = sc.highway(seed)
    pk = track_stitch.pack_tracklets(data)
    got = sc.run_all(pk["ids"], pk["offsets"], pk["cols"], pk["direction"], fill=False)
    vehicle = np.array([owner[int(i)] for i in pk["ids"]])
    assert len(pk["ids"]) > 3 * sc.LANES
    assert np.array_equal(vehicle[got["root"]], vehicle)                            # a chain holds one vehicle only ...
    assert len(set(got["root"].tolist())) == sc.LANES                               # ... and a vehicle is one chain
    worst = got["link_cost"][got["next"] >= 0].max()
    print("worst true link cost", worst)
    assert worst < 1e-9


def test_params_are_validated():
    import track_stitch
    assert track_stitch.DEFAULTS == sc.DEFAULTS and track_stitch.resolve_params() == sc.DEFAULTS
    assert track_stitch.resolve_params({"max_gap": 2, "back_tol": 0})["max_gap"] == 2.0
    for bad in ({"gap": 1.0}, {"sigma_y": 0.0}, {"max_cost": -1.0}, {"max_gap": float("nan")}, {"fit_n": 0}, {"fit_n": 65},
                {"fit_n": 2.5}, {"fill_rate": 0.0}, {"sigma_x0": float("inf")}, {"back_tol": -1.0}):
        with pytest.raises(ValueError):
            track_stitch.resolve_params(bad)


def test_packing_and_rebuilding_on_the_host():
    """pack_tracklets orders tracklets by id and rows by frame; rebuild rewrites keys and ids, puts a filled row into the frame of
    its rounded time stamp or a new one, keeps ``data`` sorted and leaves the input alone."""
    import track_stitch

    def datum(ts, i, x):
        return {"timestamp": np.round(ts, 4), "id": i, "class": "van", "x": x, "y": 1.0, "l": 2.0, "w": 3.0, "h": 4.0, "direction": 1,
                "v": 5.0, "ts_bias": {"p1c1": 0.0}, "camera": "p1c1", "frame": "0"}
    data = [{9: datum(0.0, 9, 0.0), 4: datum(0.0, 4, 50.0)}, {9: datum(0.1, 9, 1.0)}, {4: datum(0.15, 4, 51.0)}, {2: datum(0.4, 2, 4.0)}]
    pk = track_stitch.pack_tracklets(data)
    assert pk["ids"].tolist() == [2, 4, 9] and pk["offsets"].tolist() == [0, 1, 3, 5] and pk["frame"].tolist() == [3, 0, 2, 0, 1]
    assert pk["cols"][:, 1].tolist() == [4.0, 50.0, 51.0, 0.0, 1.0] and pk["direction"].dtype == np.int32
    ep = np.zeros((3, 2, 16))
    ep[:, :, 12] = 1.0
    host = dict(new_id=np.array([9, 4, 9]), next=np.array([-1, -1, 0], np.int32), ep=ep, link=np.array([2, 2, 2], np.int32),
                time=np.array([0.15, 0.25, 0.4]), side=np.array([0, 0, 1], np.uint8), fields=np.arange(18.0).reshape(3, 6))
    new, skipped = track_stitch.rebuild(data, pk, host, True)
    stamps = [[float(v["timestamp"]) for v in f.values()] for f in new]
    assert [s[0] for s in stamps] == [0.0, 0.1, 0.15, 0.25, 0.4] and all(len(set(s)) == 1 for s in stamps)
    assert [sorted(f) for f in new] == [[4, 9], [9], [4, 9], [9], [9]] and skipped == 1       # 0.4 already holds id 9: left out
    assert all(k == v["id"] for f in new for k, v in f.items())
    assert new[2][9]["x"] == 0.0 and new[3][9]["x"] == 6.0 and new[3][9]["v"] == 11.0 and new[3][9]["class"] == "van"
    assert sorted(data[3]) == [2] and data[3][2]["id"] == 2                                   # the input is untouched
    assert track_stitch.bounds(pk["offsets"], pk["direction"], sc.DEFAULTS) == (9, 2 * 92)


def test_the_operators_are_registered():
    import torch
    from retinanet_mi355x import ops, torch_ops
    for name in ("stitch_endpoints", "stitch_costs", "stitch_candidates", "stitch_compact", "stitch_assign", "stitch_chains",
                 "stitch_fill_count", "stitch_fill_rows"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    with pytest.raises(RuntimeError):
        ops.stitch_costs(torch.zeros(3, 2, 16, dtype=torch.float64), sc.P0)                   # a CPU tensor: no fallback

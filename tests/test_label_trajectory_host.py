"""CPU: the host half of the spline trajectories (label_trajectory.py) and their oracle (tests/label_trajectory_cases.py).

The restatement against scipy's UnivariateSpline and the REFERENCE's own annotator (tests/golden/label_trajectory.npz, written by
tools/make_golden_label_trajectory.py).  The golden tool measured the restatement's largest relative deviation from scipy over
the direct cases and a stride of the scene's candidates as 0.0 for coefficients and residuals, so everything FITPACK computes
is pinned here with bit equality: n, ier, the knot vector, the coefficients and the residual of every direct case and of EVERY
candidate of every (object, axis); accepted / rejected for all of them.  The sorted rows are bit-equal to
the reference's locals; the box weights within 8x the deviation the golden tool measured (3.1e-16: the reference projects the
corners with torch.bmm, whose sums differ from the kernel's order in the last bit for a few boxes).  
Scores are summed in ascending row order where numpy sums pairwise: they agree within 8x the largest deviation the golden tool
measured over every accepted candidate (``score_measured``, 6.8e-16), the golden tool keeps every winner 1e-9
clear of the other scores, and the winner index is compared exactly.  gen_trajectories and adjust_ts_with_trajectories run on
the reference's own splines: values and best times bit-equal (which pins every chosen trial).  The kernels themselves:
tests/test_gpu_label_trajectory.py."""
import os
import re

import numpy as np
import pytest
import torch

import label_audit_cases as lc
import label_trajectory_cases as tc

SCENES = tc.golden_scenes()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITTED = (0, 1, 3, 4, 5, 6, 7)                                  # the objects of "traj" that reach the fits


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def golden_splines(g, name, n_ids):
    out = []
    for i in range(n_ids):
        if g["%s_s%d_none" % (name, i)][0]:
            out.append([None, None])
            continue
        pair = []
        for a, k in (("x", 3), ("y", 2)):
            t, c = g["%s_s%d_%s_t" % (name, i, a)], g["%s_s%d_%s_c" % (name, i, a)]
            pair.append(dict(t=t, c=c, n=len(t), k=k))
        out.append(pair)
    return out


def test_direct_fits_equal_scipy_bit_for_bit(golden):
    g = golden("label_trajectory")
    seen = set()
    for i, seed in enumerate(tc.DIRECT_SEEDS):
        x, y, w, k, s = tc.direct_case(seed)
        f = tc.fit(x, y, w, k, s, len(x) + k + 1)
        n = int(g["direct_n"][i])
        assert (f["n"], f["ier"]) == (n, int(g["direct_ier"][i])), seed
        assert np.array_equal(f["t"], g["direct_t"][i, :n]) and np.array_equal(f["c"], g["direct_c"][i, :n - k - 1]), seed
        assert f["fp"] == g["direct_fp"][i], seed
        seen.add((f["ier"], n == len(x) + k + 1, n > max(len(x) // 2, 2 * k + 2)))
    assert {e[0] for e in seen} == {-2, 0, 3}                   # the classes these cases reach
    assert any(e[1] for e in seen) and any(e[2] and not e[1] for e in seen)     # interpolation knots; past the first nest


@pytest.mark.parametrize("idx", FITTED)
def test_candidates_equal_scipy_bit_for_bit(golden, idx):
    g = golden("label_trajectory")
    rows = g["traj_o%d_rows" % idx]
    t, m = rows[:, 0], len(rows)
    dur = np.floor(g["traj_o%d_duration" % idx][0])
    for axis, a, k, tpes, limit in ((0, "x", 3, tc.tpe_x(), dur * 4 + 2), (1, "y", 2, tc.tpe_y(), dur + 2)):
        G = {key: g["traj_o%d_%s_%s" % (idx, a, key)] for key in ("n", "ier", "fp", "t", "c")}
        for j in range(len(tpes)):                              # every candidate
            f = tc.fit(t, rows[:, 1 + axis], rows[:, 3 + axis], k, tc.smoothing(tpes[j], m), tc.ncap_of(limit, k, m))
            n = int(G["n"][j])
            if n - 2 * k > limit:                               # the reference skips it: the lane stopped on the way
                assert f["ier"] == tc.REJECTED and f["n"] <= n, (a, j)
                continue
            assert (f["n"], f["ier"], f["fp"]) == (n, int(G["ier"][j]), G["fp"][j]), (a, j)
            assert np.array_equal(f["t"], G["t"][j, :n]) and np.array_equal(f["c"], G["c"][j, :n - k - 1]), (a, j)


@pytest.mark.parametrize("idx", FITTED)
def test_scores_and_winners_equal_the_reference(golden, idx):
    g = golden("label_trajectory")
    rows, xw2 = g["traj_o%d_rows" % idx], g["traj_o%d_xw2" % idx]
    assert bit_equal(tc.end_weighted(rows[:, 3]), xw2)
    dur = np.floor(g["traj_o%d_duration" % idx][0])
    for axis, a, k, w2, limit in ((0, "x", 3, xw2, dur * 4 + 2), (1, "y", 2, rows[:, 4], dur + 2)):
        G = {key: g["traj_o%d_%s_%s" % (idx, a, key)] for key in ("n", "t", "c", "score_ape", "score_mpe")}
        cache = {}
        for metric in ("ape", "mpe"):
            scores = []
            for j in range(len(G["n"])):
                n = int(G["n"][j])
                if n - 2 * k > limit:
                    scores.append(float("nan"))
                    continue
                key = (metric, G["t"][j, :n].tobytes(), G["c"][j, :n].tobytes())
                if key not in cache:
                    cache[key] = tc.score(G["t"][j], G["c"][j], n, k, rows[:, 0], rows[:, 1 + axis], w2, metric, axis)
                scores.append(cache[key])
            want = G["score_" + metric]
            assert np.array_equal(np.isnan(scores), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.all(np.abs(np.array(scores)[ok] - want[ok]) <= 8 * g["score_measured"][0] * np.abs(want[ok])), (a, metric)
            assert tc.first_smallest(scores) == int(g["traj_o%d_%s_win_%s" % (idx, a, metric)][0]), (a, metric)


def test_rows_and_weights_equal_the_reference(golden):
    g = golden("label_trajectory")
    me = tc.Labels(SCENES["traj"])
    assert lc.unused_id(me.data) == int(g["traj_n_ids"][0]) == 9
    states = [int(g["traj_o%d_state" % i][0]) for i in range(9)]
    assert states == [2, 2, 1, 2, 2, 2, 2, 2, 1]                                # 1: boxes, but under 3 s
    for i in range(9):
        r = tc.object_rows(me, i)
        want = g["traj_o%d_rows" % i]
        assert bit_equal(np.stack([r["t"], r["x"], r["y"]], axis=1), want[:, :3]), i
        got = np.stack([r["xw"], r["yw"]], axis=1)              # the reference projects with torch.bmm: equal to the measured ulp
        assert np.all(np.abs(got - want[:, 3:]) <= 8 * g["traj_measured"][0] * want[:, 3:]), i
        assert r["duration"] == g["traj_o%d_duration" % i][0] and (r["duration"] >= 3) == (states[i] == 2)
    assert 2.9 < g["traj_o2_duration"][0] < 3 < g["traj_o3_duration"][0] < 3.1
    assert len(g["traj_o5_rows"]) == 4                                          # k + 1 boxes for x
    assert len({(d["camera"]) for f in me.data for d in f.values() if d["id"] == 4}) == 1


def test_scene_holds_the_edges_it_claims(golden):
    g = golden("label_trajectory")
    none = [bool(g["traj_s%d_none" % i][0]) for i in range(9)]
    assert none == [False, False, True, False, False, False, True, True, True]
    assert int(g["traj_o6_x_win_mpe"][0]) == -1 and int(g["traj_o6_y_win_mpe"][0]) >= 0       # every x candidate is skipped
    assert int(g["traj_o7_x_win_mpe"][0]) >= 0 and int(g["traj_o7_y_win_mpe"][0]) == -1       # x succeeds, y fails
    iers = np.concatenate([g["traj_o%d_%s_ier" % (i, a)][g["traj_o%d_%s_n" % (i, a)] - 2 * k <= lim]
                           for i in FITTED for a, k, lim in (("x", 3, 1e9), ("y", 2, 1e9))])
    assert {-2, 0} <= set(iers.tolist())
    # rejected at the first insertion round and at a later one
    rows = g["traj_o6_rows"]
    dur = np.floor(g["traj_o6_duration"][0])
    rounds = set()
    for tpe in (tc.tpe_x()[0], tc.tpe_x()[-1]):
        tr = []
        f = tc.fit(rows[:, 0], rows[:, 1], rows[:, 3], 3, tc.smoothing(tpe, len(rows)), tc.ncap_of(dur * 4 + 2, 3, len(rows)), trace=tr)
        assert f["ier"] == tc.REJECTED
        rounds.add(len(tr))
    f = tc.fit(rows[:, 0], rows[:, 1], rows[:, 3], 3, tc.smoothing(1.0, len(rows)), 9, trace=(tr := []))
    assert f["ier"] == tc.REJECTED and len(tr) == 2 and f["n"] == 9              # a cap of one knot: stopped in the second round
    f = tc.fit(rows[:, 0], rows[:, 1], rows[:, 3], 3, tc.smoothing(1.0, len(rows)), 8, trace=(tr := []))
    assert f["ier"] == tc.REJECTED and len(tr) == 1 and f["n"] == 8              # no knot allowed: stopped in the first
    assert min(rounds) > 1


def test_golden_file_holds_arrays_of_numbers_only(golden):
    g = golden("label_trajectory")
    assert all(g[k].dtype.kind in "fiub" for k in g.files)
    assert {k.split("_")[0] for k in g.files} == {"traj", "direct", "score"}
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "label_trajectory.npz")) < 1 << 20


def test_gen_trajectories_and_adjust_ts_equal_the_reference(golden):
    g = golden("label_trajectory")
    scene = SCENES["traj"]
    splines = golden_splines(g, "traj", 9)
    me = tc.Labels(scene)
    idx, val = tc.dump_xyt(tc.ref_gen_trajectories(me, splines), scene["names"])
    assert bit_equal(idx, g["traj_gen_idx"]) and bit_equal(val, g["traj_gen_val"])
    kinds = set()
    for run in (True, False):
        for metric in ("ape", "mpe"):
            me = tc.Labels(scene)
            got = tc.ref_adjust_ts(me, splines, metric=metric, use_running_error=run, overwrite_ts_data=True)
            tag = "traj_ts_%d_%s_" % (run, metric)
            idx, val = tc.dump_xyt(me.data, scene["names"])
            assert bit_equal(idx, g[tag + "idx"]) and bit_equal(val, g[tag + "val"]), tag
            assert bit_equal(lc.ts_table(me.all_ts, scene["names"]), g[tag + "all_ts"]), tag
            assert all(0 <= e[5] < 21 for e in got)
            kinds |= {len([i for i in range(9) if me.data[e[0]].get("{}_{}".format(scene["names"][e[1]], i))]) for e in got}
    frames = {(f, c) for f, frame in enumerate(scene["data"][:126]) for c in range(3)
              if any(d["camera"] == scene["names"][c] and d["id"] < 9 for d in frame.values())}
    assert 1 in kinds and len(frames) > len(got)                # an entry with one object; (frame, camera)s with none kept


def test_adjust_boxes_equals_the_later_annotator(golden):
    g = golden("label_trajectory")
    scene = tc.without_id(SCENES["traj"], 11)
    splines = golden_splines(g, "traj", 9)
    bound = 8 * g["traj_boxes_measured"][0]
    for tag, sx, sy in (("boxes", 2, 2), ("boxes_tight", 0.05, 0.02)):
        me = tc.Labels(scene)
        before = tc.dump_xyt(me.data, scene["names"])[1]
        got = np.array(tc.ref_adjust_boxes(me, splines, sx, sy))
        idx, val = tc.dump_xyt(me.data, scene["names"])
        want, shifts = g["traj_%s_val" % tag], g["traj_%s_shifts" % tag]
        assert bit_equal(idx, g["traj_%s_idx" % tag]) and bit_equal(val[:, 2], want[:, 2])
        assert np.all(np.max(np.abs(val - want), axis=0) <= bound * np.max(np.abs(want), axis=0)), tag
        assert got.shape == shifts.shape and np.max(np.abs(got - shifts)) <= bound * np.max(shifts), tag
        moved = np.any(val[:, :2] != before[:, :2], axis=1)
        reach = np.array([splines[i][0] is not None and f <= scene["last_frame"] for f, _, i in idx])
        assert np.array_equal(moved, reach) and len(got) == moved.sum() and not reach[idx[:, 0] > scene["last_frame"]].any()
    loose, tight = g["traj_boxes_shifts"], g["traj_boxes_tight_shifts"]
    assert np.all(tight <= loose * (1 + 1e-12)) and (tight < loose).mean() > 0.9      # the tight limits clamp nearly every box
    assert len(SCENES["traj"]["data"]) - 1 > SCENES["traj"]["last_frame"]             # frames behind last_frame stay as they are
    with pytest.raises(IndexError):                                                   # the ignored id has no entry in splines
        tc.ref_adjust_boxes(tc.Labels(SCENES["traj"]), splines)


def test_host_weights_are_the_restatement_s():
    import label_trajectory as lt
    me = tc.Labels(SCENES["traj"])
    pack = lt.pack_objects(me, range(9))
    P1, P2 = tc.rc.tables(me.hg, me.seq_keys)
    want = tc.box_weights(pack["state6"], pack["cam"], P1, P2)
    assert bit_equal(lt.host_weights(pack["state6"], pack["cam"], P1, P2), want[:, :2])
    assert bit_equal(lt.host_weights(pack["state6"], pack["cam"], P1, None), tc.box_weights(pack["state6"], pack["cam"], P1, None)[:, :2])


def test_smoothing_factor_is_torch_s_fp32_product():
    import label_trajectory as lt
    for m in (4, 120, 181):
        interp = torch.ones(m, dtype=torch.int64)
        for tpe in tc.tpe_x()[::7] + tc.tpe_y()[::7]:
            want = float(tpe ** 2 * sum(interp))                # the reference's expression, :1236
            assert tc.smoothing(tpe, m) == want == float(lt.smoothing(tpe, m))
    assert bit_equal(lt.smoothing(tc.tpe_x(), 50).astype(np.float64), np.array([tc.smoothing(v, 50) for v in tc.tpe_x()]))
    assert bit_equal(lt.tpe_x(), np.array(tc.tpe_x())) and bit_equal(lt.tpe_y(), np.array(tc.tpe_y()))


def test_spline_object_on_the_host(golden):
    import label_trajectory as lt
    g = golden("label_trajectory")
    t, c = g["traj_s0_x_t"], g["traj_s0_x_c"]
    sp = lt.Spline(t, c, 3, ier=0, fp=1.5)
    assert bit_equal(sp.get_knots(), t[3:-3]) and bit_equal(sp.get_coeffs(), c) and sp.get_residual() == 1.5
    assert (sp.k, sp.ier) == (3, 0) and len(sp.c) == len(sp.t) == len(t)
    for x in (0.0, -3.5, float(t[0]), 1.234, float(t[-1]), 99.0, np.float64(2.5)):
        got = sp(x)
        assert isinstance(got, np.ndarray) and got.shape == () and got.item() == tc.value(t, sp.c, len(t), 3, float(x))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                                       # arrays go through the device
            sp([1.0, 2.0])
    with pytest.raises(ValueError):
        lt.Spline(t, c, 4)
    m50, m10 = lt._end_multipliers(3)
    assert m50.tolist() == [50, 1, 50] and m10.tolist() == [1, 10, 1]
    m50, m10 = lt._end_multipliers(2)
    assert m50.tolist() == [50, 50] and m10.tolist() == [10, 10]
    for m in (2, 3, 4, 9):
        w = np.linspace(1, 2, m)
        m50, m10 = lt._end_multipliers(m)
        assert bit_equal((w * m50) * m10, tc.end_weighted(w))


def test_packing_and_plan_equal_the_restatement():
    import label_trajectory as lt
    me = tc.Labels(SCENES["traj"])
    pack = lt.pack_objects(me, range(9))
    for i in range(9):
        lo, hi = pack["off"][i], pack["off"][i + 1]
        r = tc.object_rows(me, i)
        assert bit_equal(pack["t"][lo:hi], r["t"]) and bit_equal(pack["state6"][lo:hi, 0], r["x"])
    plan = lt.plan_fits(pack, 2, 3, 4, lt.tpe_x(), lt.tpe_y())
    assert len(plan["chunks"]) == 1
    ch = plan["chunks"][0]
    assert ch["groups"] == [(i, a) for i in FITTED for a in (0, 1)]
    assert ch["waves"].shape == (7 * (4 + 2), 2) and len(ch["s"]) == 7 * 300
    for g, (i, a) in enumerate(ch["groups"]):
        r = tc.object_rows(me, i)
        k, lim = (3, np.floor(r["duration"]) * 4 + 2) if a == 0 else (2, np.floor(r["duration"]) + 2)
        assert ch["grp"][g, 3] == tc.ncap_of(lim, k, len(r["t"])) and ch["grp"][g, 2] == k and ch["grp"][g, 7] == a
    small = lt.plan_fits(pack, 2, 3, 4, lt.tpe_x(), lt.tpe_y(), budget=4 << 20)
    assert len(small["chunks"]) > 2 and sum((c["groups"] for c in small["chunks"]), []) == ch["groups"]
    for c in small["chunks"]:
        assert len(c["waves"]) * 64 * c["ncap"] * 19 * 8 <= 4 << 20


def test_refusals_come_before_any_device_work(monkeypatch):
    import label_trajectory as lt

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(lt, "_device", no_device)
    monkeypatch.setattr(lt, "_upload", no_device)
    scene = tc.scene_traj()
    for f in (3, 43):                                           # object 5 keeps two boxes 1.3 s apart
        del scene["data"][f]["p1c1_5"]
    me = tc.Labels(scene)
    lt.plan_fits(lt.pack_objects(me, range(9)), 2, 3, 4, lt.tpe_x(), lt.tpe_y())        # under 3 s now: no fit, no refusal
    scene = tc.scene_traj()
    del scene["data"][43]["p1c1_5"]                             # 3 boxes over 4 s: too few for the cubic x spline
    me = tc.Labels(scene)
    with pytest.raises(ValueError, match="object 5, axis x"):
        lt.get_splines(me)
    with pytest.raises(ValueError, match="object 5, axis x"):
        lt.create_trajectory(me, 5)
    for key, axis in (("l", "x"), ("w", "y")):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            me = tc.Labels(tc.scene_traj())
            me.data[20]["p1c1_3"][key] = bad
            before = tc.dump_xyt(me.data, me.seq_keys)
            with pytest.raises(ValueError, match="object 3, axis " + axis):
                lt.get_splines(me)
            assert me.splines is None and bit_equal(tc.dump_xyt(me.data, me.seq_keys)[1], before[1])
    me = tc.Labels(tc.scene_traj())                             # a projection that maps every corner to one pixel: weights of 0
    me.hg.hg1.correspondence["p1c2"]["P"] = np.array([[0, 0, 0, 5.0], [0, 0, 0, 7.0], [0, 0, 0, 1.0]])
    with pytest.raises(ValueError, match="object 0, axis x: a weight of 0.0"):
        lt.get_splines(me)
    assert me.splines is None
    me = tc.Labels(tc.scene_traj())
    with pytest.raises(NotImplementedError):
        lt.create_trajectory(me, 0, plot=True)
    with pytest.raises(NotImplementedError):
        lt.get_splines(me, plot=True)
    with pytest.raises(ValueError, match="orders"):
        lt.create_trajectory(me, 0, x_order=4)
    with pytest.raises(ValueError, match="trials"):
        lt.adjust_ts_with_trajectories(me, trials=64)


def test_there_is_no_cpu_path(monkeypatch):
    import label_trajectory as lt
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    me = tc.Labels(SCENES["traj"])
    with pytest.raises(RuntimeError):
        lt.get_splines(me)
    with pytest.raises(RuntimeError):
        lt.create_trajectory(me, 0)
    with pytest.raises(RuntimeError):
        lt.gen_trajectories(me)
    me.splines = [[lt.Spline(np.r_[[0.0] * 4, [5.0] * 4], [0.0, 1, 2, 3], 3), lt.Spline(np.r_[[0.0] * 3, [5.0] * 3], [0.0, 1, 2], 2)]] * 9
    with pytest.raises(RuntimeError):
        lt.adjust_ts_with_trajectories(me)
    for fn in (lambda o: o.label_box_weights(torch.zeros(1, 6, dtype=torch.float64), torch.zeros(1, dtype=torch.int32),
                                             torch.zeros(1, 12, dtype=torch.float64)),
               lambda o: o.spline_eval(torch.zeros(1, 8, dtype=torch.float64), torch.zeros(1, 8, dtype=torch.float64),
                                       torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                                       torch.zeros(1, dtype=torch.float64))):
        from retinanet_mi355x import ops
        with pytest.raises(RuntimeError):
            fn(ops)


def test_entry_points_at_every_layer():
    import label_audit
    import label_trajectory as lt
    from retinanet_mi355x import _hip, ops, torch_ops
    header = open(os.path.join(REPO, "include", "retinanet_mi355x.h")).read()
    for name in ("rn_label_box_weights", "rn_spline_fit", "rn_spline_select", "rn_spline_eval", "rn_label_ts_shift",
                 "rn_spline_fit_workspace_bytes"):
        assert name in _hip.SIGNATURES and re.search(r"\b%s\(" % name, header), name
    for name in ("label_box_weights", "spline_fit", "spline_select", "spline_eval", "label_ts_shift"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    assert (ops.SPLINE_GRP, ops.SPLINE_WS_COLS, ops.SPLINE_FIGS) == tuple(
        int(re.search(r"#define RN_SPLINE_%s (\d+)" % k, header).group(1)) for k in ("GRP", "WS_COLS", "FIGS"))
    assert (ops.SPLINE_UNUSED, ops.SPLINE_STUCK, ops.SPLINE_REJECTED) == (tc.UNUSED, tc.STUCK, tc.REJECTED)
    assert all(getattr(lt.LabelTrajectory, m) is getattr(lt, m) for m in lt.METHODS)
    assert lt.LabelTrajectory.get_unused_id is label_audit.get_unused_id and not set(lt.METHODS) & set(label_audit.METHODS)
    grp = np.array([[0, 9, 3, 12, 0, 200, 0, 0], [9, 9, 2, 10, 200, 65, 0, 1], [18, 9, 2, 10, 265, 1, 0, 1]], np.int32)
    waves = ops.spline_waves(grp)
    assert waves.tolist() == [[0, 0], [0, 64], [0, 128], [0, 192], [1, 0], [1, 64], [2, 0]] and grp[:, 6].tolist() == [0, 4, 6]
    assert ops.spline_metric("ape") == 0 and ops.spline_metric("mpe") == 1 and ops.spline_metric("anything") == 1

"""GPU: csrc/label_spline.hip (ops.label_box_weights / spline_fit / spline_select / spline_eval / label_ts_shift) and the public
label_trajectory functions on top of it, against the restatement of tests/label_trajectory_cases.py and the reference's own
output (tests/golden/label_trajectory.npz).

Device against restatement is compared BIT FOR BIT -- n, ier, residual, iteration count, knots and coefficients of every lane
(the workspace's first two columns), scores, winners, figures, evaluated values, best times: the kernels' arithmetic is fp64
with one rounding per operation in the restatement's order, so there is no tolerance to choose.  Device against the reference,
end to end: the None pattern, n, ier and the knot vectors equal; coefficients, residuals, gen_trajectories values and the
summary's figures within 8x the deviation the golden tool measured for the restatement (``traj_measured``: the reference projects
the box corners with torch.bmm, so a few weights differ in the last bit and the fits amplify that); best times of
adjust_ts_with_trajectories bit-equal (the golden tool keeps every winning trial 1e-9 clear of the others).

Shapes: direct fits of 5..39 points with k = 2 and 3, one candidate per group (a wave with one live lane), a group of 65 (a
second wave with one lane) and one of 200 (a partial fourth wave); fuzz scenes of 3 cameras x 100 frames x 6 objects with 16 + 7
candidates; chunks of one group and of all."""
import contextlib
import ctypes
import io
import re

import numpy as np
import pytest
import torch

import label_audit_cases as lc
import label_trajectory_cases as tc

pytestmark = pytest.mark.gpu
SCENES = tc.golden_scenes()
TPEX, TPEY = tc.tpe_x()[3::13], tc.tpe_y()[5::15]               # 16 and 7 candidates
FUZZ_SEEDS = (2, 3)


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same(a, b):
    """bit_equal, but a NaN is a NaN whatever its bits."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and bit_equal(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


@pytest.fixture(scope="module", autouse=True)
def registered():
    from retinanet_mi355x import torch_ops                     # registers torch.ops.retinanet_mi355x.*
    return torch_ops


@pytest.fixture(scope="module")
def Me(dev):
    import homography
    import label_audit as la
    import label_trajectory as lt

    class Me(tc.Labels, la.LabelAudit, lt.LabelTrajectory):
        def __init__(self, scene):
            tc.Labels.__init__(self, scene, homography.Homography, homography.Homography_Wrapper)
    return Me


def quiet(fn, *a, **k):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got = fn(*a, **k)
    return got, out.getvalue()


# ------------------------------------------------------------------------------------------------ the kernels, directly
def direct_tables():
    """Every direct case as a group of one candidate, case 2 again with 65 smoothing factors and case 3 with 200 -> the host
    tables of one launch and the restatement's fit of every candidate."""
    from retinanet_mi355x import ops
    tx, val, wt, s, grp, fits = [], [], [], [], [], []
    row0 = c0 = 0
    cases = [(seed, None) for seed in tc.DIRECT_SEEDS] + [(2, 65), (3, 200)]
    for seed, many in cases:
        x, y, w, k, s1 = tc.direct_case(seed)
        sv = [s1] if many is None else list(np.logspace(2, -3, many) * len(x))
        m = len(x)
        grp.append((row0, m, k, m + k + 1, c0, len(sv), 0, seed % 2))
        fits.append([tc.fit(x, y, w, k, v, m + k + 1) for v in sv])
        tx, val, wt, s = tx + list(x), val + list(y), wt + list(w), s + sv
        row0, c0 = row0 + m, c0 + len(sv)
    grp = np.array(grp, np.int32)
    waves = ops.spline_waves(grp)
    return dict(grp=grp, waves=waves, tx=np.array(tx), val=np.array(val), wt=np.array(wt), s=np.array(s), fits=fits,
                ncap=int(grp[:, 3].max()), cases=cases)


@pytest.fixture(scope="module")
def direct(dev):
    from datareader import _download, _upload
    from retinanet_mi355x import ops
    tab = direct_tables()
    up = _upload(dev, [tab[k] for k in ("grp", "waves", "tx", "val", "wt", "s")])
    ws, n, ier, fp, iters, status = ops.spline_fit(*up, tab["ncap"])
    tab["dev"] = dict(up=up, ws=ws, n=n, ier=ier, fp=fp, iters=iters, status=status)
    tab["host"] = dict(zip(("ws", "n", "ier", "fp", "iters", "status"), _download([ws[:2 * tab["ncap"]], n, ier, fp, iters, status])))
    return tab


def lanes_equal(host, grp, fits, ncap):
    for g, group_fits in enumerate(fits):
        k = int(grp[g, 2])
        for c, f in enumerate(group_fits):
            lane = int(grp[g, 6]) * 64 + c
            assert (host["n"][lane], host["ier"][lane], host["iters"][lane]) == (f["n"], f["ier"], f["iters"]), (g, c)
            assert host["fp"][lane] == f["fp"] or (np.isnan(host["fp"][lane]) and np.isnan(f["fp"])), (g, c)
            if f["ier"] <= 3:
                assert bit_equal(host["ws"][:f["n"], lane], f["t"]), (g, c)
                assert same(host["ws"][ncap:ncap + f["n"] - k - 1, lane], f["c"]), (g, c)
        pad = np.arange(int(grp[g, 6]) * 64 + len(group_fits), (int(grp[g, 6]) + (len(group_fits) + 63) // 64) * 64)
        assert np.all(host["ier"][pad] == tc.UNUSED)


def test_fit_kernel_equals_restatement_and_scipy(direct, golden):
    g = golden("label_trajectory")
    host = direct["host"]
    assert int(host["status"][0]) == 0
    lanes_equal(host, direct["grp"], direct["fits"], direct["ncap"])
    for i, seed in enumerate(tc.DIRECT_SEEDS):                  # and scipy's own numbers
        lane, n, k = int(direct["grp"][i, 6]) * 64, int(g["direct_n"][i]), int(direct["grp"][i, 2])
        assert (host["n"][lane], host["ier"][lane], host["fp"][lane]) == (n, g["direct_ier"][i], g["direct_fp"][i]), seed
        assert bit_equal(host["ws"][:n, lane], g["direct_t"][i, :n]), seed
        assert bit_equal(host["ws"][direct["ncap"]:direct["ncap"] + n - k - 1, lane], g["direct_c"][i, :n - k - 1]), seed
    assert {-2, 0, 3} <= set(host["ier"].tolist())


def test_fit_through_the_c_abi_and_torch_ops_and_a_reused_workspace(direct, dev):
    from datareader import _download
    from retinanet_mi355x import _hip, ops
    d, ncap = direct["dev"], direct["ncap"]
    grp, waves, tx, val, wt, s = d["up"]
    NW = waves.shape[0]
    lib = _hip.load()
    assert lib.rn_spline_fit_workspace_bytes(NW, ncap) == NW * 64 * ncap * 19 * 8 == ops.spline_workspace_bytes(NW, ncap)
    ws = torch.full((19 * ncap * NW * 64,), float("nan"), dtype=torch.float64, device=dev)
    n, ier, iters = (torch.empty(NW * 64, dtype=torch.int32, device=dev) for _ in range(3))
    fp = torch.empty(NW * 64, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = lib.rn_spline_fit(grp.data_ptr(), grp.shape[0], waves.data_ptr(), NW, tx.data_ptr(), val.data_ptr(), wt.data_ptr(), tx.numel(),
                           s.data_ptr(), s.numel(), ncap, ws.data_ptr(), n.data_ptr(), ier.data_ptr(), fp.data_ptr(), iters.data_ptr(),
                           status.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = dict(zip(("ws", "n", "ier", "fp", "iters", "status"), _download([ws.view(19 * ncap, NW * 64)[:2 * ncap], n, ier, fp, iters, status])))
    lanes_equal(got, direct["grp"], direct["fits"], ncap)
    again = ops.spline_fit(grp, waves, tx, val, wt, s, ncap, workspace=ws)          # the same workspace, used again
    via = torch.ops.retinanet_mi355x.spline_fit(grp, waves, tx, val, wt, s, ncap)
    for other in (again, via):
        o = dict(zip(("ws", "n", "ier", "fp", "iters", "status"), _download([other[0][:2 * ncap]] + list(other[1:]))))
        lanes_equal(o, direct["grp"], direct["fits"], ncap)
    assert lib.rn_spline_fit(grp.data_ptr(), grp.shape[0], waves.data_ptr(), NW, tx.data_ptr(), val.data_ptr(), wt.data_ptr(), tx.numel(),
                             s.data_ptr(), s.numel(), 5, ws.data_ptr(), n.data_ptr(), ier.data_ptr(), fp.data_ptr(), iters.data_ptr(),
                             status.data_ptr(), None) != 0                          # ncap below 6: refused, nothing launched


@pytest.mark.parametrize("metric", ["ape", "mpe"])
def test_select_kernel_equals_restatement(direct, metric):
    from datareader import _download
    from retinanet_mi355x import ops
    d, ncap, grp = direct["dev"], direct["ncap"], direct["grp"]
    _, _, tx, val, wt, s = d["up"]
    got = ops.spline_select(d["up"][0], tx, val, wt, wt, s.numel(), ncap, d["ws"], d["n"], d["ier"], d["fp"], metric)
    scores, win, fig, t, c, status = _download(list(got))
    via = torch.ops.retinanet_mi355x.spline_select(d["up"][0], tx, val, wt, wt, s.numel(), ncap, d["ws"], d["n"], d["ier"], d["fp"],
                                                   ops.spline_metric(metric))
    assert all(same(a, b) for a, b in zip(_download(list(via)), (scores, win, fig, t, c, status)))
    assert int(status[0]) == 0
    for g, fits in enumerate(direct["fits"]):
        r0, m, k, _, c0, nc, _, axis = (int(v) for v in grp[g])
        x, y, w = direct["tx"][r0:r0 + m], direct["val"][r0:r0 + m], direct["wt"][r0:r0 + m]
        want = [tc.score(f["t"], f["c"], f["n"], k, x, y, w, metric, axis) if f["ier"] <= 3 else float("nan") for f in fits]
        assert same(scores[c0:c0 + nc], want), g
        wi = tc.first_smallest(want)
        assert win[g, 0] == wi, g
        if wi >= 0:
            f = fits[wi]
            assert (win[g, 1], win[g, 2]) == (f["n"], f["ier"]) and bit_equal(t[g, :f["n"]], f["t"]), g
            assert same(c[g, :f["n"] - k - 1], f["c"]) and not t[g, f["n"]:].any() and not c[g, f["n"] - k - 1:].any(), g
            assert same(fig[g], np.array((f["fp"], want[wi]) + tc.figures(f["t"], f["c"], f["n"], k, x, y, w))), g


def test_eval_kernel_and_spline_object(direct, dev):
    import label_trajectory as lt
    from datareader import _download, _upload
    from retinanet_mi355x import ops
    splines, rng = [], np.random.RandomState(7)
    for g in (0, 1, 2, 5, 9):
        f, k = direct["fits"][g][0], int(direct["grp"][g, 2])
        splines.append(lt.Spline(f["t"], f["c"], k, f["ier"], f["fp"], device=dev))
    splines.insert(2, None)
    st, sc, snk = lt.pack_splines(splines)
    qs = rng.randint(-1, len(splines) + 1, 1000).astype(np.int32)                   # -1 and S: outside the table
    qt = rng.uniform(-5, 30, 1000)
    qt[:5] = (0.0, splines[0].t[0], splines[0].t[-1], -1e9, 1e9)
    up = _upload(dev, [st, sc, snk, qs, qt])
    out = _download([ops.spline_eval(*up), torch.ops.retinanet_mi355x.spline_eval(*up)])
    assert same(out[0], out[1])
    for i in range(1000):
        sp = splines[qs[i]] if 0 <= qs[i] < len(splines) else None
        if sp is None:
            assert np.isnan(out[0][i])
        else:
            assert out[0][i] == tc.value(sp.t, sp.c, len(sp.t), sp.k, float(qt[i])) == sp(float(qt[i])).item(), i
    sp = splines[0]
    xs = rng.uniform(-2, 20, (3, 17))
    batch = sp(xs)                                                                  # an array goes through the device
    assert batch.shape == (3, 17) and all(batch[i, j] == sp(xs[i, j]).item() for i in range(3) for j in range(17))
    assert bit_equal(sp(list(xs[0])), batch[0])


def test_bad_tables_set_the_status_and_touch_nothing(direct, dev):
    from datareader import _download, _upload
    from retinanet_mi355x import ops
    grp = direct["grp"][:3].copy()
    tx, val, wt, s = (direct[k] for k in ("tx", "val", "wt", "s"))
    for col, value in ((0, len(tx)), (1, 2), (2, 4), (3, 5), (3, direct["ncap"] + 1), (4, len(s)), (6, 3), (7, 2)):
        bad = grp.copy()
        bad[1, col] = value
        waves = np.array([[0, 0], [1, 0], [2, 0]], np.int32)
        up = _upload(dev, [bad, waves, tx, val, wt, s])
        ws, n, ier, fp, iters, status = ops.spline_fit(*up, direct["ncap"])
        h_ier, h_status = _download([ier, status])
        assert int(h_status[0]) & ops.LABEL_BAD_TABLE, (col, value)
        assert np.all(h_ier[64:128] == tc.UNUSED) and h_ier[0] == direct["fits"][0][0]["ier"], (col, value)
        sel = ops.spline_select(up[0], up[2], up[3], up[4], up[4], len(s), direct["ncap"], ws, n, ier, fp, "ape")
        win, st = _download([sel[1], sel[5]])
        assert win[1, 0] == -1 and int(st[0]) & ops.LABEL_BAD_TABLE
        with pytest.raises(RuntimeError, match="spline group"):
            ops.label_check(int(st[0]))
    up = _upload(dev, [grp, np.array([[0, 0], [1, 64], [5, 0]], np.int32), tx, val, wt, s])     # waves that are not their group's
    assert int(ops.spline_fit(*up, direct["ncap"])[5].item()) & ops.LABEL_BAD_TABLE
    assert int(ops.spline_fit(*direct["dev"]["up"], direct["ncap"])[5].item()) == 0             # the device is still well


# ------------------------------------------------------------------------------------------------ fuzz scenes
@pytest.fixture(scope="module", params=FUZZ_SEEDS)
def fuzz(request, Me):
    import label_trajectory as lt
    scene = tc.fuzz_scene(request.param)
    me = Me(scene)
    out = {}
    for metric in ("ape", "mpe"):
        results, kept, pack = lt.fit_objects(me, range(6), metric=metric, tpex=TPEX, tpey=TPEY, keep=True)
        want = [tc.ref_create_trajectory(tc.Labels(scene), i, metric=metric, tpex=TPEX, tpey=TPEY) for i in range(6)]
        out[metric] = (results, kept, pack, want)
    return scene, out


def test_fuzz_scene_every_lane_score_and_winner(fuzz):
    scene, out = fuzz
    fitted = 0
    for metric, (results, kept, pack, want) in out.items():
        assert len(kept) == 1
        ch = kept[0]
        host = dict(ws=ch["tc"], n=ch["n"], ier=ch["ier"], fp=ch["fp"], iters=ch["iters"])
        groups = {ga: g for g, ga in enumerate(ch["groups"])}
        for i, w in enumerate(want):
            if w is None:
                assert results[i] is None and (i, 0) not in groups
                continue
            fitted += 1
            for axis, sel in ((0, w["sel_x"]), (1, w["sel_y"])):
                g = groups[(i, axis)]
                assert ch["grp"][g, 3] == sel["ncap"]
                lanes_equal(host, ch["grp"][g:g + 1], [sel["fits"]], ch["ncap"])
                c0, nc = int(ch["grp"][g, 4]), int(ch["grp"][g, 5])
                assert same(ch["scores"][c0:c0 + nc], sel["scores"]) and ch["win"][g, 0] == sel["win"], (metric, i, axis)
                if sel["win"] >= 0:
                    f = sel["fits"][sel["win"]]
                    assert same(ch["fig"][g], np.array((f["fp"], sel["scores"][sel["win"]]) + sel["figs"])), (metric, i, axis)
            if w["x"] is None:
                assert results[i] is None
                continue
            r = results[i]
            assert bit_equal(r["t"], w["rows"]["t"])
            for a in "xy":
                sp = r[a]
                assert (len(sp.t), sp.k, sp.ier, sp.fp) == (w[a]["n"], w[a]["k"], w[a]["ier"], w[a]["fp"])
                assert bit_equal(sp.t, w[a]["t"]) and bit_equal(sp.get_coeffs(), w[a]["c"])
        lo = pack["off"][:-1]
        for i in range(6):                                      # the packed rows and the weights the fits saw
            rows = tc.object_rows(tc.Labels(scene), i)
            assert (rows is None) == (pack["off"][i] == pack["off"][i + 1])
            if rows is not None:
                assert bit_equal(pack["t"][lo[i]:pack["off"][i + 1]], rows["t"])
    assert fitted >= 6 and any(w is not None and w["x"] is None for w in out["ape"][3]) and any(w is None for w in out["ape"][3])
    rejected = [f["ier"] == tc.REJECTED for w in out["ape"][3] if w is not None for f in w["sel_x"]["fits"] + w["sel_y"]["fits"]]
    assert any(rejected) and not all(rejected)


def test_box_weights_kernel(fuzz, dev):
    import label_trajectory as lt
    from datareader import _download, _upload
    from retinanet_mi355x import ops
    scene, out = fuzz
    pack = out["ape"][2]
    P1, P2 = tc.rc.tables(tc.Labels(scene).hg, scene["names"])
    up = _upload(dev, [pack["state6"], pack["cam"], P1, P2])
    got, status = ops.label_box_weights(*up)
    via = torch.ops.retinanet_mi355x.label_box_weights(*up)
    h, h2, st = _download([got, via[0], status])
    assert int(st[0]) == 0 and bit_equal(h, h2)
    assert bit_equal(h, tc.box_weights(pack["state6"], pack["cam"], P1, P2))
    assert (pack["state6"][:, 1] > 60).any() and (pack["state6"][:, 1] < 60).any()      # both sides of the wrapper
    one, _ = ops.label_box_weights(up[0], up[1], up[2], None)
    assert bit_equal(_download([one])[0], tc.box_weights(pack["state6"], pack["cam"], P1, None))
    cam = pack["cam"].copy()
    cam[3] = 3
    got, status = ops.label_box_weights(up[0], _upload(dev, [cam])[0], up[2], up[3])
    h, st = _download([got, status])
    assert int(st[0]) == ops.LABEL_BAD_CAMERA and np.isnan(h[3]).all() and not np.isnan(np.delete(h, 3, 0)).any()


def test_chunked_and_repeated_runs_are_identical(fuzz, Me):
    import label_trajectory as lt
    scene, out = fuzz
    results = out["mpe"][0]
    for budget in (None, 1 << 18, 1):                           # all groups at once, a few per chunk, one per chunk
        again, kept, _ = lt.fit_objects(Me(scene), range(6), metric="mpe", tpex=TPEX, tpey=TPEY, budget=budget, keep=True)
        assert budget is None or len(kept) > 1
        assert budget != 1 or all(len(ch["groups"]) == 1 for ch in kept)
        for a, b in zip(results, again):
            assert (a is None) == (b is None)
            if a is not None:
                assert bit_equal(a["x"].t, b["x"].t) and bit_equal(a["x"].c, b["x"].c) and bit_equal(a["y"].c, b["y"].c)
                assert bit_equal(a["figs_x"], b["figs_x"]) and bit_equal(a["figs_y"], b["figs_y"])


@pytest.mark.parametrize("run", [True, False])
@pytest.mark.parametrize("metric", ["ape", "mpe"])
def test_ts_shift_equals_restatement(fuzz, Me, run, metric):
    scene, out = fuzz
    results, _, _, want = out["mpe"]
    me, ref = Me(scene), tc.Labels(scene)
    me.splines = [[None, None] if r is None else [r["x"], r["y"]] for r in results]
    splines = [[None, None] if w is None or w["x"] is None else [w["x"], w["y"]] for w in want]
    got, _ = quiet(me.adjust_ts_with_trajectories, metric=metric, use_running_error=run, overwrite_ts_data=True, trials=21)
    exp = tc.ref_adjust_ts(ref, splines, metric=metric, use_running_error=run, overwrite_ts_data=True)
    assert len(got) == len(exp) > 50
    assert same(np.array(got, np.float64), np.array(exp, np.float64))
    assert bit_equal(tc.dump_xyt(me.data, scene["names"])[1], tc.dump_xyt(ref.data, scene["names"])[1])
    assert bit_equal(lc.ts_table(me.all_ts, scene["names"]), lc.ts_table(ref.all_ts, scene["names"]))
    sizes = {len([i for i in range(6) if me.data[e[0]].get("{}_{}".format(scene["names"][e[1]], i))]) for e in got}
    assert 1 in sizes and max(sizes) > 1


# ------------------------------------------------------------------------------------------------ end to end against the reference
@pytest.fixture(scope="module")
def fitted(Me):
    me = Me(SCENES["traj"])
    _, text = quiet(me.get_splines)
    return me, text


def close(a, b, bound):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.max(np.abs(a - b)) <= bound * np.max(np.abs(b))


def test_get_splines_equals_the_reference(fitted, golden, Me):
    g = golden("label_trajectory")
    me, text = fitted
    dev_c, dev_fp, dev_fig = 8 * g["traj_measured"][1], 8 * g["traj_measured"][2], 8 * g["traj_measured"][4]
    assert len(me.splines) == 9
    for i, (xs, ys) in enumerate(me.splines):
        assert (xs is None) == (ys is None) == bool(g["traj_s%d_none" % i][0]), i
        if xs is None:
            continue
        for a, sp in (("x", xs), ("y", ys)):
            j = int(g["traj_o%d_%s_win_mpe" % (i, a)][0])
            assert bit_equal(sp.t, g["traj_s%d_%s_t" % (i, a)]) and sp.ier == g["traj_o%d_%s_ier" % (i, a)][j], (i, a)
            assert close(sp.get_coeffs(), g["traj_s%d_%s_c" % (i, a)], dev_c), (i, a)
            assert abs(sp.get_residual() - g["traj_o%d_%s_fp" % (i, a)][j]) <= dev_fp * g["traj_o%d_%s_fp" % (i, a)][j], (i, a)
    want = [float(v) for v in re.findall(r"[-+0-9.e]+(?=ft ase|px ape)", bytes(g["traj_summary"]).decode())]
    last = text.strip().split("\n")[-1]
    have = [float(v) for v in re.findall(r"[-+0-9.e]+(?=ft ase|px ape)", last)]
    assert last.startswith("Spline errors: ") and len(have) == 2 and all(abs(h - w) <= dev_fig * w for h, w in zip(have, want))
    assert text.count("Object ") == 5
    # create_trajectory: one object through the same launches
    for i in (0, 2, 6, 8):
        (t, xs, ys, avg_x, avg_xp), text1 = quiet(Me(SCENES["traj"]).create_trajectory, i, metric="mpe")
        if me.splines[i][0] is None:
            assert t is None and xs is None and ys is None and avg_x is None and avg_xp is None and text1 == ""
        else:
            assert bit_equal(t, g["traj_o%d_rows" % i][:, 0]) and bit_equal(xs.c, me.splines[i][0].c) and bit_equal(ys.t, me.splines[i][1].t)
            assert all(abs(h - w) <= dev_fig * w for h, w in zip((avg_x, avg_xp), g["traj_o%d_fig_mpe" % i])) and "Object 0:" in text1
    assert quiet(Me(SCENES["traj"]).create_trajectory, 0, verbose=False)[1] == ""


def test_gen_trajectories_equals_the_reference(fitted, golden, Me):
    g = golden("label_trajectory")
    me, _ = fitted
    before = tc.dump_xyt(me.data, me.seq_keys)
    me.gen_trajectories()
    idx, val = tc.dump_xyt(me.spline_data, me.seq_keys)
    assert bit_equal(idx, g["traj_gen_idx"]) and bit_equal(val[:, 2], g["traj_gen_val"][:, 2])
    for col in (0, 1):
        assert close(val[:, col], g["traj_gen_val"][:, col], 8 * g["traj_measured"][3]), col
    assert bit_equal(tc.dump_xyt(me.data, me.seq_keys)[1], before[1])           # ``data`` itself is untouched
    moved = np.any(val[:, :2] != before[1][:, :2], axis=1)
    kept = np.array([me.splines[i][0] is not None if i < 9 else False for i in idx[:, 2]])
    assert np.array_equal(moved, kept)                                          # the ignored id 11 and the spline-less stay
    fresh = Me(SCENES["traj"])                                                  # without splines: fits first, metric "ape"
    quiet(fresh.gen_trajectories)
    assert fresh.splines is None and len(fresh.spline_data) == len(fresh.data)


@pytest.mark.parametrize("run", [True, False])
@pytest.mark.parametrize("metric", ["ape", "mpe"])
def test_adjust_ts_equals_the_reference(fitted, golden, Me, run, metric):
    g = golden("label_trajectory")
    me = Me(SCENES["traj"])
    me.splines = fitted[0].splines
    report, text = quiet(me.adjust_ts_with_trajectories, metric=metric, use_running_error=run, overwrite_ts_data=True)
    tag = "traj_ts_%d_%s_" % (run, metric)
    idx, val = tc.dump_xyt(me.data, me.seq_keys)
    assert bit_equal(idx, g[tag + "idx"]) and bit_equal(val, g[tag + "val"])
    assert bit_equal(lc.ts_table(me.all_ts, me.seq_keys), g[tag + "all_ts"])
    assert all(0 <= e[5] < 21 for e in report) and text.count("shifted time by") == len(report)
    assert text.startswith("Adjusting ts for frame 0\n") and "Adjusting ts for frame 100\n" in text
    silent = Me(SCENES["traj"])
    silent.splines = me.splines
    assert quiet(silent.adjust_ts_with_trajectories, verbose=False)[1] == ""


def test_refusals_raise_before_any_launch(Me, monkeypatch):
    import label_trajectory as lt
    from retinanet_mi355x import ops

    def launched(*a, **k):
        raise AssertionError("a launch before the refusal")
    for name in ("label_box_weights", "spline_fit", "spline_select", "spline_eval", "label_ts_shift"):
        monkeypatch.setattr(ops, name, launched)
    monkeypatch.setattr(lt, "_upload", launched)
    scene = tc.scene_traj()
    del scene["data"][43]["p1c1_5"]
    with pytest.raises(ValueError, match="object 5, axis x"):
        Me(scene).get_splines()
    me = Me(tc.scene_traj())
    me.data[20]["p1c1_3"]["w"] = 0.0
    with pytest.raises(ValueError, match="object 3, axis y"):
        me.create_trajectory(3)
    with pytest.raises(NotImplementedError):
        me.create_trajectory(0, plot=True)
    assert me.splines is None
    me = Me(tc.scene_traj())                                    # every corner on one pixel: a weight of 0, found on the host
    me.hg.hg1.correspondence["p1c2"]["P"] = np.array([[0, 0, 0, 5.0], [0, 0, 0, 7.0], [0, 0, 0, 1.0]])
    with pytest.raises(ValueError, match="object 0, axis x: a weight of 0.0"):
        me.get_splines()
    me = Me(tc.scene_traj())
    me.splines = [[None, None]] * 9                             # the ignored id 11 has no entry
    with pytest.raises(IndexError):
        me.adjust_boxes_with_trajectories()


# ------------------------------------------------------------------------------------------------ every golden candidate, the later annotator, the rest of the C ABI
FITTED = (0, 1, 3, 4, 5, 6, 7)


def test_every_golden_candidate_lane_by_lane(golden, dev):
    """All 7 x (200 + 100) candidates of the golden scene in one launch, from the reference's own rows and weights: every lane's
    n, ier, residual, knots and coefficients against scipy's record, accepted / rejected, then the scores and winners."""
    from datareader import _download, _upload
    from retinanet_mi355x import ops
    g = golden("label_trajectory")
    tx, val, wt, wsc, s, grp, meta = [], [], [], [], [], [], []
    for i in FITTED:
        rows, xw2 = g["traj_o%d_rows" % i], g["traj_o%d_xw2" % i]
        m, dur = len(rows), np.floor(g["traj_o%d_duration" % i][0])
        for axis, a, k, tpes, limit, w2 in ((0, "x", 3, tc.tpe_x(), dur * 4 + 2, xw2), (1, "y", 2, tc.tpe_y(), dur + 2, rows[:, 4])):
            grp.append((len(tx), m, k, tc.ncap_of(limit, k, m), len(s), len(tpes), 0, axis))
            meta.append((i, a, k, limit))
            tx, val, wt, wsc = tx + list(rows[:, 0]), val + list(rows[:, 1 + axis]), wt + list(rows[:, 3 + axis]), wsc + list(w2)
            s += [tc.smoothing(v, m) for v in tpes]
    grp = np.array(grp, np.int32)
    waves, ncap = ops.spline_waves(grp), int(grp[:, 3].max())
    up = _upload(dev, [grp, waves, np.array(tx), np.array(val), np.array(wt), np.array(s), np.array(wsc)])
    ws, n, ier, fp, iters, status = ops.spline_fit(*up[:6], ncap)
    h_ws, h_n, h_ier, h_fp, h_status = _download([ws[:2 * ncap], n, ier, fp, status])
    assert int(h_status[0]) == 0
    compared = 0
    for gi, (i, a, k, limit) in enumerate(meta):
        G = {key: g["traj_o%d_%s_%s" % (i, a, key)] for key in ("n", "ier", "fp", "t", "c")}
        for j in range(int(grp[gi, 5])):
            lane, gn = int(grp[gi, 6]) * 64 + j, int(G["n"][j])
            if gn - 2 * k > limit:
                assert h_ier[lane] == tc.REJECTED and h_n[lane] <= gn, (i, a, j)
                continue
            compared += 1
            assert (h_n[lane], h_ier[lane], h_fp[lane]) == (gn, G["ier"][j], G["fp"][j]), (i, a, j)
            assert bit_equal(h_ws[:gn, lane], G["t"][j, :gn]) and bit_equal(h_ws[ncap:ncap + gn - k - 1, lane], G["c"][j, :gn - k - 1]), (i, a, j)
    assert compared > 1000
    for metric in ("ape", "mpe"):
        scores, win, _, _, _, st = _download(list(ops.spline_select(up[0], up[2], up[3], up[4], up[6], len(s), ncap, ws, n, ier, fp, metric)))
        assert int(st[0]) == 0
        for gi, (i, a, k, limit) in enumerate(meta):
            want = g["traj_o%d_%s_score_%s" % (i, a, metric)]
            got = scores[grp[gi, 4]:grp[gi, 4] + grp[gi, 5]]
            ok = ~np.isnan(want)
            assert np.array_equal(np.isnan(got), ~ok) and np.all(np.abs(got[ok] - want[ok]) <= 8 * g["score_measured"][0] * want[ok]), (i, a)
            assert win[gi, 0] == g["traj_o%d_%s_win_%s" % (i, a, metric)][0], (i, a, metric)


def test_adjust_boxes_equals_the_later_annotator_and_the_restatement(fitted, golden, Me, fuzz):
    g = golden("label_trajectory")
    scene = tc.without_id(SCENES["traj"], 11)
    bound = 8 * g["traj_boxes_e2e_measured"][0]                 # what the golden tool measured for the restatement end to end
    for tag, sx, sy in (("boxes", 2, 2), ("boxes_tight", 0.05, 0.02)):
        me = Me(scene)
        me.splines = fitted[0].splines
        got, text = quiet(me.adjust_boxes_with_trajectories, max_shift_x=sx, max_shift_y=sy, verbose=True)
        idx, val = tc.dump_xyt(me.data, scene["names"])
        want, shifts = g["traj_%s_val" % tag], g["traj_%s_shifts" % tag]
        assert bit_equal(idx, g["traj_%s_idx" % tag]) and bit_equal(val[:, 2], want[:, 2])
        assert np.all(np.max(np.abs(val - want), axis=0) <= bound * np.max(np.abs(want), axis=0)), tag
        assert len(got) == len(shifts) and np.max(np.abs(np.array(got) - shifts)) <= bound * np.max(shifts), tag
        assert text == "Adusted boxes for frame 0\nAdusted boxes for frame 100\n"
    with pytest.raises(IndexError):
        bad = Me(SCENES["traj"])
        bad.splines = fitted[0].splines
        bad.adjust_boxes_with_trajectories()
    # and bit for bit against the restatement, on the fuzz scene with its own splines
    fscene, out = fuzz
    results, _, _, want = out["mpe"]
    me, ref = Me(fscene), tc.Labels(fscene)
    me.splines = [[None, None] if r is None else [r["x"], r["y"]] for r in results]
    got = me.adjust_boxes_with_trajectories(max_shift_x=0.5, max_shift_y=1)
    exp = tc.ref_adjust_boxes(ref, [[None, None] if w is None or w["x"] is None else [w["x"], w["y"]] for w in want], 0.5, 1)
    assert len(got) == len(exp) > 100 and bit_equal(np.array(got), np.array(exp))
    assert bit_equal(tc.dump_xyt(me.data, fscene["names"])[1], tc.dump_xyt(ref.data, fscene["names"])[1])


def test_three_boxes_share_their_end_weights(Me):
    """x_order = 2 with three boxes over more than 3 s: [0, -1] and [1, -2] are (0, 2) and (1, 1) -- the middle box is multiplied by
    10 once -- and n = nmin = nmax from the start."""
    import label_trajectory as lt
    s = lc.empty_scene(3, 130, seed=77)
    for f, x, y in ((0, 10.0, 30.0), (50, 31.0, 30.4), (100, 49.5, 31.1)):
        lc.put(s, f, 0, 0, x, y)
    s["hg_old"] = tc.rc.hg_spec(s["names"])
    results, kept, pack = lt.fit_objects(Me(s), [0], x_order=2, tpex=TPEX, tpey=TPEY, keep=True)
    w = tc.ref_create_trajectory(tc.Labels(s), 0, x_order=2, tpex=TPEX, tpey=TPEY)
    ch = kept[0]
    assert len(pack["t"]) == 3 and w["x"] is not None and results[0] is not None
    for g, sel in enumerate((w["sel_x"], w["sel_y"])):
        lanes_equal(dict(ws=ch["tc"], n=ch["n"], ier=ch["ier"], fp=ch["fp"], iters=ch["iters"]), ch["grp"][g:g + 1], [sel["fits"]], ch["ncap"])
        c0, nc = int(ch["grp"][g, 4]), int(ch["grp"][g, 5])
        assert same(ch["scores"][c0:c0 + nc], sel["scores"]) and ch["win"][g, 0] == sel["win"] >= 0
    assert bit_equal(tc.end_weighted(np.ones(3)), np.array([50.0, 10.0, 50.0]))
    with pytest.raises(ValueError, match="object 0, axis x"):                   # the cubic needs four
        lt.fit_objects(Me(s), [0], tpex=TPEX, tpey=TPEY)


def shift_tables(direct, E=70, seed=5):
    import label_trajectory as lt
    rng = np.random.RandomState(seed)
    splines = [lt.Spline(direct["fits"][g][0]["t"], direct["fits"][g][0]["c"], int(direct["grp"][g, 2])) for g in range(12)]
    st, sc, snk = lt.pack_splines(splines)
    sizes = rng.randint(1, 6, E)
    sizes[:3] = (1, 1, 5)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    rs = rng.randint(0, len(splines), off[-1]).astype(np.int32)
    rx = rng.uniform(-5, 5, off[-1])
    base, run = rng.uniform(0, 15, E), rng.uniform(-0.05, 0.05, E)
    return splines, [st, sc, snk, off, rs, rx, base, run]


@pytest.mark.parametrize("trials", [1, 21, 63])
def test_ts_shift_kernel_directly(direct, dev, trials):
    from datareader import _download, _upload
    from retinanet_mi355x import ops
    splines, host = shift_tables(direct)
    shifts = np.linspace(-0.01, 0.01, trials)
    up = _upload(dev, host + [shifts])
    off, rs, rx, base, run = host[3:]
    dicts = [dict(t=s.t, c=s.c, n=len(s.t), k=s.k) for s in splines]
    for use_run in (True, False):
        for metric in ("ape", "mpe"):
            got = _download(list(ops.label_ts_shift(*up, use_run=use_run, metric=metric)))
            via = _download(list(torch.ops.retinanet_mi355x.label_ts_shift(*up, use_run, ops.spline_metric(metric))))
            assert all(same(a, b) for a, b in zip(got, via)) and int(got[3][0]) == 0
            for e in range(len(base)):
                rows = range(off[e], off[e + 1])
                bt, be, ie, bi = tc.ts_shift_entry([dicts[rs[r]] for r in rows], [rx[r] for r in rows], float(base[e]), float(run[e]),
                                                   shifts, use_run, metric)
                assert (got[0][e], got[1][e, 0], got[1][e, 1], got[2][e]) == (bt, be, ie, bi), (e, use_run, metric)
    # a row range out of order, a spline index outside the table: left out, flagged, nothing else disturbed
    good = _download(list(ops.label_ts_shift(*up)))
    bad_off, bad_rs = off.copy(), rs.copy()
    bad_off[2] = off[3] + 1
    bad_rs[off[5]] = len(splines)
    for tables, hit, touched in (([bad_off, rs], (2,), (1, 2)), ([off, bad_rs], (5,), (5,))):     # entry 1 only gets other rows
        up2 = _upload(dev, host[:3] + tables + host[5:] + [shifts])
        bt, errs, bi, status = _download(list(ops.label_ts_shift(*up2)))
        assert int(status[0]) == ops.LABEL_BAD_TABLE and all(bi[e] == -1 for e in hit)
        keep = np.setdiff1d(np.arange(len(base)), touched)
        assert bit_equal(bt[keep], good[0][keep]) and bit_equal(bi[keep], good[2][keep])
        assert all(np.isnan(bt[e]) or bt[e] == base[e] for e in hit)


def test_the_other_kernels_through_the_c_abi(direct, dev):
    from datareader import _download, _upload
    from retinanet_mi355x import _hip, ops
    lib, stream = _hip.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d, ncap, grp = direct["dev"], direct["ncap"], direct["grp"]
    g_, _, tx, val, wt, s = d["up"]
    G, NC, NL = grp.shape[0], s.numel(), d["n"].numel()
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # rn_spline_select
    scores, win, fig, t, c = e(NC, torch.float64), e((G, 3), torch.int32), e((G, 5), torch.float64), e((G, ncap), torch.float64), e((G, ncap), torch.float64)
    assert lib.rn_spline_select(g_.data_ptr(), G, tx.data_ptr(), val.data_ptr(), wt.data_ptr(), wt.data_ptr(), tx.numel(), NC, NL // 64, ncap,
                                d["ws"].data_ptr(), d["n"].data_ptr(), d["ier"].data_ptr(), d["fp"].data_ptr(), 1, scores.data_ptr(),
                                win.data_ptr(), fig.data_ptr(), t.data_ptr(), c.data_ptr(), status.data_ptr(), stream) == 0
    want = ops.spline_select(g_, tx, val, wt, wt, NC, ncap, d["ws"], d["n"], d["ier"], d["fp"], "mpe")
    assert all(same(a, b) for a, b in zip(_download([scores, win, fig, t, c]), _download(list(want[:5]))))
    # rn_spline_eval and rn_label_ts_shift
    splines, host = shift_tables(direct)
    shifts = np.linspace(-0.01, 0.01, 21)
    up = _upload(dev, host + [shifts, host[4], host[5]])
    st, sc, snk, off, rs, rx, base, run, sh, qs, qt = up
    out = e(qs.numel(), torch.float64)
    assert lib.rn_spline_eval(st.data_ptr(), sc.data_ptr(), snk.data_ptr(), st.shape[0], st.shape[1], qs.data_ptr(), qt.data_ptr(), qs.numel(),
                              out.data_ptr(), stream) == 0
    assert same(_download([out])[0], _download([ops.spline_eval(st, sc, snk, qs, qt)])[0])
    E = base.numel()
    bt, errs, bi = e(E, torch.float64), e((E, 2), torch.float64), e(E, torch.int32)
    assert lib.rn_label_ts_shift(st.data_ptr(), sc.data_ptr(), snk.data_ptr(), st.shape[0], st.shape[1], off.data_ptr(), rs.data_ptr(),
                                 rx.data_ptr(), E, rs.numel(), base.data_ptr(), run.data_ptr(), sh.data_ptr(), 21, 1, 0, bt.data_ptr(),
                                 errs.data_ptr(), bi.data_ptr(), status.data_ptr(), stream) == 0
    assert all(same(a, b) for a, b in zip(_download([bt, errs, bi]), _download(list(ops.label_ts_shift(st, sc, snk, off, rs, rx, base, run, sh))[:3])))
    assert lib.rn_label_ts_shift(st.data_ptr(), sc.data_ptr(), snk.data_ptr(), st.shape[0], st.shape[1], off.data_ptr(), rs.data_ptr(),
                                 rx.data_ptr(), E, rs.numel(), base.data_ptr(), run.data_ptr(), sh.data_ptr(), 64, 1, 0, bt.data_ptr(),
                                 errs.data_ptr(), bi.data_ptr(), status.data_ptr(), stream) != 0       # 64 trials: refused
    # rn_label_box_weights
    rng = np.random.RandomState(3)
    n = 300
    cam = rng.randint(0, 3, n).astype(np.int32)
    y = np.where(rng.rand(n) < 0.5, rng.uniform(10, 50, n), rng.uniform(70, 110, n))
    state = np.stack([60.0 * cam + rng.uniform(-10, 80, n), y, rng.uniform(12, 60, n), rng.uniform(5, 9, n), rng.uniform(4, 13, n),
                      np.where(y < 60, 1.0, -1.0)], axis=1)
    spec = tc.rc.hg_spec(lc.camera_names(3), seed=9)
    P1, P2 = (np.stack([spec[k][c].reshape(12) for c in lc.camera_names(3)]) for k in ("P1", "P2"))
    d_state, d_cam, d_P1, d_P2 = _upload(dev, [state, cam, P1, P2])
    out = e((n, 4), torch.float64)
    assert lib.rn_label_box_weights(d_state.data_ptr(), d_cam.data_ptr(), n, d_P1.data_ptr(), d_P2.data_ptr(), 3, out.data_ptr(),
                                    status.data_ptr(), stream) == 0
    h = _download([out, status])
    assert int(h[1][0]) == 0 and bit_equal(h[0], tc.box_weights(state, cam, P1, P2))

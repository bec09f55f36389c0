"""GPU: csrc/label_quality.hip (ops.label_series / label_group_rmse) and the public label_quality functions on top of it,
against the reference's own output (tests/golden/label_quality.npz) and the restatement of tests/label_quality_cases.py.

Everything that involves only IEEE operations -- the sorted order, the keep flags, the counts, the range, the variation, the
feasible fractions, t, x, y, v, vy, a -- is compared BIT FOR BIT.  theta goes through atan2 and is compared at
qc.theta_bound; an RMSE is compared at qc.rmse_bound (the reference's torch.mean does not sum in row order).  Both bounds are
derived in tests/label_quality_cases.py, not measured.

Shapes: the edge table holds objects of 1, 2, 63, 64, 65, 255, 256, 257 and 513 rows (the wave, workgroup and power-of-two
padding edges of the sort and of the scans), a row exactly 0.01 s behind its predecessor and one an ulp short of it, a
reverse-sorted object, exact timestamp ties across two cameras, an object the lane filter empties and one it halves; all in
ONE launch, and again with the LDS row cap below their sizes, which sends them through the global-memory sort: the outputs
must be the same bytes.  The 50 fuzz scenes have 3 to 5 cameras, at most 60 frames and 8 ids."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import label_audit_cases as lc
import label_quality_cases as qc

pytestmark = pytest.mark.gpu
SCENES = qc.golden_scenes()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_quality.npz")
LANE = (50.0, 60.0)
N_CAM = 2
EXACT = ("order", "keep", "counts", "figs", "t", "x", "y", "v", "vy", "a")


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def Me(dev):
    import label_quality as lq

    class Me(qc.rc.Labels, lq.LabelQuality):
        pass
    return Me


def quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


# ------------------------------------------------------------------------------------------------ ops.label_series
def run_series(dev, offsets, cols, n_cam, lane=None, lds_rows=None):
    from retinanet_mi355x import ops
    got = ops.label_series(torch.from_numpy(offsets).to(dev), torch.from_numpy(cols).to(dev), n_cam, lane, lds_rows)
    order, keep, ser, counts, figs, status = (t.cpu().numpy() for t in got)
    ops.label_check(int(status[0]))
    out = dict(order=order, keep=keep, counts=counts, figs=figs)
    out.update(zip(("t", "x", "y", "v", "vy", "a", "theta"), ser))
    return out


def want_series(offsets, cols, n_cam, lane=None):
    order, keep, ser, counts, figs, _ = qc.series_table(offsets, cols, n_cam, lane)
    out = dict(order=order, keep=keep, counts=counts, figs=figs)
    out.update(zip(("t", "x", "y", "v", "vy", "a", "theta"), ser))
    return out


def check_series(got, want, tag):
    for k in EXACT:
        assert bit_equal(got[k], want[k]), (tag, k)
    bound = np.array([qc.theta_bound(t) for t in want["theta"]])
    assert np.all(np.abs(got["theta"] - want["theta"]) <= bound), (tag, "theta")


def edge_table():
    """-> (offsets, cols) of the edge objects, two cameras each, and their names in object order."""
    rng = np.random.RandomState(77)
    objs, names = [], []

    def add(name, cam0, cam1=()):
        names.append(name)
        objs.append((np.array([0, len(cam0), len(cam0) + len(cam1)], np.int64), np.array(list(cam0) + list(cam1), np.float64).reshape(-1, 3)))
    add("one row", [(5.0, 55.0, 1.0)])
    add("two rows", [(5.0, 55.0, 1.0)], [(4.0, 55.5, 1.5)])
    add("two rows closer than 0.01 s", [(5.0, 55.0, 1.0), (4.0, 55.0, 1.005)])
    add("exactly two kept rows of three", [(5.0, 55.0, 1.0), (4.5, 55.0, 1.002)], [(4.0, 55.0, 1.3)])
    for n in (63, 64, 65, 255, 256, 257, 513):
        t = np.sort(rng.uniform(0.0, n * 0.02, n))              # gaps on both sides of 0.01 s
        x = 900.0 - 80.0 * t + rng.normal(0, 0.4, n)
        y = rng.uniform(45.0, 65.0, n)
        cam = rng.rand(n) < 0.5                                 # each camera's rows ascend; their concatenation does not
        rows = np.stack([x, y, t], 1)
        add("%d rows" % n, rows[cam], rows[~cam])
    t0 = 1.25
    add("a row at t + 0.01 exactly", [(9.0, 55.0, t0), (8.0, 55.0, t0 + 0.01), (7.0, 55.0, 2.0)])
    add("a row an ulp below t + 0.01", [(9.0, 55.0, t0), (8.0, 55.0, float(np.nextafter(t0 + 0.01, 0.0))), (7.0, 55.0, 2.0)])
    add("reverse-sorted", [(float(k), 55.0 + 0.01 * k, 9.0 - 0.03 * k) for k in range(100)])
    add("ties across two cameras", [(10.0, 55.0, 1.0), (9.0, 55.0, 2.0), (8.0, 55.0, 3.0)], [(10.5, 55.0, 1.0), (9.5, 55.0, 2.0), (8.5, 55.0, 3.0)])
    add("emptied by the lane", [(float(k), 10.0, 0.1 * k) for k in range(70)])
    add("halved by the lane", [(200.0 - 3.0 * k, 55.0 if k % 2 else 10.0, 0.04 * k) for k in range(130)])
    add("no rows", [])
    offsets, cols = qc.join_tables(objs)
    return offsets, cols, names


@pytest.fixture(scope="module")
def edges(dev):
    offsets, cols, names = edge_table()
    runs = {(lane, cap): run_series(dev, offsets, cols, N_CAM, lane, cap) for lane in (None, LANE) for cap in (None, 32, 2)}
    return offsets, cols, names, runs


def test_edge_scenes_against_the_restatement(edges):
    offsets, cols, names, runs = edges
    for lane in (None, LANE):
        want = want_series(offsets, cols, N_CAM, lane)
        check_series(runs[(lane, None)], want, lane)
    counts = dict(zip(names, runs[(None, None)]["counts"].tolist()))
    assert counts["one row"][:2] == [1, 1] and counts["two rows"][:2] == [2, 2] and counts["two rows closer than 0.01 s"][:2] == [2, 1]
    assert counts["exactly two kept rows of three"][:2] == [3, 2]
    assert counts["a row at t + 0.01 exactly"][1] == 3 and counts["a row an ulp below t + 0.01"][1] == 2
    assert counts["513 rows"][0] == 513 and 1 < counts["513 rows"][1] < 513 and counts["no rows"] == [0, 0, 0]
    first = offsets[:-1:N_CAM]
    s0 = int(first[names.index("ties across two cameras")])
    assert (runs[(None, None)]["order"][s0:s0 + 6] - s0).tolist() == [0, 3, 1, 4, 2, 5]
    s0 = int(first[names.index("reverse-sorted")])
    assert (runs[(None, None)]["order"][s0:s0 + 100] - s0).tolist() == list(range(99, -1, -1))
    laned = dict(zip(names, runs[(LANE, None)]["counts"].tolist()))
    assert laned["emptied by the lane"] == [0, 0, 0] and laned["halved by the lane"][0] == 65


@pytest.mark.parametrize("cap", [32, 2])
def test_global_memory_sort_gives_the_same_bytes(edges, cap):
    """lds_rows below the objects' sizes: they are sorted in the global workspace by the same network."""
    runs = edges[3]
    for lane in (None, LANE):
        for k in EXACT + ("theta",):
            assert bit_equal(runs[(lane, cap)][k], runs[(lane, None)][k]), (lane, k)


# ------------------------------------------------------------------------------------------------ golden scenes
def test_golden_scenes(dev, Me, golden):
    for name, scene in SCENES.items():
        g = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "_")}
        x_var, x_range = quiet(Me(scene).calculate_total_variation)
        assert all(type(v) is np.float64 for v in x_var + x_range)
        assert bit_equal(np.array(x_var), g["x_var"]) and bit_equal(np.array(x_range), g["x_range"])
        assert bit_equal(np.array(Me(scene).calculate_feasibility()), g["feasible"])
        kin = Me(scene).kinematics()
        assert [k["id"] for k in kin] == g["ids"].tolist()
        for j, k in enumerate(kin):
            a, b = g["off"][j], g["off"][j + 1]
            for key in ("time", "v", "a"):
                assert bit_equal(k[key], g[key][a:b]), (name, k["id"], key)
            assert np.all(np.abs(k["theta"] - g["theta"][a:b]) <= [qc.theta_bound(t) for t in g["theta"][a:b]]), (name, k["id"])
        want = qc.ref_kinematics(qc.rc.Labels(scene))
        assert [k["length"] for k in kin] == [w[7] for w in want]
        rmse, per = quiet(Me(scene).annotator_rmse)
        assert len(per) == len(g["rmse_groups"])
        for i in range(len(per)):
            assert abs(per[i] - g["rmse_groups"][i]) <= qc.rmse_bound(int(g["rmse_counts"][i]), float(g["rmse_largest"][i])), (name, i)
        assert abs(rmse - g["rmse"][0]) <= qc.rmse_bound(int(g["rmse_counts"].max()), float(g["rmse_largest"].max()))
        offsets, cols, _ = qc.table(scene["data"], scene["names"])
        C = len(scene["names"])
        check_series(run_series(dev, offsets, cols, C), want_series(offsets, cols, C), name)


def test_quality_report_and_kinematics_with_a_lane(Me):
    import label_audit as la
    scene = SCENES["score"]
    rep = quiet(Me(scene).quality_report)
    x_var, x_range = qc.ref_total_variation(qc.rc.Labels(scene))
    fr = qc.ref_feasibility(qc.rc.Labels(scene))
    xe, ye = quiet(la.estimate_projection_error, Me(scene))
    assert rep["v_total"] == sum(x_var) / sum(x_range) and rep["feasible"] == sum(fr) / len(fr)
    assert rep["ccde_x"] == sum(xe) / len(xe) and rep["ccde_y"] == sum(ye) / len(ye)
    lane = (82, 98)                                             # the reference's default lane
    kin, want = Me(scene).kinematics(lane=lane), qc.ref_kinematics(qc.rc.Labels(scene), lane)
    assert 0 < len(want) < 14 and [k["id"] for k in kin] == [w[0] for w in want]
    for k, w in zip(kin, want):
        for col, key in ((1, "time"), (2, "x"), (3, "y"), (4, "v"), (5, "a")):
            assert bit_equal(k[key], np.array(w[col])), (k["id"], key)
        assert k["length"] == w[7]
    with pytest.raises(NotImplementedError):
        Me(scene).kinematics(smooth=3)
    with pytest.raises(NotImplementedError):
        Me(scene).kinematics(plot=True)


# ------------------------------------------------------------------------------------------------ fuzz
def test_fuzz_scenes(dev, Me):
    tried = raised = 0
    for seed in range(50):
        scene = qc.fuzz_scene(seed)
        offsets, cols, _ = qc.table(scene["data"], scene["names"])
        C = len(scene["names"])
        lane = (20.0, 100.0) if seed % 2 else None
        check_series(run_series(dev, offsets, cols, C, lane), want_series(offsets, cols, C, lane), seed)
        x_var, x_range = Me(scene).calculate_total_variation(verbose=False)
        w_var, w_range = qc.ref_total_variation(qc.rc.Labels(scene))
        assert bit_equal(np.array(x_var), np.array(w_var)) and bit_equal(np.array(x_range), np.array(w_range)), seed
        assert bit_equal(np.array(Me(scene).calculate_feasibility()), np.array(qc.ref_feasibility(qc.rc.Labels(scene)))), seed
        if lc.unused_id(scene["data"]) < qc.GROUP:
            with pytest.raises(ValueError):
                Me(scene).annotator_rmse(verbose=False)
            raised += 1
            continue
        rmse, per = Me(scene).annotator_rmse(verbose=False)
        w_rmse, w_per, counts, largest = qc.ref_annotator_rmse(qc.rc.Labels(scene))
        assert len(per) == len(w_per)
        for i in range(len(per)):
            assert abs(per[i] - w_per[i]) <= qc.rmse_bound(counts[i], largest[i]), (seed, i)
        assert abs(rmse - w_rmse) <= qc.rmse_bound(max(counts), max(largest)), seed
        tried += 1
    assert tried >= 10 and raised >= 1


# ------------------------------------------------------------------------------------------------ ops.label_group_rmse
def test_group_rmse_sizes_and_sides(dev):
    """Groups of 1, 64 and 65 boxes (one staged chunk of the ascending sum is 256 terms; 300 crosses it), and a group whose
    boxes all lie beyond y = 60: the wrapper's second side."""
    from retinanet_mi355x import ops
    rng = np.random.RandomState(9)
    names = lc.camera_names(3)
    P1, P2 = (np.stack([qc.rc.hg_spec(names)[k][n].reshape(12) for n in names]) for k in ("P1", "P2"))
    sizes, cams, west = [1, 64, 65, 300, 40], [0, 1, 2, 1, 2], [False, False, False, False, True]
    states = []
    for n, c, w in zip(sizes, cams, west):
        x = 60.0 * c + rng.uniform(0, 60, n)
        y = rng.uniform(70, 110, n) if w else rng.uniform(5, 50, n)
        states.append(np.stack([x, y, rng.uniform(12, 22, n), rng.uniform(5, 8, n), rng.uniform(4, 7, n), np.full(n, -1.0 if w else 1.0)], 1))
    state = np.concatenate(states).astype(np.float32)
    group = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    cam = np.repeat(np.array(cams, np.int32), sizes)
    up = [torch.from_numpy(a).to(dev) for a in (state, group, cam, P1.reshape(-1, 3, 4), P2.reshape(-1, 3, 4))]
    im = ops.hg_to_im(up[0], up[3], up[4], up[2], from_state=True)
    rmse, mean, count, status = ops.label_group_rmse(im, up[1], len(sizes) + 1)       # one more group than ids: empty
    ops.label_check(status.cpu())
    rmse, mean, count = rmse.cpu().numpy(), mean.cpu().numpy(), count.cpu().numpy()
    assert count.tolist() == sizes + [0] and np.isnan(rmse[-1]) and np.isnan(mean[-1]).all()
    for g, (st, c) in enumerate(zip(states, cams)):
        corners = qc.image_pos(st.astype(np.float32).astype(np.float64), P1[c], P2[c])
        want, (mx, my) = qc.group_rmse(corners)
        largest = max(abs(v) for cn in corners for v in cn)
        assert abs(rmse[g] - want) <= qc.rmse_bound(sizes[g], largest), g
        assert abs(mean[g, 0] - mx) <= qc.rmse_bound(sizes[g], largest) and abs(mean[g, 1] - my) <= qc.rmse_bound(sizes[g], largest)
    assert rmse[0] == 0.0 and np.all(rmse[1:-1] > 0)
    with pytest.raises(RuntimeError):                           # ids that do not ascend
        _, _, _, status = ops.label_group_rmse(im, torch.flip(up[1], [0]).contiguous(), len(sizes))
        ops.label_check(status.cpu())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev, Me):
    from retinanet_mi355x import ops
    offsets, cols, _ = edge_table()
    d_off, d_cols = torch.from_numpy(offsets).to(dev), torch.from_numpy(cols).to(dev)
    with pytest.raises(RuntimeError):
        ops.label_series(torch.from_numpy(offsets), torch.from_numpy(cols), N_CAM)              # CPU tensors
    with pytest.raises(RuntimeError):
        ops.label_series(d_off.int(), d_cols, N_CAM)                                            # offsets int32
    with pytest.raises(RuntimeError):
        ops.label_series(d_off, d_cols.float(), N_CAM)                                          # cols fp32
    with pytest.raises(RuntimeError):
        ops.label_series(d_off, d_cols, (len(offsets) - 1) // 2 + 1)                            # n_cam does not divide the tracklets
    with pytest.raises(RuntimeError):
        ops.label_series(d_off, d_cols, N_CAM, lds_rows=48)                                     # not a power of two
    with pytest.raises(RuntimeError):
        ops.label_series(d_off, d_cols, N_CAM, lds_rows=8192)
    with pytest.raises(RuntimeError):                                                           # offsets that do not end at R
        status = ops.label_series(d_off, d_cols[:-1].contiguous(), N_CAM)[5]
        ops.label_check(status.cpu())
    im, grp = torch.zeros((4, 8, 2), dtype=torch.float64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.label_group_rmse(im, grp, 1)                                                        # CPU tensors
    with pytest.raises(RuntimeError):
        ops.label_group_rmse(im.to(dev).float(), grp.to(dev), 1)
    with pytest.raises(RuntimeError):
        ops.label_group_rmse(im.to(dev), grp.to(dev).long(), 1)
    with pytest.raises(RuntimeError):
        ops.label_group_rmse(im.to(dev)[:3], grp.to(dev), 1)
    few = lc.scene_few()                                                                        # two ids
    few["hg_old"] = qc.rc.hg_spec(few["names"])
    with pytest.raises(ValueError):
        Me(few).annotator_rmse()

"""GPU: detection -> track association (csrc/track_assoc.hip, ops.track_cost / linear_sum_assignment / match,
mc3d_track.TrackManager) against the reference's own outputs in tests/golden/tracker_assoc.npz and against the Python
restatement of scipy's solver in tests/track_cases.py."""
import itertools

import numpy as np
import pytest
import torch

import track_cases as tc

pytestmark = pytest.mark.gpu


def _lsa(cost, dev):
    from retinanet_mi355x import ops
    r, c = ops.linear_sum_assignment(torch.from_numpy(np.ascontiguousarray(cost)).to(dev))
    assert r.is_cuda and c.is_cuda and r.dtype == torch.int64 and c.dtype == torch.int64
    return r.cpu().numpy(), c.cpu().numpy()


def test_lsap_equals_scipy_goldens(dev, golden):
    g = golden("tracker_assoc")
    for name, cost in tc.lsap_cases():
        r, c = _lsa(cost, dev)
        assert np.array_equal(r, g["lsap_%s_row" % name]), name
        assert np.array_equal(c, g["lsap_%s_col" % name]), name


def test_lsap_fuzz_equals_restatement(dev):
    bad = []
    for t, cost in enumerate(tc.fuzz_matrices()):
        want = tc.lsap_restated(cost)
        got = _lsa(cost, dev)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            bad.append(t)
    assert not bad, bad[:20]


def test_lsap_is_optimal_by_brute_force(dev):
    for t, cost in enumerate(tc.fuzz_matrices(300, seed=5000)):
        n, m = cost.shape
        if max(n, m) > 7:
            continue
        r, c = _lsa(cost, dev)
        got = cost[r, c].sum()
        k = min(n, m)
        if n <= m:
            best = min(sum(cost[i, p[i]] for i in range(k)) for p in itertools.permutations(range(m), k))
        else:
            best = min(sum(cost[p[j], j] for j in range(k)) for p in itertools.permutations(range(n), k))
        assert len(r) == k and abs(got - best) <= 1e-12 * max(1.0, abs(best)), (t, got, best)


def test_lsap_errors_gate_and_limits(dev):
    from retinanet_mi355x import ops
    c = np.ones((3, 4))
    for badv in (np.nan, -np.inf):
        x = c.copy()
        x[1, 2] = badv
        with pytest.raises(ValueError, match="invalid numeric entries"):
            _lsa(x, dev)
        rm, info = ops.match(torch.from_numpy(x).to(dev), np.inf, info=True)
        assert info.cpu().tolist() == [0, ops.LSAP_INVALID] and (rm.cpu() == -1).all()
    x = np.full((3, 3), np.inf)
    x[0, 0] = x[1, 1] = 1.0                                     # row 2 can only take an infinite column
    with pytest.raises(ValueError, match="infeasible"):
        _lsa(x, dev)
    rm, info = ops.match(torch.from_numpy(x).to(dev), np.inf, info=True)
    assert info.cpu().tolist() == [0, ops.LSAP_INFEASIBLE] and (rm.cpu() == -1).all()
    # the gate: strict `cost > max_cost`, also on a tall (transposed) problem
    x = np.array([[0.2, 0.9, 1.0], [0.95, 0.5, 1.0], [1.0, 1.0, 0.9]])
    rm = ops.match(torch.from_numpy(x).to(dev), 0.9).cpu().tolist()
    assert rm == [0, 1, 2]
    rm = ops.match(torch.from_numpy(x).to(dev), np.nextafter(0.9, 0)).cpu().tolist()
    assert rm == [0, 1, -1]
    rm, info = ops.match(torch.from_numpy(np.array([[0.3], [0.1], [0.95]])).to(dev), 0.2, info=True)
    assert rm.cpu().tolist() == [-1, 0, -1] and info.cpu().tolist() == [1, 0]
    r, c = _lsa(np.zeros((0, 5)), dev)
    assert len(r) == 0 and len(c) == 0
    with pytest.raises(RuntimeError, match="at most"):
        ops.linear_sum_assignment(torch.zeros((4097, 4097), dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="at most"):
        ops.linear_sum_assignment(torch.zeros((2, 16385), dtype=torch.float64, device=dev))


def test_track_cost_is_bit_identical(dev, golden):
    from retinanet_mi355x import ops
    g = golden("tracker_assoc")
    for name, pre, det in tc.hungarian_cases():
        if not len(pre) or not len(det):
            continue
        got = ops.track_cost(torch.from_numpy(pre).to(dev), torch.from_numpy(det).to(dev)).cpu().numpy()
        want = g["hung_%s_dist" % name]
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), name


def test_match_hungarian_cpu_and_gpu(dev, golden):
    import mc3d_track
    g = golden("tracker_assoc")
    me = mc3d_track.TrackManager()
    me.phi_match = tc.PHI_MATCH
    for name, pre, det in tc.hungarian_cases():
        want = g["hung_%s_match" % name]
        is_list = bool(g["hung_%s_is_list" % name])
        cpu = me.match_hungarian(torch.from_numpy(pre), torch.from_numpy(det))
        gpu = me.match_hungarian(torch.from_numpy(pre).to(dev), torch.from_numpy(det).to(dev))
        if is_list:
            assert isinstance(cpu, list) and cpu == [], name
            assert len(gpu) == 0, name
            continue
        assert isinstance(cpu, np.ndarray) and np.array_equal(cpu.reshape(-1, 2), want), name
        assert isinstance(gpu, torch.Tensor) and gpu.is_cuda and gpu.dtype == torch.int64, name
        assert np.array_equal(gpu.cpu().numpy().reshape(-1, 2), want), name


def _tracker(dev):
    import mc3d_track
    from util_track.kf import Torch_KF

    class T(mc3d_track.TrackManager):
        pass
    t = T()
    for k, v in tc.PARAMS.items():
        setattr(t, k, v)
    t.class_dict = tc.class_dict()
    t.filter = Torch_KF(dev, INIT=tc.kf_init())
    t.fsld, t.all_classes, t.all_confs, t.all_cameras = {}, {}, {}, {}
    t.next_obj_id, t.updated_this_frame = 0, []
    t.ts_bias = list(tc.TS_BIAS)
    return t


def test_sequence_associate_and_prune(dev, golden):
    g = golden("tracker_assoc")
    t = _tracker(dev)
    log, phase = {}, ["none"]
    remove = t.filter.remove

    def logged_remove(ids):
        log[phase[0]] = sorted(int(i) for i in ids)
        remove(ids)
    t.filter.remove = logged_remove
    inc = t.increment_fslds

    def increment(*a):
        phase[0] = "fsld"
        return inc(*a)
    t.increment_fslds = increment
    worst = []
    for f, fr in enumerate(tc.sequence()):
        log.clear()
        t.timestamps = list(fr["timestamps"])
        det = torch.from_numpy(fr["detections"]).to(dev)
        pre_ids, matchings = t.associate(det, torch.from_numpy(fr["labels"]).to(dev), torch.from_numpy(fr["scores"]).to(dev),
                                         torch.from_numpy(fr["cameras"]).to(dev))
        phase[0] = "over"
        t.remove_overlaps()
        phase[0] = "anom"
        t.remove_anomalies(x_bounds=t.x_range)
        phase[0] = "none"
        k = "seq%d_" % f
        assert pre_ids == g[k + "pre_ids"].tolist(), f
        m = matchings.cpu().numpy() if isinstance(matchings, torch.Tensor) else np.asarray(matchings)
        assert np.array_equal(m.reshape(-1, 2), g[k + "match"]), f
        assert sorted(t.fsld.items()) == [tuple(r) for r in g[k + "fsld"].tolist()], f
        assert t.next_obj_id == int(g[k + "next_obj_id"]), f
        for ph in ("fsld", "over", "anom"):
            assert log.get(ph, []) == g[k + "rm_" + ph].tolist(), (f, ph)
        assert t.filter.view()[0] == g[k + "ids"].tolist(), f
        ck = sorted(t.all_classes)
        assert ck == g[k + "class_ids"].tolist() and np.array_equal(np.array([t.all_classes[c] for c in ck]), g[k + "classes"]), f
        errs = []
        for name, got in (("X", t.filter.X), ("P", t.filter.P)):
            want = g[k + name]
            e = float(np.abs(got.cpu().numpy() - want).max() / max(1.0, np.abs(want).max()))
            errs.append(e)
            assert e <= 1e-4, (f, name, e)
        assert np.array_equal(t.filter.T.cpu().numpy(), g[k + "T"]) or \
            np.abs(t.filter.T.cpu().numpy() - g[k + "T"]).max() <= 1e-9, f
        worst.append(max(errs))
    print("per-frame worst relative X/P error:", ["%.1e" % e for e in worst])


def test_linear_sum_assignment_custom_op(dev):
    from retinanet_mi355x import torch_ops
    cost = torch.from_numpy(tc.lsap_cases()[4][1]).to(dev)
    r, c = torch.ops.retinanet_mi355x.linear_sum_assignment(cost)
    want = tc.lsap_restated(cost.cpu().numpy())
    assert np.array_equal(r.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1])
    torch.library.opcheck(torch_ops.linear_sum_assignment, (cost,),
                          test_utils=("test_schema", "test_autograd_registration"))

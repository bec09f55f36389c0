"""CPU: the pieces of the track association that need no kernel -- the Python restatement of scipy's solver (the GPU
tests' fuzz oracle) against scipy, the new ops' refusal of CPU tensors, the custom op's registration, and the host
bookkeeping of mc3d_track (manage_tracks / increment_fslds) against the reference's 8-frame run."""
import numpy as np
import pytest
import torch

import track_cases as tc


def test_restatement_equals_scipy():
    sp = pytest.importorskip("scipy.optimize")
    for cost in tc.fuzz_matrices(600, seed=77) + [c for n, c in tc.lsap_cases() if c.size <= 2000]:
        a = sp.linear_sum_assignment(cost)
        b = tc.lsap_restated(cost)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for bad in (np.nan, -np.inf):
        x = np.ones((2, 3))
        x[0, 1] = bad
        with pytest.raises(ValueError, match="invalid numeric entries"):
            tc.lsap_restated(x)
    with pytest.raises(ValueError, match="infeasible"):
        tc.lsap_restated(np.array([[1.0, np.inf], [2.0, np.inf]]))


def test_restatement_equals_scipy_goldens(golden):
    g = golden("tracker_assoc")
    for name, cost in tc.lsap_cases():
        if cost.size > 2000:
            continue
        r, c = tc.lsap_restated(cost)
        assert np.array_equal(r, g["lsap_%s_row" % name]) and np.array_equal(c, g["lsap_%s_col" % name]), name


def test_new_ops_refuse_cpu_tensors():
    from retinanet_mi355x import ops
    with pytest.raises(RuntimeError):
        ops.linear_sum_assignment(torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.match(torch.zeros(3, 3, dtype=torch.float64), 0.9)
    with pytest.raises(RuntimeError):
        ops.track_cost(torch.zeros(3, 7), torch.zeros(2, 6))
    from retinanet_mi355x import torch_ops
    assert "linear_sum_assignment" in torch_ops.OPERATORS
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.retinanet_mi355x.linear_sum_assignment(torch.zeros(3, 3, dtype=torch.float64))


class _HostFilter:
    """Records what manage_tracks / increment_fslds hand to the filter (no kernel)."""
    def __init__(self):
        self.calls = []

    def update(self, det, ids):
        self.calls.append(("update", list(ids), np.asarray(det, dtype=np.float64).copy()))

    def add(self, det, ids, directions, times, init_speed=False, classes=None):
        self.calls.append(("add", list(ids), np.asarray(det, dtype=np.float64).copy(), np.asarray(directions).copy(),
                           np.asarray(times).copy(), init_speed, list(classes)))

    def remove(self, ids):
        self.calls.append(("remove", sorted(ids)))


def test_bookkeeping_against_the_sequence_golden(golden):
    """manage_tracks + the swapped increment_fslds on host tensors, fed the reference's matchings and pre_ids: the
    fsld dictionary, next_obj_id, all_classes and the fsld removals of every frame equal the reference's (the filter
    is a recorder: pruning needs the kernels and is left to the GPU test, so the ids the reference prunes are
    removed from the recorder's view by hand)."""
    import mc3d_track
    g = golden("tracker_assoc")
    t = mc3d_track.TrackManager()
    t.f_max = tc.PARAMS["f_max"]
    t.class_dict = tc.class_dict()
    t.filter = _HostFilter()
    t.fsld, t.all_classes, t.all_confs, t.all_cameras = {}, {}, {}, {}
    t.next_obj_id = 0
    for f, fr in enumerate(tc.sequence()):
        k = "seq%d_" % f
        t.updated_this_frame = []
        pre_ids = g[k + "pre_ids"].tolist()
        m = g[k + "match"]
        det = torch.from_numpy(fr["detections"])
        cams = fr["cameras"]
        times = [fr["timestamps"][c] + tc.TS_BIAS[c] for c in cams]
        t.manage_tracks(det, m, pre_ids, torch.from_numpy(fr["labels"]), torch.from_numpy(fr["scores"]),
                        torch.from_numpy(cams), times)
        updated = set(t.updated_this_frame)
        undetected = [i for i in pre_ids if i not in updated]
        removed = t.increment_fslds(pre_ids, undetected)
        assert removed == g[k + "rm_fsld"].tolist(), f
        assert sorted(t.fsld.items()) == [tuple(r) for r in g[k + "fsld"].tolist()], f
        assert t.next_obj_id == int(g[k + "next_obj_id"]), f
        ck = sorted(t.all_classes)
        assert ck == g[k + "class_ids"].tolist(), f
        assert np.array_equal(np.array([t.all_classes[c] for c in ck]), g[k + "classes"]), f
        assert all(isinstance(x, float) for c in t.all_confs.values() for x in c)
        assert all(isinstance(x, int) for c in t.all_cameras.values() for x in c)
        adds = [c for c in t.filter.calls if c[0] == "add"]
        if adds:
            assert adds[-1][5] is True and all(isinstance(n, str) for n in adds[-1][6])
        t.filter.calls.clear()

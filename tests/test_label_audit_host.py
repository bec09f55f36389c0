"""CPU: the label audit's host half (label_audit.py) and its oracle (tests/label_audit_cases.py).

The restatement equals the REFERENCE's own annotator bit for bit on the scripted scenes (tests/golden/label_audit.npz, written
by tools/make_golden_labels.py): every diff list, every ts_bias, what remove_outliers leaves, every interpolated datum in dict
order, and unbias_timestamps' data and all_ts.  The scenes hold the edges they claim, the packing refuses what it must, the
fuzz generator produces scenes that exercise every method, and the entry points are registered at every layer.  The kernels
themselves: tests/test_gpu_label_audit.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

import label_audit_cases as lc

SCENES = lc.golden_scenes()


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_equals_the_reference_bit_for_bit(golden, name):
    g = golden("label_audit")
    want = {k: g[k] for k in g.files if k.startswith(name + "_")}
    got = lc.restated(name, SCENES[name])
    assert sorted(got) == sorted(want) and len(got) == 20
    for k in sorted(got):
        assert bit_equal(got[k], want[k]), k


def test_golden_file_holds_outputs_of_every_scene_only(golden):
    g = golden("label_audit")
    assert sorted({k.split("_")[0] for k in g.files}) == sorted(SCENES)
    assert all(g[k].dtype.kind in "fi" for k in g.files)                        # arrays of numbers only


def test_audit_scene_holds_its_edges(golden):
    s = SCENES["audit"]
    tr = lc.tracklets(s["data"], s["names"])
    assert lc.unused_id(s["data"]) == 12 and any(i["id"] == 14 for fd in s["data"] for i in fd.values())
    lengths = {len(tr.get((c, o), [])) for c in (0, 1, 2) for o in range(12)}
    assert {0, 1, 2, 63, 64, 65, 130} <= lengths
    flags, values = lc.sample_block(s, 0, 2)                                    # key x, value timestamp; pair (1, 0) is index 0
    assert flags[0, 3].tolist() == [0] * 5                                      # 1 row against 10: no guard
    x4 = [r[1] for r in tr[(1, 4)]]
    assert any(sum((x4[i] - p) * (x4[i - 1] - p) <= 0 for i in range(1, len(x4))) > 1 for p in (101.0, 110.0, 120.0))   # zig-zag
    assert flags[0, 5].tolist() == [7] * 5 and values[0, 5, 0, 0] == 0.0 and values[0, 5, 0, 1] == 0.0   # an exact 0.0 time
    x5 = [r[1] for r in tr[(0, 5)]]
    assert sum((x5[i] - 2.0) * (x5[i - 1] - 2.0) == 0 for i in range(1, len(x5))) == 2   # a point on a row: two segments
    x6 = [r[1] for r in tr[(1, 6)]]
    assert x6[0] == x6[1]                                                       # K[i] == K[i-1]
    x7 = [r[1] for r in tr[(1, 7)]]
    assert min(x7) == max(x7) and flags[0, 7].tolist() == [7] * 5               # ran == 0
    assert max(r[1] for r in tr[(1, 8)]) < min(r[1] for r in tr[(0, 8)])        # hi < lo ...
    assert flags[0, 8].tolist() == [5, 1, 1, 1, 3]              # ... the guard passes; lo and hi are rows, nothing in between
    g = golden("label_audit")
    assert g["audit_ts_pairs"].tolist() == [[1, 0], [2, 1], [3, 1], [4, 3]]     # camera 3: decrement 2; camera 5: no partner
    assert g["audit_ts_bias"][5] == s["ts_bias"][5]                             # ... keeps its old value
    assert 0 < len(g["audit_ts_diffs"]) < 5 * 12 * 4                            # zeros and missing crossings were dropped
    assert g["audit_y_off"][1] == 5 * 8                                         # est_y_error keeps every point of a guarded object
    assert not bit_equal(g["audit_curve_y"], g["audit_proj_y"]) and bit_equal(g["audit_curve_x"], g["audit_proj_x"])
    fx, _ = lc.sample_block(s, 2, 0, 1)
    assert len(g["audit_proj_x"]) == 14 and fx[2, 5].tolist() == [7] * 5        # id 5 in (2, 1): one x of 0.0 was dropped
    assert len(SCENES["few"]["names"]) == 5 and lc.projection_partners(4, 2) == [3, 1]
    assert len(golden("label_audit")["few_proj_x"]) == 4 * 2 * 5                # pairs (2,1), (3,2), (4,3), (4,1)


def test_outlier_and_interpolation_scenes_hold_their_edges(golden):
    g = golden("label_audit")
    s = SCENES["outliers"]
    before, _ = lc.dump(s["data"], s["names"])
    left = {tuple(r[:3]) for r in g["outliers_outliers_idx"].tolist()}
    gone = {tuple(r[:3]) for r in before.tolist()} - left
    assert gone == {(9, 0, 0), (10, 0, 0),                     # the x jump at frame 10: 9 from ahead, 10 from ahead (9 is gone)
                    (5, 0, 1), (14, 0, 1),                      # y up: deleted from behind; y down: deleted from ahead
                    (0, 1, 2)}                                  # frame 0 against frame 29, the last
    assert (11, 0, 0) in left                                   # the chain: row 10 gone, so row 11 stays
    assert (26, 2, 1) in left and (27, 2, 1) in left            # past the empty frame 24 > last_frame: never visited
    assert lc.visited(s["data"], s["last_frame"]) == 24 and len(s["data"][24]) == 0
    s = SCENES["interp"]
    idx = g["interp_interp_idx"]
    new = idx[idx[:, 4] == 1]
    assert sorted(new[(new[:, 1] == 0) & (new[:, 2] == 0)][:, 0].tolist()) == [1] + list(range(4, 74))     # gaps of 1 and of 70
    assert sorted(new[(new[:, 1] == 1) & (new[:, 2] == 0)][:, 0].tolist()) == [6, 7, 8]                    # a second camera
    assert not len(new[new[:, 2] == 1]) and len(new[new[:, 2] == 4]) == 3 + 14                             # no gap; interpolate(4)
    ts = lc.ts_table(s["all_ts"], s["names"])
    assert len(set(np.round(np.diff(ts[:, 0]), 9).tolist())) > 50                                          # uneven all_ts


def test_packing_builds_the_tracklet_table_and_refuses_bad_entries():
    import label_audit as la
    s = SCENES["audit"]
    tab = la.pack_tracklets(s["data"], s["names"])
    tr = lc.tracklets(s["data"], s["names"])
    C = len(s["names"])
    assert tab["n_cam"] == C and tab["ids"] == list(range(12)) and tab["n_frames"] == 200
    assert tab["offsets"].dtype == np.int64 and tab["cols"].dtype == np.float64 and tab["frame"].dtype == np.int32
    assert len(tab["offsets"]) == 12 * C + 1 and tab["offsets"][-1] == len(tab["cols"]) == sum(len(v) for v in tr.values())
    for obj in range(12):
        for c in range(C):
            lo, hi = tab["offsets"][obj * C + c], tab["offsets"][obj * C + c + 1]
            rows = tr.get((c, obj), [])
            assert tab["frame"][lo:hi].tolist() == [r[0] for r in rows]
            assert tab["cols"][lo:hi].tolist() == [list(r[1:4]) for r in rows]
            assert tab["keys"][lo:hi] == [r[4] for r in rows]
    assert not any(k.endswith("_14") for k in tab["keys"])                      # above the first unused id
    one = la.pack_tracklets(s["data"], s["names"], [14])
    assert len(one["keys"]) == 24 and all(k.endswith("_14") for k in one["keys"])

    def broken(change):
        data = [dict((k, dict(v)) for k, v in fd.items()) for fd in s["data"][:40]]
        change(data)
        return data
    cases = {"key": lambda d: d[30].__setitem__("p1c1_7", d[30].pop("p1c1_3")),
             "camera": lambda d: d[30]["p1c2_3"].__setitem__("camera", "p9c9") or d[30].__setitem__("p9c9_3", d[30].pop("p1c2_3")),
             "finite": lambda d: d[31]["p1c2_3"].__setitem__("x", float("nan"))}
    for what, change in cases.items():
        with pytest.raises(ValueError) as e:
            la.pack_tracklets(broken(change), s["names"])
        assert "frame 3" in str(e.value) and ("p1c1_7" in str(e.value) or "p9c9_3" in str(e.value) or "p1c2_3" in str(e.value)), what


def test_host_only_helpers(capsys):
    import label_audit as la
    me = lc.Labels(SCENES["interp"])
    assert la.get_unused_id(me) == 3 == lc.unused_id(me.data)
    assert la.frames_visited(SCENES["outliers"]["data"], 20) == 24 and la.frames_visited(SCENES["outliers"]["data"], 24) == 30
    la.count_classes(me)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Class counts:" and "sedan:11" in out and "midsize:11" in out


def test_without_a_device_every_method_raises(monkeypatch):
    import label_audit as la
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Me(lc.Labels, la.LabelAudit):
        pass
    for call in (lambda m: m.estimate_ts_bias(), lambda m: m.est_y_error(), lambda m: m.estimate_projection_error(),
                 lambda m: m.remove_outliers(), lambda m: m.interpolate(0), lambda m: m.interpolate_all(),
                 lambda m: m.unbias_timestamps()):
        me = Me(SCENES["interp"])
        before = lc.dump(me.data, SCENES["interp"]["names"])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(me)
        assert bit_equal(before[0], lc.dump(me.data, SCENES["interp"]["names"])[0])


def test_fuzz_generator_exercises_every_method():
    """A condition on the inputs of tests/test_gpu_label_audit.py's fuzz comparison: of the 100 scenes at most 5 may end in the
    extinct-id RuntimeError, at least 60 must delete something and at least 80 must give every estimator a non-empty list."""
    extinct = deleting = full = 0
    for seed in range(100):
        scene = lc.fuzz_scene(seed)
        assert len(scene["names"]) <= 6 and len(scene["data"]) <= 200 and lc.unused_id(scene["data"]) <= 40
        try:
            deleting += len(lc.ref_outliers(lc.Labels(scene))) > 0
        except RuntimeError:
            extinct += 1
        pairs, _, _ = lc.ref_ts_bias(lc.Labels(scene))
        try:
            means = lc.ref_y_error(lc.Labels(scene))[2]
        except ValueError:
            means = []
        full += len(pairs) > 0 and len(means) > 0 and len(lc.ref_projection_error(lc.Labels(scene))[0]) > 0
    assert extinct <= 5 and deleting >= 60 and full >= 80, (extinct, deleting, full)


def test_entry_points_are_registered_at_every_layer():
    from retinanet_mi355x import _hip, ops, torch_ops
    for name in ("rn_label_pair_samples", "rn_label_outliers", "rn_label_interpolate", "rn_label_interpolate_workspace_bytes"):
        assert name in _hip.SIGNATURES
    for name in ("label_pair_samples", "label_outliers", "label_interpolate"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    assert _hip.load().rn_label_interpolate_workspace_bytes(10, 100) >= 100 * 4 + 10 * 4 + 11 * 8
    with pytest.raises(RuntimeError):
        ops.label_pair_samples(torch.zeros(3, dtype=torch.int64), torch.zeros((0, 3), dtype=torch.float64), 2, 0, 2)
    with pytest.raises(RuntimeError, match="status 3"):
        ops.label_check(3)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():                                      # shape inference without a device
        off = torch.empty(12 * 3 + 1, dtype=torch.int64, device="cuda")
        cols = torch.empty((50, 3), dtype=torch.float64, device="cuda")
        frame = torch.empty(50, dtype=torch.int32, device="cuda")
        fl, va, st = torch.ops.retinanet_mi355x.label_pair_samples(off, cols, 3, 0, 2, -1)
        assert tuple(fl.shape) == (3, 12, 5) and tuple(va.shape) == (3, 12, 5, 4) and fl.dtype == torch.uint8 and tuple(st.shape) == (1,)
        de, st = torch.ops.retinanet_mi355x.label_outliers(off, cols, frame, 30, 30)
        assert tuple(de.shape) == (50,) and de.dtype == torch.uint8
        got = torch.ops.retinanet_mi355x.label_interpolate(off, cols, frame, torch.empty((30, 3), dtype=torch.float64, device="cuda"), 7)
        assert [tuple(t.shape) for t in got] == [(7, 3), (7,), (7,), (1,), (1,)] and got[3].dtype == torch.int64

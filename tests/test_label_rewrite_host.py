"""CPU: the host half of the label re-basing (label_rewrite.py) and its oracle (tests/label_rewrite_cases.py).

The restatement against the REFERENCE's own annotator on the scripted scenes (tests/golden/label_rewrite.npz, written by
tools/make_golden_label_rewrite.py): every winning index of replace_homgraphy's search equal, the new x and y bit-equal, the
minimum errors within 1e-9 relative (the reference's matrix product is torch.matmul's), and every datum after replace_y (both
directions) and replace_timestamps bit-equal in dict order, all_ts included.  The scenes hold the edges they claim, every
refusal is raised with ``data`` untouched, and the entry points are registered at every layer.  The kernels themselves:
tests/test_gpu_label_rewrite.py."""
import contextlib
import copy
import io
import os
import pickle

import numpy as np
import pytest
import torch

import label_audit_cases as lc
import label_rewrite_cases as rc

SCENES = rc.golden_scenes()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def snapshot(me):
    return copy.deepcopy((me.data, me.all_ts))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_equals_the_reference(golden, name):
    g = golden("label_rewrite")
    want = {k: g[k] for k in g.files if k.startswith(name + "_")}
    got = rc.restated(name, SCENES[name])
    assert sorted(got) == sorted(want) and len(got) == (13 if name == "rebase" else 8)
    for k in sorted(got):
        if k.endswith("_rebase_err"):
            assert got[k].shape == want[k].shape and np.all(np.abs(got[k] - want[k]) <= 1e-9 * np.abs(want[k])), k
        else:
            assert bit_equal(got[k], want[k]), k


def test_golden_file_holds_outputs_of_every_scene_only(golden):
    g = golden("label_rewrite")
    assert sorted({k.split("_")[0] for k in g.files}) == sorted(SCENES)
    assert all(g[k].dtype.kind in "fi" for k in g.files)                        # arrays of numbers only
    assert not any(k.startswith("curve_rebase") or k.startswith("curve_hg") for k in g.files)


def test_linspace_and_radii_are_numpy_and_the_reference_s():
    rng = np.random.RandomState(3)
    for n in (2, 8, 11, 16):
        for c, r in zip(rng.uniform(-500, 500, 50), np.tile([50, 10.0, 2.0, 0.4, 1e-3], 10)):
            assert bit_equal(rc.linspace(c - r, c + r, n), np.linspace(c - r, c + r, n))
    from retinanet_mi355x import ops
    assert rc.radii() == ops.label_rebase_radii() == [50, 10.0, 2.0] and type(rc.radii()[1]) is float
    assert ops.label_rebase_radii(50, 0.1) == [50, 10.0, 2.0, 0.4]


def test_rebase_scene_holds_its_edges(golden):
    s, g = SCENES["rebase"], golden("label_rewrite")
    assert lc.unused_id(s["data"]) == 5 and any(i["id"] == 7 for fd in s["data"] for i in fd.values())
    assert rc.all_have_gen(s) and not rc.all_have_gen(SCENES["curve"])
    me = rc.Labels(s)
    boxes = [o for _, _, o in rc.visit(me, s["last_frame"] + 1) if o["gen"] == "Manual"]
    assert len(boxes) == len(g["rebase_rebase_win"]) == 87 and len(s["data"]) == 36 > s["last_frame"] + 1
    assert {o["direction"] for o in boxes} == {1, -1} and len({o["camera"] for o in boxes}) == 4
    win = g["rebase_rebase_win"]
    assert all(len(set(win[:, r].tolist())) > 3 for r in range(3)) and win.min() >= 0 and win.max() < 121      # every round moves
    hg = g["rebase_hg_idx"]
    assert hg[:, 0].max() == s["last_frame"] and 7 not in hg[:, 2] and (hg[:, 4] == 2).sum() == 87              # cut; id 7 gone
    assert (hg[:, 4] == 1).sum() > 87                                           # the rest was re-interpolated
    one = next(o for o in boxes if o["id"] == 1)                                # y = 55: the grid straddles the switch
    ys = rc.linspace(one["y"] - 50, one["y"] + 50, rc.GRID)
    corner = (ys - one["direction"] * one["w"] / 2.0).astype(np.float32)
    assert 0 < (corner > 60).sum() < rc.GRID
    old, new = s["hg_old"], s["hg_new"]
    assert all(not bit_equal(old[k][n], new[k][n]) for k in ("P1", "P2") for n in s["names"])
    assert all(not bit_equal(new["P1"][n], new["P2"][n]) for n in s["names"])
    c = SCENES["curve"]
    assert lc.visited(c["data"], c["last_frame"]) == 25 and g["curve_y0_idx"][:, 0].max() < 25 < len(c["data"])
    assert any("gen" not in i for fd in c["data"] for i in fd.values())
    assert not bit_equal(g["curve_y0_val"], g["curve_y1_val"]) and bit_equal(g["curve_y0_idx"], g["curve_y1_idx"])
    ts = g["curve_ts_table"]
    assert np.ptp(np.diff(ts[:, 1])) < 1e-9 and not bit_equal(ts, lc.ts_table(c["all_ts"], c["names"]))    # a nominal rate


def test_the_pass_over_data_visits_in_the_reference_s_order():
    import label_rewrite as lw
    for scene in list(SCENES.values()) + [rc.fuzz_scene(k) for k in range(4)]:
        me = rc.Labels(scene)
        me.data[3]["junk"] = {"id": 0}                          # keys of other shapes are passed over
        me.data[3]["p1c1_x"] = {"id": 0}
        me.data[3]["p1c1_007"] = {"id": 0}
        for n in (len(me.data), 7, 0):
            assert [(f, k) for f, k, _, _ in lw._visit(me, n)] == [(f, k) for f, k, _ in rc.visit(me, n)]


def test_offset_box_y_is_the_reference_s_on_the_host(golden):
    import label_rewrite as lw
    for name, scene in SCENES.items():
        me = rc.Labels(scene)
        got = [lw.offset_box_y(me, copy.deepcopy(o), reverse=rev)["y"] for rev in (False, True)
               for _, _, o in rc.visit(me, len(me.data))]
        assert bit_equal(np.array(got, np.float64), golden("label_rewrite")[name + "_box_y"])


def test_every_refusal_is_raised_and_leaves_data_untouched():
    import label_rewrite as lw
    scene = SCENES["rebase"]
    new = rc.build_hg(scene["hg_new"])
    first = next((f, k) for f, k, o in rc.visit(rc.Labels(scene), 36) if o["gen"] == "Manual" and f > 2)

    def gen_less(me):
        del me.data[first[0]][first[1]]["gen"]
        return new

    def camera_not_in_new(me):
        lost = rc.build_hg(scene["hg_new"])
        del lost.hg2.correspondence["p1c2"]
        return lost

    def camera_not_in_old(me):
        del me.hg.hg1.correspondence["p1c3"]
        return new

    def not_finite(what):
        def change(me):
            me.data[first[0]][first[1]][what] = float("inf")
            return new
        return change
    cases = [(gen_less, KeyError, "gen"), (camera_not_in_new, KeyError, "p1c2"), (camera_not_in_old, KeyError, "p1c3")]
    cases += [(not_finite(k), ValueError, "frame {}: key '{}'".format(*first)) for k in ("x", "y", "l", "w", "h")]
    for change, error, text in cases:
        me = rc.Labels(scene)
        hg_new = change(me)
        before, hg = snapshot(me), me.hg
        with pytest.raises(error) as e, contextlib.redirect_stdout(io.StringIO()):
            lw.replace_homgraphy(me, hg_new)
        assert text in str(e.value) and snapshot(me) == before and me.hg is hg, change.__name__
    for reverse in (False, True):                               # replace_y: a polynomial that is not there
        me = rc.Labels(SCENES["curve"])
        del me.poly_params["p1c2_WB"]
        before = snapshot(me)
        with pytest.raises(KeyError, match="p1c2_WB"):
            lw.replace_y(me, reverse)
        assert snapshot(me) == before
    with pytest.raises(KeyError, match="p1c2_WB"):
        lw.offset_box_y(me, {"camera": "p1c2", "direction": -1, "x": 1.0, "y": 2.0}, True)


def test_without_a_device_every_pass_raises_and_changes_nothing(monkeypatch):
    import label_rewrite as lw
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Me(rc.Labels, lw.LabelRewrite):
        pass
    scene = SCENES["rebase"]
    for call in (lambda m: m.replace_homgraphy(rc.build_hg(scene["hg_new"])), lambda m: m.replace_y(), lambda m: m.replace_y(True),
                 lambda m: m.replace_timestamps()):
        me = Me(scene)
        before, hg = snapshot(me), me.hg
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(me)
        assert snapshot(me) == before and me.hg is hg


def test_the_default_homography_comes_from_the_two_pickles(tmp_path, monkeypatch):
    import label_rewrite as lw
    from homography import Homography_Wrapper
    new = rc.build_hg(SCENES["rebase"]["hg_new"])
    for side, hg in (("EB", new.hg1), ("WB", new.hg2)):
        with open(tmp_path / "{}_homography5.cpkl".format(side), "wb") as f:
            pickle.dump(hg, f)
    monkeypatch.chdir(tmp_path)
    got = lw.load_homography()
    assert isinstance(got, Homography_Wrapper)
    assert bit_equal(got.hg1.correspondence["p1c2"]["P"], new.hg1.correspondence["p1c2"]["P"])
    assert bit_equal(got.hg2.correspondence["p1c4"]["P"], new.hg2.correspondence["p1c4"]["P"])
    monkeypatch.chdir(tmp_path.parent)
    with pytest.raises(FileNotFoundError):
        lw.replace_homgraphy(rc.Labels(SCENES["rebase"]))


def test_entry_points_are_registered_at_every_layer():
    import label_audit
    import label_rewrite as lw
    from retinanet_mi355x import _hip, ops, torch_ops
    header = open(os.path.join(REPO, "include", "retinanet_mi355x.h")).read()
    for name in ("rn_label_rebase", "rn_label_offset_y"):
        assert name in _hip.SIGNATURES and "int {}(".format(name) in header
    assert len(_hip.SIGNATURES["rn_label_rebase"][1]) == 16 and len(_hip.SIGNATURES["rn_label_offset_y"][1]) == 8
    for name, value in (("RN_LABEL_REBASE_MAX_GRID", ops.LABEL_REBASE_MAX_GRID), ("RN_LABEL_REBASE_MAX_ROUNDS", ops.LABEL_REBASE_MAX_ROUNDS),
                        ("RN_LABEL_BAD_CAMERA", ops.LABEL_BAD_CAMERA), ("RN_LABEL_BAD_ERROR", ops.LABEL_BAD_ERROR)):
        assert "#define {} {}".format(name, value) in header
    for name in ("label_rebase", "label_offset_y"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    assert lw.METHODS == ("replace_homgraphy", "replace_y", "offset_box_y", "replace_timestamps")
    assert all(getattr(lw.LabelRewrite, m) is getattr(lw, m) for m in lw.METHODS) and not set(lw.METHODS) & set(label_audit.METHODS)
    assert lw.interpolate_all is label_audit.interpolate_all and lw.get_unused_id is label_audit.get_unused_id
    with pytest.raises(RuntimeError, match="status 24"):
        ops.label_check(24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_offset_y(torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1, 3), dtype=torch.float64),
                           torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():                                      # shape inference without a device
        e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")
        P = e((4, 3, 4), torch.float64)
        got = torch.ops.retinanet_mi355x.label_rebase(e((9, 6), torch.float64), e((9,), torch.int32), P, None, P, P,
                                                      e((3,), torch.float64), 11)
        assert [tuple(t.shape) for t in got] == [(9, 2), (9,), (9, 3), (1,)]
        assert [t.dtype for t in got] == [torch.float64, torch.float64, torch.int32, torch.int32]
        y = torch.ops.retinanet_mi355x.label_offset_y(e((9, 2), torch.float64), e((9, 3), torch.float64), e((9,), torch.float64),
                                                      e((9,), torch.int32), True)
        assert tuple(y.shape) == (9,) and y.dtype == torch.float64

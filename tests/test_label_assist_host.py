"""CPU: the host half of the detector-assisted labelling (label_assist.py) and its oracle (tests/label_assist_cases.py).

The restatement against the REFERENCE's own annotator on the scripted scene (tests/golden/label_assist.npz, written by
tools/make_golden_label_assist.py, which found the errors of all 7 260 candidates bit-equal): every winning index of
paste_in_2D_bbox's search, every round's minimum error, every centre, box_to_state, find_box, automate's two rectangles and
every datum written by paste_in_2D_bbox, copy_paste and automate bit-equal, key for key and type for type.  The scene holds
the edges it claims.  The restated linspace, best-anchor rule and crop window against torch on the CPU, ties and NaN included.
Every refusal of the Python surface that can be raised without a device.  The kernels themselves: tests/test_gpu_label_assist.py."""
import copy
import os

import numpy as np
import pytest
import torch

import label_assist_cases as ac

SCENES = ac.golden_scenes()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def restated():
    return {name: ac.restated(name, scene) for name, scene in SCENES.items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_equals_the_reference(golden, restated, name):
    g = golden("label_assist")
    want = {k: g[k] for k in g.files if k.startswith(name + "_")}
    got = restated[name]
    assert sorted(got) == sorted(want) and len(got) == 9
    for k in sorted(got):                                       # the tool found every candidate's error bit-equal: so is all else
        assert bit_equal(got[k], want[k]), k
    assert want[name + "_data_idx"][:, 5:].all()                # every written x and y is a Python float
    assert want[name + "_win"].shape == (16, 3) and want[name + "_err"].dtype == np.float32


def test_golden_file_holds_outputs_only(golden):
    g = golden("label_assist")
    assert sorted({k.split("_")[0] for k in g.files}) == sorted(SCENES)
    assert all(g[k].dtype.kind in "fi" for k in g.files)                        # arrays of numbers only


def test_the_scene_holds_the_edges_it_claims(golden, restated):
    scene, got = SCENES["assist"], restated["assist"]
    steps = ac.golden_script(scene)
    pastes = [s[1] for s in steps if s[0] == "paste2d"]
    assert {p.dtype for p in pastes} == {np.dtype(np.int64), np.dtype(np.float32)}              # a drawn box, a detected box
    assert any(p[0] > 1920 for p in pastes) and any(p[0] <= 1920 for p in pastes)               # both views
    data = scene["data"][scene["frame_idx"]]
    used = {(s[2], s[1]) for s in steps if s[0] == "view"}
    assert {d["direction"] for d in data.values()} == {1, -1} and len(used) > 4
    # the search of id 4 ends within one last radius (2 ft) of the wrapper switch: corner-0 y = y - w / 2 against 60
    centre = got["assist_centre"]
    near = [c for c in centre if abs((c[1] - 3.0) - 60.0) < 2.0]
    assert len(near) >= 2 and len(pastes) == len(centre) == 16
    # automate: each of the four edge tests fails once, alone
    box, skip = got["assist_auto_box"], got["assist_auto_skip"]
    fails = [(b[0] < 0, b[1] < 0, b[2] > 1920, b[3] > 1080) for b, s in zip(box, skip) if s]
    assert [f for f in fails if sum(f) == 1 and f[0]] and [f for f in fails if sum(f) == 1 and f[1]]
    assert [f for f in fails if sum(f) == 1 and f[2]] and [f for f in fails if sum(f) == 1 and f[3]]
    assert (skip == 0).sum() >= 3 and any(b[0] > 1920 for b, s in zip(box, skip) if not s)     # and the shifted second view
    assert all(np.isnan(b[4:]).all() for b, s in zip(box, skip) if s)


def test_every_round_s_winner_is_clear_of_the_runner_up():
    """The tool's fixture condition again, on the restatement (bit-equal to the reference's errors): no round is a near tie."""
    scene = SCENES["assist"]
    me = ac.Labels(scene)
    seen = []

    def paste2d(m, box):
        got = ac.ref_paste_in_2D_bbox(m, box)
        seen.append(got)
        return got
    ac.replay(me, [s for s in ac.golden_script(scene) if s[0] != "automate"], dict(ac.RESTATED, paste2d=paste2d))
    assert len(seen) == 16
    for rounds in seen:
        for e, i in rounds:
            e1, e2 = np.sort(e)[:2]
            assert int(np.argmin(e)) == i and e2 > e1


def test_linspace_is_numpy_s_on_float32_torch_scalars():
    rng = np.random.RandomState(3)
    for n in (2, 8, 11, 16):
        for c, r in zip(rng.uniform(-500, 500, 40).astype(F32), np.tile([50, 10.0, 2.0, 0.4], 10)):
            t = torch.tensor(c)
            want = np.linspace(t - r, t + r, n)
            assert isinstance(want, torch.Tensor) and want.dtype == torch.float32
            assert bit_equal(ac.linspace32(F32(c) - F32(r), F32(c) + F32(r), n), want.numpy())


def torch_best_anchor(cls, reg, win, cs):
    """crop_detect's lines on CPU tensors: torch.max over the classes, torch.argmax over the anchors, the move to the frame."""
    out = []
    for b in range(len(cls)):
        confs, classes = torch.max(torch.from_numpy(cls[b:b + 1]), dim=2)
        max_idx = torch.argmax(confs.squeeze(0))
        box = torch.from_numpy(reg[b].copy())[max_idx]
        box = box * torch.tensor(win[b, 2]) / cs
        box[[0, 2]] += torch.tensor(win[b, 0])
        box[[1, 3]] += torch.tensor(win[b, 1])
        out.append((box.numpy(), int(max_idx), confs[0, max_idx].numpy(), int(classes[0, max_idx])))
    return out


@pytest.mark.parametrize("name", sorted(ac.anchor_edge_cases()))
def test_best_anchor_restatement_is_torch_s(name):
    cls, reg, win = ac.anchor_edge_cases()[name]
    box, anchor, conf, klass = ac.best_anchor(cls, reg, win, 112)
    for b, (tb, ta, tc, tk) in enumerate(torch_best_anchor(cls, reg, win, 112)):
        assert (anchor[b], klass[b]) == (ta, tk), (name, b)
        assert bit_equal(box[b], tb) and bit_equal(conf[b], tc.astype(F32).reshape(())), (name, b)
    if name == "edges":
        assert anchor.tolist() == [129, 5, 0, 77, 9] and klass.tolist()[1:] == [2, 0, 4, 2]


def test_crop_window_restatement_is_torch_s():
    """crop_detect :707-717 on float32 tensors, as automate hands them over."""
    rng = np.random.RandomState(11)
    names = ac.lc.camera_names(2)
    spec = ac.rc.hg_spec(names)
    P1, P2 = (np.stack([spec[k][n].reshape(12) for n in names]) for k in ("P1", "P2"))
    state = np.stack([rng.uniform(20, 60, 40), rng.uniform(5, 110, 40), rng.uniform(12, 50, 40), rng.uniform(5, 8, 40),
                      rng.uniform(4, 12, 40), rng.choice([-1.0, 1.0], 40)], axis=1).astype(F32)
    crop, rois, win, skipped, status = ac.crop_windows(state, np.arange(40) % 2, P1, P2)
    assert status == 0 and 0 < skipped.sum() < 40
    for b in np.nonzero(skipped == 0)[0]:
        c = torch.from_numpy(crop[b].copy())
        w, h = c[2] - c[0], c[3] - c[1]
        scale = max(w, h) * 1.2
        minx, maxx = (c[2] + c[0]) / 2.0 - scale / 2.0, (c[2] + c[0]) / 2.0 + scale / 2.0
        miny, maxy = (c[3] + c[1]) / 2.0 - scale / 2.0, (c[3] + c[1]) / 2.0 + scale / 2.0
        want = torch.tensor([b % 2, minx, miny, maxx, maxy]).float()
        assert bit_equal(rois[b], want.numpy()) and bit_equal(win[b], torch.stack([minx, miny, scale]).numpy())


def test_refusals_without_a_device(monkeypatch):
    import label_assist as la
    from retinanet_mi355x import ops
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_fit_box2d(z((1, 4), dtype=f32), z(1, dtype=i32), z((1, 2), dtype=f32), z((1, 4), dtype=f32), z((1, 3, 4), dtype=f64),
                            None, z(3, dtype=f64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_best_anchor(z((1, 2, 3), dtype=f32), z((1, 2, 4), dtype=f32), z((1, 3), dtype=f32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_crop_windows(z((1, 6), dtype=f32), z(1, dtype=i32), z((1, 3, 4), dtype=f64), None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Me(ac.Labels, la.LabelAssist):
        pass
    scene = SCENES["assist"]
    me = Me(scene)
    me.active_cam, me.clicked_camera = 1, scene["names"][1]
    key = "{}_{}".format(scene["names"][1], 0)
    me.copied_box = (0, me.data[1][key].copy(), [F32(0), F32(0)])
    before = copy.deepcopy(me.data)
    point = np.array([900, 300, 940, 330], np.int64)
    for call in (lambda: me.box_to_state(point), lambda: me.find_box(point), lambda: me.copy_paste(point),
                 lambda: me.paste_in_2D_bbox(point.copy()), lambda: me.automate(0),
                 lambda: me.crop_detect(np.zeros((8, 8, 3), np.uint8), np.array([1, 1, 5, 5], F32)),
                 lambda: me.automate_many([key], {scene["names"][1]: np.zeros((8, 8, 3), np.uint8)})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
        assert me.data == before
    with pytest.raises(KeyError):
        me.automate_many(["p9c9_0"], {})
    assert me.automate(99) is None and me.data == before


def test_entry_points_are_registered_at_every_layer():
    import label_assist as la
    from retinanet_mi355x import _hip, ops, torch_ops
    header = open(os.path.join(REPO, "include", "retinanet_mi355x.h")).read()
    for name, n_args in (("rn_label_fit_box2d", 17), ("rn_label_best_anchor", 12), ("rn_label_crop_windows", 15)):
        assert name in _hip.SIGNATURES and "int {}(".format(name) in header and len(_hip.SIGNATURES[name][1]) == n_args
    for name in ("label_fit_box2d", "label_best_anchor", "label_crop_windows"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    assert all(getattr(la.LabelAssist, m) is getattr(la, m) for m in la.METHODS) and len(la.METHODS) == 7
    assert ops.label_rebase_radii(la.SEARCH_RAD) == ac.radii() == [50, 10.0, 2.0] and la.GRID_SIZE == ac.GRID
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():                                      # shape inference without a device
        e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")
        P = e((4, 3, 4), torch.float64)
        got = torch.ops.retinanet_mi355x.label_fit_box2d(e((9, 4), torch.float32), e((9,), torch.int32), e((9, 2), torch.float32),
                                                         e((9, 4), torch.float32), P, None, e((3,), torch.float64), 11, None)
        assert [tuple(t.shape) for t in got] == [(9, 2), (9,), (9, 3), (1,)]
        assert [t.dtype for t in got] == [torch.float32, torch.float32, torch.int32, torch.int32]
        got = torch.ops.retinanet_mi355x.label_best_anchor(e((5, 70, 8), torch.float32), e((5, 70, 4), torch.float32),
                                                           e((5, 3), torch.float32), 112.0)
        assert [tuple(t.shape) for t in got] == [(5, 4), (5,), (5,), (5,)]
        assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.float32, torch.int32]
        got = torch.ops.retinanet_mi355x.label_crop_windows(e((7, 6), torch.float32), e((7,), torch.int32), P, P, 1.2, 1920.0, 1080.0)
        assert [tuple(t.shape) for t in got] == [(7, 4), (7, 5), (7, 3), (7,), (1,)]
        assert [t.dtype for t in got] == [torch.float32] * 3 + [torch.uint8, torch.int32]


def test_the_end_to_end_scene_restates_to_sane_labels():
    scene = ac.small_scene()
    me = ac.Labels(scene)
    before = copy.deepcopy(me.data[0])
    got = ac.ref_automate_keys(me, scene, scene["keys"])
    skipped = [k for k in got if got[k]["skipped"]]
    assert skipped == ["p1c1_4"] and len(got) == 13 and me.data[0]["p1c1_4"] == before["p1c1_4"]
    for key, res in got.items():
        if not res["skipped"]:
            new, old = me.data[0][key], before[key]
            assert new["gen"] == "Manual" and type(new["x"]) is float and type(new["y"]) is float
            assert 0 < abs(new["x"] - old["x"]) + abs(new["y"] - old["y"]) < 8.0        # moved, by the detector's little
            assert 0 <= res["crop_box"][0] and res["crop_box"][2] <= 96 and 0 <= res["crop_box"][1] and res["crop_box"][3] <= 64

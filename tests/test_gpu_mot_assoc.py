"""GPU: identity and association scores on the device (csrc/mot_assoc.hip: rn_mot_id_counts / id_assign / hota_align /
hota_assign / hota_reduce; ops.mot_id_* / mot_hota_*; mot_evaluator.evaluate_association, MOT_Evaluator(params={"association":
True})) against the restatement in tests/mot_assoc_cases.py, stage by stage through each stage's own op:

  gc, pc, C exact; IDTP exact and the matching scipy's on the same C; pot bit for bit; every frame's matched pairs and prefix
  lengths exact; TP / FN / FP exact; Loc and the association sums bit for bit (the restatement uses the kernel's order).

The IoU matrices are injected through ``ious=``.  End to end: evaluate_association on every scene, and MOT_Evaluator on a small
CSV pair with the device's own IoUs.  Two runs give the same bits; the torch operators give the same tensors as ops.*; the
refusals raise; the closed-form scenes give their hand-derived answers."""
import contextlib
import csv
import io
import os

import numpy as np
import pytest
import torch

import mot_assoc_cases as ac
import mot_cases as mc

pytestmark = pytest.mark.gpu

CLOSED = ac.closed_form_scenes()
EDGE = ac.edge_scenes()
SCENES = dict({k: v for k, v in EDGE.items()}, **{k: (v[0], 0.5) for k, v in CLOSED.items()})


def _hg(dev):
    import homography
    hg = homography.Homography(device=str(dev))
    hg.correspondence = {"cam": {"H": np.asarray(mc.SYN_H, np.float64), "P": np.asarray(mc.SYN_P, np.float64)}}
    hg.default_correspondence = "cam"
    return hg


@pytest.fixture(scope="module")
def want():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ac.restated(*SCENES[name])
        return cache[name]
    return get


def _packed(scene):
    gids, gmap = ac.dense_ids(scene["gt_ids"])
    pids, pmap = ac.dense_ids(scene["pred_ids"])
    flat = [np.asarray(m, np.float64).reshape(-1) for m in scene["ious"] if m is not None]
    return dict(n_gt=[len(g) for g in gids], n_pred=[len(p) for p in pids], gt_id=np.concatenate(gids).astype(np.int32),
                pred_id=np.concatenate(pids).astype(np.int32), n_gid=len(gmap), n_pid=len(pmap),
                ious=np.concatenate(flat) if flat else np.zeros(0))


def _stages(scene, id_iou, dev, t=None):
    """Every stage through its own op (t: the torch.ops namespace instead of ops) -> numpy arrays."""
    from retinanet_mi355x import ops
    pk = _packed(scene)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    gt_id, pred_id, iou, alphas = up(pk["gt_id"]), up(pk["pred_id"]), up(pk["ious"]), up(ops.mot_alphas())
    csr = tuple(up(a) for a in ops.mot_id_csr(pk["n_gt"], pk["n_pred"], pk["gt_id"], pk["n_gid"]))
    if t is None:
        offsets, totals = ops.mot_offsets(pk["n_gt"], pk["n_pred"], dev)
        gc, pc, C, st = ops.mot_id_counts(iou, offsets, totals, gt_id, pred_id, pk["n_gid"], pk["n_pid"], id_iou)
        match, info = ops.mot_id_assign(C)
        pot, st2 = ops.mot_hota_align(iou, offsets, totals, gt_id, pred_id, csr, pk["n_gid"], pk["n_pid"])
        assigned = ops.mot_hota_assign(iou, offsets, totals, gt_id, pred_id, gc, pc, pot, alphas)
        result = ops.mot_hota_reduce(offsets, totals, assigned, gt_id, pred_id, gc, pc)
    else:
        n_gt, n_pred = pk["n_gt"], pk["n_pred"]
        gc, pc, C, st = t.mot_id_counts(iou, n_gt, n_pred, gt_id, pred_id, pk["n_gid"], pk["n_pid"], float(id_iou))
        match, info = t.mot_id_assign(C)
        pot, st2 = t.mot_hota_align(iou, n_gt, n_pred, gt_id, pred_id, *csr, pk["n_gid"], pk["n_pid"])
        assigned = t.mot_hota_assign(iou, n_gt, n_pred, gt_id, pred_id, gc, pc, pot, alphas)
        result = t.mot_hota_reduce(n_gt, n_pred, *assigned, gt_id, pred_id, gc, pc)
    names = ("gc", "pc", "C", "st_counts", "match", "info", "pot", "st_align", "slot_row", "slot_col", "slot_s", "slot_n",
             "frame_status", "result")
    return {k: v.cpu().numpy() for k, v in zip(names, (gc, pc, C, st, match, info, pot, st2) + tuple(assigned) + (result,))}


def _check_stages(got, w):
    assert list(got["st_counts"]) == [0, -1] and list(got["st_align"]) == [0, -1] and not got["frame_status"].any()
    assert np.array_equal(got["gc"], w["gc"]) and np.array_equal(got["pc"], w["pc"]) and np.array_equal(got["C"], w["C"])
    assert int(got["info"][0]) == w["IDTP"] and int(got["info"][1]) == 0
    match = np.full(len(w["gc"]), -1, np.int64)
    match[w["id_rows"]] = w["id_cols"]
    assert np.array_equal(got["match"], match)                           # scipy's matching on the same C
    assert got["pot"].tobytes() == w["pot"].tobytes()
    slots = w["slots"]
    assert np.array_equal(got["slot_row"], [s[1] for s in slots]) and np.array_equal(got["slot_col"], [s[2] for s in slots])
    assert np.array_equal(got["slot_n"], [s[4] for s in slots])
    assert got["slot_s"].tobytes() == np.array([s[3] for s in slots], np.float64).tobytes()
    blk = got["result"][:19 * 7].reshape(19, 7)
    for k, key in enumerate(("TP", "FN", "FP")):
        assert np.array_equal(blk[:, k], w[key]), key
    for k, key in enumerate(("loc", "a_sum", "re_sum", "pr_sum")):
        assert blk[:, 3 + k].tobytes() == np.asarray(w[key], np.float64).tobytes(), key
    assert got["result"][133] == 0


def _check_dict(m, w):
    import mot_evaluator as me
    assert list(m) == list(me.ASSOC_SCALARS) + ["alphas", "per_alpha"]
    for key in me.ASSOC_SCALARS:
        assert m[key] == w[key], (key, m[key], w[key])                   # the same sums through the same formulas
    assert m["alphas"].tobytes() == ac.ALPHAS.tobytes()
    for key in ac.FIGURES:
        assert m["per_alpha"][key].tobytes() == w["per_alpha"][key].tobytes(), key
    for key in ("TP", "FN", "FP"):
        assert np.array_equal(m["per_alpha"][key], w[key])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_stages_against_the_restatement(dev, want, name):
    scene, id_iou = SCENES[name]
    _check_stages(_stages(scene, id_iou, dev), want(name))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_evaluate_association_end_to_end(dev, want, name):
    import mot_evaluator as me
    scene, id_iou = SCENES[name]
    gt, pred, flat = ac.scene_rows(scene)
    m, out = me.evaluate_association(gt, pred, _hg(dev), id_iou=id_iou, collect=True, ious=torch.from_numpy(flat).to(dev))
    w = want(name)
    _check_dict(m, w)
    assert out["pot"].tobytes() == w["pot"].tobytes() and np.array_equal(out["C"], w["C"])
    if name in CLOSED:                                                   # ... and the hand-derived answers themselves
        for key, v in CLOSED[name][1].items():
            assert m[key] == v if isinstance(v, int) or (v * 2.0 ** 20) % 1 == 0 else abs(m[key] - v) <= np.spacing(v), (key, m[key], v)


def test_two_runs_and_the_torch_operators(dev, want):
    from retinanet_mi355x import torch_ops  # noqa: F401  (registers torch.ops.retinanet_mi355x.mot_*)
    for name in ("ids_tall", "wide70"):
        scene, id_iou = SCENES[name]
        a, b = _stages(scene, id_iou, dev), _stages(scene, id_iou, dev)
        c = _stages(scene, id_iou, dev, t=torch.ops.retinanet_mi355x)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key
            assert a[key].tobytes() == c[key].tobytes() and a[key].dtype == c[key].dtype and a[key].shape == c[key].shape, key


def _csv_pair(tmp_path):
    """12 frames of up to three vehicles: a prediction id that changes, an id absent for a stretch, a frame only in the ground
    truth and one only in the predictions."""
    gt, pred = {}, {}
    for f in range(12):
        for k in range(3):
            if k == 2 and 4 <= f < 7:
                continue
            g, p = mc._veh(f, k, 10 + k + (5 if (k == 0 and f >= 6) else 0), 64.0 * k, 8.0, dx=0.5 * ((f + k) % 4), dy=0.25 * (f % 3))
            if f != 9:
                gt.setdefault(f, []).append(g)
            if f != 3:
                pred.setdefault(f, []).append(p)
    paths = []
    for name, rows in (("gt", gt), ("pred", pred)):
        paths.append(os.path.join(str(tmp_path), name + ".csv"))
        with open(paths[-1], "w", newline="") as fh:
            wr = csv.writer(fh)
            wr.writerow(["Frame #"] + ["c%d" % i for i in range(1, 45)])
            for f in sorted(rows):
                wr.writerows(rows[f])
    return gt, pred, paths


def test_mot_evaluator_with_association(dev, tmp_path):
    import mot_evaluator as me
    gt, pred, (gpath, ppath) = _csv_pair(tmp_path)
    ref = mc.restated(gt, pred, mc.SYN_H, mc.SYN_P, 0, 10000)
    frames = sorted(set(gt) | set(pred))
    scene = dict(gt_ids=[[int(r[2]) for r in gt.get(f, ())] for f in frames], pred_ids=[[int(r[2]) for r in pred.get(f, ())] for f in frames],
                 ious=[ref["ious"].get(f) for f in frames])
    w = ac.restated(scene, 0.5)
    assert w["IDFN"] > 0 and w["IDFP"] > 0 and 0 < w["AssA"] < 1         # the pair exercises something
    hg = _hg(dev)
    text_off, text_on = io.StringIO(), io.StringIO()
    plain = me.MOT_Evaluator(gpath, ppath, hg, {"match_iou": 0})
    with contextlib.redirect_stdout(text_off):
        plain.evaluate()
    ev = me.MOT_Evaluator(gpath, ppath, hg, {"match_iou": 0, "association": True, "id_iou": 0.5})
    with contextlib.redirect_stdout(text_on):
        ev.evaluate()
    assert list(ev.metrics) == list(plain.metrics) + list(me.ASSOC_SCALARS)
    assert not set(plain.metrics) & set(me.ASSOC_SCALARS)
    for key in me.ASSOC_SCALARS:
        assert ev.metrics[key] == w[key], key
    for key in plain.metrics:
        a, b = plain.metrics[key], ev.metrics[key]
        assert (a == b) if not isinstance(a, tuple) else (float(a[0]) == float(b[0]) and float(a[1]) == float(b[1])), key
    on = text_on.getvalue().split("\n")
    assert [ln for ln in on if ln.split(":")[0].strip() not in me.ASSOC_SCALARS] == text_off.getvalue().split("\n")
    assert "{:<30}: {:.3f}".format("HOTA", w["HOTA"]) in on and "{:<30}: {:.3f}".format("IDF1", w["IDF1"]) in on
    only = me.MOT_Evaluator(gpath, ppath, hg).evaluate_association()
    _check_dict(only, w)


def test_refusals(dev):
    import mot_evaluator as me
    from retinanet_mi355x import _hip, ops
    hg = _hg(dev)
    gt, pred, flat = ac.scene_rows(ac.duplicate_scene())
    with pytest.raises(ValueError, match="twice"):
        me.evaluate_association(gt, pred, hg, ious=torch.from_numpy(flat).to(dev))
    gt, pred, flat = ac.scene_rows(ac.nan_scene())
    with pytest.raises(ValueError, match="invalid numeric entries"):
        me.evaluate_association(gt, pred, hg, ious=torch.from_numpy(flat).to(dev))
    with pytest.raises(RuntimeError, match="MOT_MAX"):
        me.evaluate_association(*mc.too_large_case(), hg)
    lib, z = _hip.load(), torch.zeros(8, dtype=torch.int64, device=dev)
    p = z.data_ptr()
    # the C entries refuse a frame above RN_MOT_MAX and ids above the storage cap with an error code: nothing is launched
    assert lib.rn_mot_hota_assign(p, p, p, p, p, 1, ops.MOT_MAX + 1, 1, 1, 1, 1, p, p, 1, 1, p, p, p, p, p, p, p, p, p, p,
                                  _hip.stream()) == 10001
    assert lib.rn_mot_id_counts(p, p, p, p, p, 1, ops.MOT_MAX + 1, 1, 1, 1, 1, p, p, 1, 1, 0.5, p, p, p, p, _hip.stream()) == 10001
    assert lib.rn_mot_assoc_workspace_bytes(2048, 1024) == 0 and lib.rn_mot_assoc_workspace_bytes(1024, 1024) > 0
    assert lib.rn_mot_id_assign(p, 2048, 1024, p, p, p, _hip.stream()) == 10001
    assert lib.rn_mot_hota_reduce(p, p, p, p, 1, 1, 1, 1, 1, 1, p, p, p, p, p, p, p, p, p, 2048, 1024, p, p, _hip.stream()) == 10001
    torch.cuda.synchronize()
    assert not z.any()
    with pytest.raises(RuntimeError, match="2048 ground-truth ids x 1024 predicted ids"):
        ops.mot_id_assign(torch.zeros((2048, 1024), dtype=torch.int32, device=dev))
    pk = dict(n_gt=[1], n_pred=[1], gid=dict.fromkeys(range(2048)), pid=dict.fromkeys(range(1024)))
    with pytest.raises(RuntimeError, match="cells"):
        me.run_association(pk, hg, 0.5, dev)

"""GPU: tracking evaluation on the device (csrc/mot_eval.hip: rn_mot_prepare / iou / assign / frame_metrics / reduce;
ops.mot_*; mot_evaluator.MOT_Evaluator / evaluate_tracks) against the restatement in tests/mot_cases.py and the reference's
own results in tests/golden/mot_eval.npz.

Synthetic cases (identity-like homography, dyadic coordinates: no transform rounds): everything exact -- IoU matrices,
assignment slots, matches, error vectors, counters, ids, confusion, and the fp64 sums of every figure bit for bit.
Staged: the golden IoU matrices fed to kernels 3-5: assignments, matches, counters, id metrics and confusion exact.
End to end on the stable first frames of the cut reference files: eps = the largest |IoU_device - IoU_reference| is
measured and printed (run with -s; profiles/mot_eval_gpu_tests.log keeps one run); frames that mot_cases.stable_frame calls
stable at 16 eps are compared exactly and at most 5 % may be unstable; the figures hold to 4 x
test_mot_eval_host.FIRST_FIGURE_DEV; the printed table and the per-match lists of ``self.m`` equal the reference's.  Two
evaluations give the same bits."""
import contextlib
import io

import numpy as np
import pytest
import torch

import mot_cases as mc
from test_mot_eval_host import CASES, FIRST_FIGURE_DEV, FIRST_CASES, case_of, golden_ious, rows_of

pytestmark = pytest.mark.gpu

RESULT_Q = ["pre", "match", 0, 1, 2, 3, 4, 5, 6, "bot", "top"]            # figure order of the result block


def _hg(H, P, dev):
    import homography
    hg = homography.Homography(device=str(dev))
    hg.correspondence = {"cam": {"H": np.asarray(H, np.float64), "P": np.asarray(P, np.float64)}}
    hg.default_correspondence = "cam"
    return hg


def _pairs(out):
    """The device's slots in the restatement's form: (frame, gt row, pred column, IoU, matched) per assigned pair."""
    pk = out["packed"]
    frame = np.repeat(np.asarray(pk["frames"], np.int64), np.minimum(pk["n_gt"], pk["n_pred"]))
    return dict(pair_frame=frame, pair_gt=out["slot_row"].astype(np.int64), pair_pred=out["slot_col"].astype(np.int64),
                pair_iou=out["slot_iou"], pair_ok=out["slot_gid"] >= 0)


def _device_ious(out):
    pk, res, o = out["packed"], {}, 0
    for f, n, m in zip(pk["frames"], pk["n_gt"], pk["n_pred"]):
        if n and m:
            res[f] = out["iou"][o:o + n * m].reshape(n, m)
        o += n * m
    return res


INT_METRICS = ("True unique objects", "Predicted unique objects", "TP", "FP", "FN", "FP edge-case", "FP @ 0.2", "FN @ 0.2",
               "Fragmentations", "ID switches", "Recall", "Precision", "False Alarm Rate", "MOTA", "MOTA edge-case", "MOTA @ 0.2")


def _check_exact(metrics, confusion, out, want):
    for k in INT_METRICS:
        assert metrics[k] == want["metrics"][k], k
    assert np.array_equal(confusion, want["confusion"])
    got = _pairs(out)
    for k in ("pair_frame", "pair_gt", "pair_pred", "pair_ok"):
        assert np.array_equal(got[k], want[k]), k
    assert got["pair_iou"].tobytes() == want["pair_iou"].tobytes()
    ok = got["pair_ok"]
    assert out["state_err"][ok].tobytes() == want["state_err"].tobytes()
    assert out["bot"][ok].tobytes() == want["bot_err"].tobytes() and out["top"][ok].tobytes() == want["top_err"].tobytes()


def _check_sums(out):
    """The result block's sums against fixed_sums of the DEVICE's own per-slot vectors: the same inputs, so bit for bit."""
    res, ok = out["result"], out["slot_gid"] >= 0
    vec = {"pre": (out["slot_iou"], out["slot_row"] >= 0), "match": (out["slot_iou"], ok), "bot": (out["bot"], ok),
           "top": (out["top"], ok)}
    for c in range(7):
        vec[c] = (out["state_err"][:, c], ok)
    for q, key in enumerate(RESULT_Q):
        n, s1, s2 = mc.fixed_sums(*vec[key])
        got = res[16 + 3 * q:19 + 3 * q]
        assert got[0] == n and np.float64(s1).tobytes() == got[1].tobytes(), (key, s1, got)
        assert np.float64(s2).tobytes() == got[2].tobytes() or (np.isnan(s2) and np.isnan(got[2])), (key, s2, got)


SYNTHETIC = mc.synthetic_cases()


@pytest.fixture(scope="module")
def synthetic_want():
    cache = {}

    def get(name):
        if name not in cache:
            gt, pred, thr, cutoff = SYNTHETIC[name]
            cache[name] = mc.restated(gt, pred, mc.SYN_H, mc.SYN_P, thr, cutoff)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_synthetic_cases_exact(dev, synthetic_want, name):
    import mot_evaluator as me
    gt, pred, thr, cutoff = SYNTHETIC[name]
    want = synthetic_want(name)
    metrics, confusion, out = me.evaluate_tracks(gt, pred, _hg(mc.SYN_H, mc.SYN_P, dev), thr, cutoff, collect=True)
    got_iou = _device_ious(out)
    assert sorted(got_iou) == sorted(want["ious"])
    for f, mat in want["ious"].items():
        assert got_iou[f].tobytes() == mat.tobytes(), f
    _check_exact(metrics, confusion, out, want)
    _check_sums(out)
    for fig_name, (mean, std) in want["figures"].items():               # the same sums through the same formulas
        g = metrics[fig_name]
        dt = np.float64 if not isinstance(g[0], torch.Tensor) or g[0].dtype == torch.float64 else np.float32
        assert np.array_equal(np.array([float(g[0]), float(g[1])]), np.array([mean, std]).astype(dt).astype(np.float64),
                              equal_nan=True), fig_name


def test_limits_and_errors(dev):
    import mot_evaluator as me
    from retinanet_mi355x import _hip, ops
    hg = _hg(mc.SYN_H, mc.SYN_P, dev)
    gt, pred = mc.too_large_case()
    with pytest.raises(RuntimeError, match="MOT_MAX"):
        me.evaluate_tracks(gt, pred, hg)
    z = torch.zeros(4, dtype=torch.int32, device=dev)                    # the C entry refuses it too: an error code, no launch
    rc = _hip.load().rn_mot_assign(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, ops.MOT_MAX + 1, 1, 1,
                                   z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), _hip.stream())
    assert rc == 10001
    with pytest.raises(ValueError, match="invalid numeric entries"):
        me.evaluate_tracks(*mc.nan_case(), hg)
    gt, pred, thr = mc.no_tp_case()
    with pytest.raises(ZeroDivisionError):
        me.evaluate_tracks(gt, pred, hg, thr)


def test_repeatable_and_operators(dev, golden, tmp_path):
    """Two evaluations: bit-identical result blocks.  The registered operators run the same kernels."""
    import mot_evaluator as me
    from retinanet_mi355x import ops, torch_ops  # noqa: F401  (registers torch.ops.retinanet_mi355x.mot_*)
    gt, pred, thr, cutoff = SYNTHETIC["65x70"]
    hg = _hg(mc.SYN_H, mc.SYN_P, dev)
    pk = me.pack_tracks(gt, pred, hg, cutoff)
    a = me.run_packed(pk, hg, thr, dev, collect=True)
    b = me.run_packed(pk, hg, thr, dev)
    assert a["result"].tobytes() == b["result"].tobytes()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)     # noqa: E731
    t = torch.ops.retinanet_mi355x
    gt_state, gt_box, pred_box, pred_im = t.mot_prepare(up(pk["gt_im"]), up(pk["gt_h0"]), up(pk["gt_vel"]), up(pk["pred_state"]),
                                                        up(mc.SYN_H), up(mc.SYN_P))
    iou = t.mot_iou(gt_box, pred_box, pk["n_gt"], pk["n_pred"])
    assert iou.cpu().numpy().tobytes() == a["iou"].tobytes()
    assigned = t.mot_assign(iou, pk["n_gt"], pk["n_pred"])
    assert np.array_equal(assigned[1].cpu().numpy(), a["slot_col"])
    per_slot = t.mot_frame_metrics(iou, pk["n_gt"], pk["n_pred"], *assigned, float(thr), gt_state, up(pk["pred_state"]),
                                   up(pk["gt_im"]), pred_im, up(pk["gt_cls"]), up(pk["pred_cls"]), up(pk["gt_id"]), up(pk["pred_id"]))
    res = t.mot_reduce(pk["n_gt"], pk["n_pred"], *assigned, per_slot, up(pk["gt_id"]), up(pk["pred_id"]), len(pk["gid"]),
                       len(pk["pid"]))
    assert res.cpu().numpy().tobytes() == a["result"].tobytes()


@pytest.mark.parametrize("case", CASES)
def test_staged_golden_matrices(dev, golden, tmp_path, case):
    """The reference's IoU matrices straight into kernels 3-5."""
    import mot_evaluator as me
    g = golden("mot_eval")
    pkey, thr, frames = case_of(case)
    gt, pred = rows_of(golden, "gt", tmp_path)[1], rows_of(golden, pkey, tmp_path)[1]
    hg = _hg(g["H"], g["P"], dev)
    pk = me.pack_tracks(gt, pred, hg, frames)
    assert [f for f, n, m in zip(pk["frames"], pk["n_gt"], pk["n_pred"]) if n and m] == list(g[case + "_iou_frames"][:, 0])
    assert all(n and m for n, m in zip(pk["n_gt"], pk["n_pred"]))         # the cut holds no one-sided frame: offsets line up
    out = me.run_packed(pk, hg, thr, dev, ious=torch.from_numpy(g[case + "_iou"]).to(dev), collect=True)
    out["packed"] = pk
    got, a = _pairs(out), g[case + "_assign"]
    assert np.array_equal(got["pair_frame"], a[:, 0]) and np.array_equal(got["pair_gt"], a[:, 1])
    assert np.array_equal(got["pair_pred"], a[:, 2])
    assert got["pair_iou"].tobytes() == g[case + "_pre_thresh_iou"].tobytes()
    assert got["pair_iou"][got["pair_ok"]].tobytes() == g[case + "_match_iou"].tobytes()
    res = out["result"]
    assert [int(v) for v in res[:6]] == list(g[case + "_counters"])
    assert np.array_equal(res[52:152].astype(np.int64).reshape(10, 10), g[case + "_confusion"])
    assert int(res[6]) == len(g[case + "_gt_ids"]) and int(res[7]) == len(g[case + "_pred_ids"])
    ids = g[case + "_ids"]
    frag = len(ids) - len(set(ids[:, 0].tolist()))
    sw = sum(max(0, len(set(ids[ids[:, 1] == p, 0].tolist())) - 1) for p in set(ids[:, 1].tolist()))
    assert (int(res[8]), int(res[9])) == (frag, sw)
    if bool(g[case + "_raises_zero_division"]):
        with pytest.raises(ZeroDivisionError):
            me.metrics_from_result(res, thr)
    else:
        m, _ = me.metrics_from_result(res, thr)
        want = dict(zip((str(n) for n in g[case + "_metric_names"]), g[case + "_metric_values"]))
        assert m["Fragmentations"] == want["Fragmentations"] and m["ID switches"] == want["ID switches"] and m["MOTA"] == want["MOTA"]
    _check_sums(out)


@pytest.mark.parametrize("case", FIRST_CASES)
def test_end_to_end_on_the_reference_files(dev, golden, tmp_path, case):
    import mot_evaluator as me
    g = golden("mot_eval")
    pkey, thr, frames = case_of(case)
    gpath, ppath = rows_of(golden, "gt", tmp_path)[0], rows_of(golden, pkey, tmp_path)[0]
    hg = _hg(g["H"], g["P"], dev)
    ev = me.MOT_Evaluator(gpath, ppath, hg, {"match_iou": thr, "cutoff_frame": frames})
    metrics, confusion, out = me.evaluate_tracks(ev.gt, ev.pred, hg, thr, frames, collect=True)
    want_iou, got_iou = golden_ious(g, case), _device_ious(out)
    assert sorted(want_iou) == sorted(got_iou)
    eps = max(float(np.abs(got_iou[f] - want_iou[f]).max()) for f in want_iou)
    unstable = mc.unstable_frames(want_iou, thr, eps)
    print("%s: eps = max |IoU_device - IoU_reference| = %.3e over %d frames; unstable at 16 eps: %d"
          % (case, eps, len(want_iou), len(unstable)))
    assert len(unstable) <= 0.05 * len(want_iou), unstable
    a, got = g[case + "_assign"], _pairs(out)
    keep_w, keep_g = ~np.isin(a[:, 0], unstable), ~np.isin(got["pair_frame"], unstable)
    assert np.array_equal(got["pair_frame"][keep_g], a[keep_w, 0]) and np.array_equal(got["pair_gt"][keep_g], a[keep_w, 1])
    assert np.array_equal(got["pair_pred"][keep_g], a[keep_w, 2])
    assert np.array_equal(got["pair_ok"][keep_g], g[case + "_pre_thresh_iou"][keep_w] >= thr)
    _check_sums(out)
    if unstable:                                                         # the whole-sequence numbers hold only with nothing left out
        return
    assert [int(v) for v in out["result"][:6]] == list(g[case + "_counters"])
    assert np.array_equal(confusion, g[case + "_confusion"])
    want = dict(zip((str(n) for n in g[case + "_metric_names"]), g[case + "_metric_values"]))
    for k in INT_METRICS:
        assert float(metrics[k]) == want[k], k
    # the per-match vectors.  state_err: the ground-truth state comes through the transforms, which may differ from torch's in
    # the last bit -- 4 ulp of an fp32 at the largest coordinate (two values each within 1 ulp, doubled).  Pixel errors: fp64
    # throughout; this camera's far boxes project to 1e4 px because the homogeneous divisor cancels to a few hundredths, so a
    # few ulp of its terms (2e-16) come out as ~1e-10 px.  The bound is 1e-9 of the clamp of 500 px: 5e-7 px.
    ok = got["pair_ok"]
    tol = 4 * np.spacing(np.float32(max(np.abs(out["gt_state"]).max(), np.abs(out["packed"]["pred_state"]).max())))
    se_dev = float(np.abs(out["state_err"][ok].astype(np.float64) - g[case + "_state_err"]).max())
    px_dev = max(float(np.abs(out["bot"][ok] - g[case + "_bot_err"]).max()), float(np.abs(out["top"][ok] - g[case + "_top_err"]).max()))
    print("%s: state_err deviation %.3e (bound %.3e), pixel error deviation %.3e (bound 5e-7)" % (case, se_dev, tol, px_dev))
    assert se_dev <= tol and px_dev <= 1e-9 * 500
    dev_fig = 0.0
    for name, w in zip(g[case + "_figure_names"], g[case + "_figure_values"]):
        for x, y in zip(metrics[str(name)], w):
            dev_fig = max(dev_fig, abs(float(x) - y) / max(abs(y), 1.0))
    print("%s: figure deviation device vs reference %.3e (restatement vs reference %.3e, bound 4x)" % (case, dev_fig, FIRST_FIGURE_DEV))
    assert dev_fig <= 4 * FIRST_FIGURE_DEV
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        ev.evaluate(collect=True)
    assert text.getvalue()[text.getvalue().index("\n\n"):] == g[case + "_table"].tobytes().decode()
    # the lists the reference keeps in self.m, in its order
    ids = np.array([[gid, p] for gid, v in ev.m["ids"].items() for p in v], np.int64).reshape(-1, 2)
    assert np.array_equal(ids, g[case + "_ids"])
    assert ev.m["gt_ids"] == list(g[case + "_gt_ids"]) and ev.m["pred_ids"] == list(g[case + "_pred_ids"])
    assert [ev.m[k] for k in ("TP", "FP", "FN", "FP edge-case", "FP @ 0.2", "FN @ 0.2")] == list(g[case + "_counters"])
    assert np.abs(np.array(ev.m["pre_thresh_IOU"]) - g[case + "_pre_thresh_iou"]).max() <= eps
    assert len(ev.m["match_IOU"]) == len(g[case + "_match_iou"]) == len(ev.m["state_err"]) == len(ev.m["im_top_err"])
    assert ev.m["state_err"][0].dtype == torch.float32 and ev.m["im_bot_err"][0].dtype == torch.float64

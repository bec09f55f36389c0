"""CPU: the restatement of MOT_Evaluator.evaluate in tests/mot_cases.py against the reference's own results
(tests/golden/mot_eval.npz, written by tools/make_golden.py:gen_mot_eval), load_i24_csv, and the host side of the mirror.

The fixture: the reference's 3D_tracking_results.csv as ground truth against its _20 and _90 files, first 100 frames, at
match_iou 0 and 0.51.  The camera is fitted to the ground-truth file's own state and image-corner columns (it reprojects
them to 0.01 px), so boxes overlap where the trackers agree: at 0.51 there are true matches, and most pixel errors are below
the clamp.  The trackers drift apart after the first frames; from then on most pairs of a frame have IoU 0 and scipy's tie
rule decides, which the restatement and the staged device test reproduce exactly from the recorded matrices.  The
end-to-end device comparison needs frames that stay decided when the IoU moves in its last bit: the ``_first`` cases are
the prefixes (frames below 9 for _20, below 5 for _90) in which every frame is stable, asserted here from the golden
alone (test_first_frames_are_stable).

Exact: IoU matrices, assignments, match lists, counters, id lists, confusion matrix; bit-equal: the fp32 per-match state
errors; the fp64 pixel errors to PIXEL_DEV.  The (mean, deviation) figures: the restatement sums in fp64 in a fixed order, the reference in fp32 (torch) or
pairwise fp64 (numpy); FIGURE_DEV / FIRST_FIGURE_DEV below are the deviations measured between the two on this fixture, and
the GPU test gives the device 4x the latter on the _first cases."""
import contextlib
import io
import os

import numpy as np
import pytest

import mot_cases as mc

CASES = ("p20_iou0", "p20_iou51", "p90_iou0", "p90_iou51")                       # 100 frames: restatement and staged
FIRST_CASES = tuple(c + "_first" for c in CASES)                                # the stable prefixes: end to end
IOU_ULP = float(np.spacing(np.float32(1.0)))                                    # one fp32 ulp of an IoU just below 1


def case_of(case):
    """-> (prediction file key, match_iou, cutoff_frame)"""
    pkey = "pred20" if case.startswith("p20") else "pred90"
    return pkey, (0.51 if "iou51" in case else 0), ((9 if pkey == "pred20" else 5) if case.endswith("_first") else 100)
# largest |restated - reference| / max(|reference|, 1) over every figure, measured by test_restatement_equals_the_reference
# (printed there) and rounded up; the reference's fp32 sums are the cause.  Over the 100-frame cases: 1.43e-7 (1203 terms);
# over the _first cases, on which the device is compared with the reference: 3.34e-8
FIGURE_DEV = 1.5e-7
FIRST_FIGURE_DEV = 3.4e-8
# the fp64 pixel errors: the reference projects through a BLAS matrix product, whose summation order and fused multiply-adds
# are the library's, so they are not held to the bit.  This camera's far boxes project to 1e4 px because the homogeneous
# divisor cancels to a few hundredths; a few ulp of its terms (2e-16) come out as ~1e-10 px (measured: 3.5e-11).  The
# bound is 1e-9 of the clamp of 500 px.
PIXEL_DEV = 1e-9 * 500


def rows_of(golden, key, tmp_path):
    from homography import load_i24_csv
    path = os.path.join(str(tmp_path), key + ".csv")
    with open(path, "wb") as f:
        f.write(golden("mot_eval")[key + "_csv"].tobytes())
    return path, load_i24_csv(path)[1]


def golden_ious(g, case):
    out, o = {}, 0
    for f, n, m in g[case + "_iou_frames"]:
        out[int(f)] = g[case + "_iou"][o:o + n * m].reshape(n, m)
        o += n * m
    return out


def check_against_golden(g, case, r, exact_vectors=True):
    """What every path (restatement, device) is compared with exactly."""
    a = g[case + "_assign"]
    assert np.array_equal(r["pair_frame"], a[:, 0]) and np.array_equal(r["pair_gt"], a[:, 1]) and np.array_equal(r["pair_pred"], a[:, 2])
    assert np.array_equal(r["pair_iou"], g[case + "_pre_thresh_iou"])
    assert np.array_equal(r["pair_iou"][r["pair_ok"]], g[case + "_match_iou"])
    assert np.array_equal(r["confusion"], g[case + "_confusion"])
    if exact_vectors:
        assert r["state_err"].dtype == np.float32 and r["state_err"].tobytes() == g[case + "_state_err"].tobytes()
        px = max(np.abs(r["bot_err"] - g[case + "_bot_err"]).max(), np.abs(r["top_err"] - g[case + "_top_err"]).max())
        print("pixel error deviation restated vs reference, %s: %.3e" % (case, px))
        assert px <= PIXEL_DEV


@pytest.mark.parametrize("case", CASES + FIRST_CASES)
def test_restatement_equals_the_reference(golden, tmp_path, case):
    g = golden("mot_eval")
    pkey, thr, frames = case_of(case)
    gt, pred = rows_of(golden, "gt", tmp_path)[1], rows_of(golden, pkey, tmp_path)[1]
    want_iou = golden_ious(g, case)
    assert max(want_iou) < frames
    for f, mat in want_iou.items():                                       # the IoU arithmetic, before anything depends on it
        got = mc.iou_matrix(mc.prepare_gt(gt[f], g["H"], g["P"])[1], mc.prepare_pred(pred[f], g["P"])[1])
        assert got.tobytes() == mat.tobytes(), f
    if bool(g[case + "_raises_zero_division"]):
        with pytest.raises(ZeroDivisionError):
            mc.restated(gt, pred, g["H"], g["P"], thr, frames)
        # the bookkeeping up to the raise: rerun at a threshold that keeps it alive is not the same case, so compare the parts
        a, k = g[case + "_assign"], 0
        for f, mat in want_iou.items():
            ra, rb = mc.linear_sum_assignment(mat, maximize=True)
            assert np.array_equal(a[k:k + len(ra), 1], ra) and np.array_equal(a[k:k + len(ra), 2], rb)
            k += len(ra)
        assert g[case + "_counters"][0] == 0 and len(g[case + "_match_iou"]) == 0
        return
    r = mc.restated(gt, pred, g["H"], g["P"], thr, frames)
    check_against_golden(g, case, r)
    m = r["metrics"]
    assert [m[k] for k in ("TP", "FP", "FN", "FP edge-case", "FP @ 0.2", "FN @ 0.2")] == list(g[case + "_counters"])
    ids = np.array([[gid, p] for gid, v in r["ids"].items() for p in v], np.int64).reshape(-1, 2)
    assert np.array_equal(ids, g[case + "_ids"])
    assert r["gt_ids"] == list(g[case + "_gt_ids"]) and r["pred_ids"] == list(g[case + "_pred_ids"])
    for name, want in zip(g[case + "_metric_names"], g[case + "_metric_values"]):
        assert float(m[str(name)]) == want, name                          # integers and the ratios of integers
    dev = 0.0
    for name, want in zip(g[case + "_figure_names"], g[case + "_figure_values"]):
        got = r["figures"][str(name)]
        for a, b in zip(got, want):
            dev = max(dev, abs(a - b) / max(abs(b), 1.0))
    print("figure deviation restated vs reference, %s: %.3e" % (case, dev))
    assert dev <= (FIRST_FIGURE_DEV if case in FIRST_CASES else FIGURE_DEV)


@pytest.mark.parametrize("case", FIRST_CASES)
def test_first_frames_are_stable(golden, case):
    """The condition of the end-to-end comparison, from the reference's matrices alone: at most 5 % of the frames change
    their assignment or a threshold decision when every IoU moves by 16 ulp -- here none does -- and the cases are not
    trivial: matches above the threshold, pixel errors below the clamp."""
    import mot_evaluator as me
    g = golden("mot_eval")
    _, thr, frames = case_of(case)
    ious = golden_ious(g, case)
    assert len(ious) >= 4 and max(ious) < frames and me.STATE_COLS == tuple(mc.STATE_COLS)
    assert len(mc.unstable_frames(ious, thr, IOU_ULP)) <= 0.05 * len(ious)
    assert not bool(g[case + "_raises_zero_division"]) and g[case + "_counters"][0] >= 28
    assert (g[case + "_match_iou"] > 0.2).sum() >= 28
    assert (g[case + "_bot_err"] < 500).mean() > 0.8 and (g[case + "_top_err"] < 500).mean() > 0.8


def test_fixed_sums_order():
    """A self-check of the restatement the device is held to: the documented order, entry k to partial k % 256, partials
    in increasing order; invalid entries add +0.0.  The result block of the module has one (n, s1, s2) triple per figure."""
    import mot_evaluator as me
    from retinanet_mi355x import ops
    assert ops.MOT_RESULT == 52 + 100 and 16 + 3 * len(me.FIGURES) <= 52
    v = np.array([1e16, 1.0, -1e16] + [0.0] * 253 + [1.0], np.float64)      # entry 256 joins partial 0
    n, s1, _ = mc.fixed_sums(v)
    assert n == 257 and s1 == (1e16 + 1.0) + 1.0 + -1e16
    n, s1, s2 = mc.fixed_sums([3.0, 100.0, 5.0], [True, False, True])
    assert (n, s1, s2) == (2, 8.0, 2.0)


def test_known_answers_of_the_synthetic_cases():
    """A self-check of the cases the GPU test runs: the answers worked out by hand, and the size limit they are built to."""
    from retinanet_mi355x import ops
    cases = mc.synthetic_cases()
    assert len(cases["at_limit"][0][0]) == ops.MOT_MAX and len(mc.too_large_case()[1][0]) == ops.MOT_MAX + 1
    r = mc.restated(*cases["ids"][:2], mc.SYN_H, mc.SYN_P, *cases["ids"][2:])
    assert r["metrics"]["Fragmentations"] == 3 and r["ids"][3] == [21, 22, 21] and r["ids"][1] == [11, 12]
    assert r["metrics"]["ID switches"] == 1 and r["ids"][2] == [11]
    r = mc.restated(*cases["missing_frames"][:2], mc.SYN_H, mc.SYN_P, *cases["missing_frames"][2:])
    m = r["metrics"]
    assert (m["TP"], m["FP"], m["FN"]) == (1, 2, 2) and m["True unique objects"] == 2 and m["Predicted unique objects"] == 2
    r0 = mc.restated(*cases["zero_iou_0"][:2], mc.SYN_H, mc.SYN_P, *cases["zero_iou_0"][2:])
    r51 = mc.restated(*cases["zero_iou_51"][:2], mc.SYN_H, mc.SYN_P, *cases["zero_iou_51"][2:])
    assert r0["metrics"]["TP"] == 4 and r51["metrics"]["TP"] == 1 and r0["metrics"]["FP @ 0.2"] == r51["metrics"]["FP @ 0.2"] == 1
    r = mc.restated(*cases["rows_and_classes"][:2], mc.SYN_H, mc.SYN_P, *cases["rows_and_classes"][2:])
    assert r["confusion"][5, 5] == 1 and r["confusion"][3, 5] == 1 and r["confusion"][5, 4] == 1 and r["confusion"].sum() == 3
    assert r["state_err"][1, 6] == 500.0 and r["state_err"][0, 6] == 8.0          # clamp; "" velocity is 0
    r = mc.restated(*cases["edge_case"][:2], mc.SYN_H, mc.SYN_P, *cases["edge_case"][2:])
    assert r["metrics"]["FP edge-case"] == 3 and r["metrics"]["TP"] == 1
    with pytest.raises(ZeroDivisionError):
        gt, pred, thr = mc.no_tp_case()
        mc.restated(gt, pred, mc.SYN_H, mc.SYN_P, thr)
    with pytest.raises(ValueError):
        mc.restated(*mc.nan_case(), mc.SYN_H, mc.SYN_P)


def test_stability_rule():
    """A self-check of the rule that decides which frames the end-to-end comparison holds exactly; the statuses the module
    raises on are distinct from a clean frame."""
    from retinanet_mi355x import ops
    assert len({ops.MOT_OK, ops.MOT_INVALID, ops.MOT_INFEASIBLE, ops.MOT_TOO_LARGE}) == 4
    m = np.array([[0.9, 0.1], [0.2, 0.8]])
    assert mc.stable_frame(m, 0.51, 1e-7)
    assert not mc.stable_frame(np.array([[0.5, 0.5], [0.5, 0.5]]), 0.0, 1e-7)      # a tie
    assert not mc.stable_frame(np.array([[0.51 + 1e-7]]), 0.51, 1e-7)              # at the threshold
    assert mc.stable_frame(np.zeros((3, 4)), 0.51, 0.0)                            # identical matrices cannot differ


def test_load_i24_csv(tmp_path):
    from homography import load_i24_csv
    p = tmp_path / "t.csv"
    p.write_text("camera,p1c1\nnote\n\nFrame #,Timestamp,Object ID\n5,0.1,7\n\n3,0.2,8\n5,0.3,9\n")
    headers, data = load_i24_csv(str(p))
    assert headers == ["Frame #", "Timestamp", "Object ID"]
    assert list(data) == [5, 3] and data[5] == [["5", "0.1", "7"], ["5", "0.3", "9"]] and data[3] == [["3", "0.2", "8"]]


def test_mirror_interface_without_gpu(golden, tmp_path):
    import homography
    import mot_evaluator as me
    from retinanet_mi355x import ops, torch_ops
    for name in ("mot_prepare", "mot_iou", "mot_assign", "mot_frame_metrics", "mot_reduce"):
        assert name in torch_ops.OPERATORS
    assert ops.MOT_MAX == mc.MOT_MAX
    hg = homography.Homography()
    gpath = rows_of(golden, "gt", tmp_path)[0]
    with pytest.raises(NotImplementedError):
        me.MOT_Evaluator(gpath, gpath, hg, {"sequence": "video.mp4"})
    ev = me.MOT_Evaluator(gpath, gpath, hg, {"match_iou": 0.51, "cutoff_frame": 7})
    assert (ev.match_iou, ev.cutoff_frame, ev.sequence) == (0.51, 7, None) and ev.m["cls"].shape == (10, 10)
    assert set(ev.units) == {n for n, _ in mc.FIGURES}
    pk = me.pack_tracks(ev.gt, ev.pred, hg, 7)
    assert pk["frames"] == sorted(f for f in ev.gt if f < 7) and pk["gt_im"].shape == (sum(pk["n_gt"]), 8, 2)
    assert pk["pred_state"].dtype == np.float32 and pk["gt_id"].max() == len(pk["gid"]) - 1
    gt, pred = mc.too_large_case()
    with pytest.raises(RuntimeError, match="MOT_MAX"):                     # refused on the host, before any launch
        ops.mot_offsets([len(gt[0])], [len(pred[0])], "cpu")
    # the result block -> the reference's dict and table
    res = np.zeros(ops.MOT_RESULT)
    res[:11] = [4, 1, 2, 1, 0, 1, 3, 3, 1, 0, 5]
    for q in range(11):
        res[16 + 3 * q:19 + 3 * q] = [4, 8.0, 2.0]
    m, conf = me.metrics_from_result(res, 0)
    assert m["Recall"] == 4 / 6 and m["MOTA edge-case"] == 1 - (2 + 1 + 0 + 1 - 1) / 4 and isinstance(m["Match IOU"], tuple)
    assert float(m["Match IOU"][1]) == np.sqrt(0.5) and abs(float(m["X precision"][1]) - np.sqrt(2 / 3)) < 1e-7
    assert list(m)[:9] == ["iou_threshold", "True unique objects", "Predicted unique objects", "TP", "FP", "FN", "FP edge-case",
                           "FP @ 0.2", "FN @ 0.2"]
    ev.metrics, ev.confusion = m, conf
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        ev.print_metrics()
    assert "X precision                   : 2.00ft avg., 0.82ft st.dev." in text.getvalue()
    res[:] = 0
    with pytest.raises(ZeroDivisionError):
        me.metrics_from_result(res, 0)
    res[11], res[12] = ops.MOT_INVALID, 3
    with pytest.raises(ValueError):
        me.metrics_from_result(res, 0)

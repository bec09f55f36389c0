#!/usr/bin/env python3
"""Generate tests/golden/label_trajectory.npz by running the REFERENCE's own annotator methods (seems_to_be_working.py, and
adjust_boxes_with_trajectories of manual_annotator_state_v3.py) and scipy's UnivariateSpline.

The reference module is loaded unmodified from its checkout (never copied) under a private name, behind the stand-ins of
tools/make_golden.py, as tools/make_golden_label_rewrite.py does; the homographies are the REFERENCE's Homography /
Homography_Wrapper objects filled from the scene's matrices.  For every scene of tests/label_trajectory_cases.py:
golden_scenes() its methods create_trajectory (both metrics), get_splines, gen_trajectories and adjust_ts_with_trajectories
(use_running_error on and off, both metrics) run UNBOUND on a stand-in ``self``.  create_trajectory keeps its sorted boxes and
weights to itself: a tracer reads the locals ``boxes``, ``x_weight``, ``y_weight``, ``x_weight2`` and ``duration`` when the
method returns (it depends on these names, :1179-1223).  With those inputs every candidate smoothing factor is fitted again
with scipy.interpolate.UnivariateSpline directly, and its knot vector, coefficients, ier, residual and score are recorded (knots
and coefficients only for candidates inside the reference's knot limit).

Fixture conditions, asserted here on the reference's own numbers so that the tests' comparisons cannot be decided by rounding:
  * no two boxes of one object share a timestamp (torch.sort leaves ties unordered);
  * in every selection -- the candidates of an axis, the trials of a (frame, camera) -- the winner's score differs from every
    other DISTINCT score by more than 1e-9 relative (exactly equal scores are fine: the first wins on both sides).
A scene that fails is re-scripted, never exempted.

It also measures the restatement of tests/label_trajectory_cases.py against scipy over a stride of the golden candidates and
prints the largest relative deviation of coefficients and residuals (0.0: bit equality, which the host test then pins).  End
to end the restatement cannot be bit-equal: the reference projects the box corners with torch.bmm, whose sums differ from the
kernel's in the last bit for a few boxes, so a few weights differ by one ulp and the fits amplify that by their conditioning.
``<scene>_measured`` records that deviation (weights, coefficients, residuals, gen_trajectories values, reported figures); the
tests bound the end-to-end comparisons at 8x those figures, never at anything derived from the kernels' output.

adjust_boxes_with_trajectories is loaded the same way from the later annotator (matplotlib.collections gets a stand-in) and runs
on the scene without the ignored id 11 (it indexes ``splines`` with every id of a frame), with the splines of get_splines.

The file holds arrays only, outputs only; the inputs are scripted in tests/label_trajectory_cases.py.  This script needs the
reference checkout and scipy.

    python tools/make_golden_label_trajectory.py [--out DIR]
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402  (REF, the stand-ins; puts the package and tests/ on sys.path)
import make_golden_label_rewrite as mr      # noqa: E402  (import_reference, save_npz)
import label_trajectory_cases as tc         # noqa: E402  (tests/label_trajectory_cases.py)

METHODS = ("safe", "get_unused_id", "create_trajectory", "get_splines", "gen_trajectories", "adjust_ts_with_trajectories")
MIN_GAP = 1e-9
STRIDE = 9                                  # the restatement is measured on every STRIDE-th candidate


def stand_in(ref, hgmod, scene):
    members = {name: getattr(ref.Annotator, name) for name in METHODS if hasattr(ref.Annotator, name)}
    cls = type("StandIn", (tc.Labels,), members)
    return cls(scene, hgmod.Homography, hgmod.Homography_Wrapper)


def traced_locals(me, idx, metric):
    """me.create_trajectory(idx) -> (its result, its locals at return)."""
    code = type(me).create_trajectory.__code__
    kept = {}

    def local(frame, event, arg):
        if event == "return":
            kept.update(frame.f_locals)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        got = me.create_trajectory(idx, plot=False, metric=metric)
    finally:
        sys.settrace(None)
    return got, kept


def import_later_annotator(hgmod):
    """manual_annotator_state_v3.py, unmodified, under a private name."""
    import types
    if "matplotlib.collections" not in sys.modules:
        col = types.ModuleType("matplotlib.collections")
        col.LineCollection = type("LineCollection", (), {})
        sys.modules["matplotlib.collections"] = col
    mr._forget()
    sys.path.insert(0, mg.REF)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            v3 = mg.ref_module_from_file("_reference_annotator_v3", "manual_annotator_state_v3.py")
    finally:
        sys.path.remove(mg.REF)
        mr._forget()
    return v3


def check_gap(scores, win, what):
    s = np.asarray(scores, np.float64)
    others = s[np.isfinite(s) & (s != s[win])]
    if len(others) and not np.all(np.abs(others - s[win]) > MIN_GAP * np.abs(s[win])):
        raise SystemExit("fixture condition: %s: the winner's score %r is within 1e-9 of another" % (what, s[win]))
    assert win == tc.first_smallest(list(s)), what


def candidates(t, v, w, w2, k, tpes, limit, axis, metric_scores):
    """Every candidate through scipy -> dict of arrays; metric_scores: {metric: list to fill}."""
    from scipy.interpolate import UnivariateSpline
    m, NC = len(t), len(tpes)
    cap = tc.ncap_of(limit, k, m)
    out = dict(n=np.zeros(NC, np.int32), ier=np.zeros(NC, np.int32), fp=np.zeros(NC), t=np.zeros((NC, cap)), c=np.zeros((NC, cap)))
    for metric in metric_scores:
        out["score_" + metric] = np.full(NC, np.nan)
    for j, tpe in enumerate(tpes):
        spl = UnivariateSpline(t, v, k=k, w=w, s=tc.smoothing(tpe, m))
        tt, cc, _ = spl._eval_args
        n = len(tt)
        out["n"][j], out["ier"][j], out["fp"][j] = n, spl._data[-1], spl.get_residual()
        if np.isnan(spl(0)) or len(spl.get_knots()) > limit:
            continue
        out["t"][j, :n], out["c"][j, :n - k - 1] = tt, cc[:n - k - 1]
        pe = (w2 * (spl(t) - v)) ** 2
        for metric in metric_scores:
            if metric == "ape":
                out["score_" + metric][j] = np.sqrt(np.mean(pe))
            else:
                out["score_" + metric][j] = np.sqrt(np.max(pe)) if axis == 0 else np.mean(np.max(pe))
    return out


def measure(t, v, w, k, tpes, limit, gold, worst):
    """The restatement against scipy on a stride of the candidates -> updates worst = [coefficients, residual]."""
    m = len(t)
    for j in range(0, len(tpes), STRIDE):
        f = tc.fit(t, v, w, k, tc.smoothing(tpes[j], m), tc.ncap_of(limit, k, m))
        if f["ier"] == tc.REJECTED:
            assert gold["n"][j] - 2 * k > limit
            continue
        n = gold["n"][j]
        assert f["n"] == n and f["ier"] == gold["ier"][j] and np.array_equal(f["t"], gold["t"][j, :n]), (j, f["n"], n, f["ier"])
        c = gold["c"][j, :n - k - 1]
        worst[0] = max(worst[0], float(np.max(np.abs(f["c"] - c) / np.maximum(np.abs(c), 1e-300))))
        worst[1] = max(worst[1], abs(f["fp"] - gold["fp"][j]) / abs(gold["fp"][j]))


def spline_arrays(spl):
    tt, cc, k = spl._eval_args
    return np.asarray(tt, np.float64), np.asarray(cc[:len(tt) - k - 1], np.float64)


def run_scene(ref, hgmod, name, scene, worst, tally):
    out, names = {}, scene["names"]
    tpex, tpey = tc.tpe_x(), tc.tpe_y()
    me = stand_in(ref, hgmod, scene)
    n_ids = me.get_unused_id()
    out["n_ids"] = np.array([n_ids], np.int64)
    for idx in range(n_ids):
        res = {}
        for metric in ("ape", "mpe"):
            res[metric], loc = traced_locals(stand_in(ref, hgmod, scene), idx, metric)
        tag = "o%d_" % idx
        state = 0 if not hasattr(loc.get("boxes"), "numpy") else (1 if loc["duration"] < 3 else 2)   # no boxes / too short / fitted
        out[tag + "state"] = np.array([state], np.int64)
        if out[tag + "state"][0] == 0:
            continue
        boxes = loc["boxes"].numpy()
        t, x, y = boxes[:, 6].copy(), boxes[:, 0].copy(), boxes[:, 1].copy()
        xw, yw = loc["x_weight"].numpy().astype(np.float64), loc["y_weight"].numpy().astype(np.float64)
        assert loc["x_weight"].dtype.is_floating_point and len(set(t.tolist())) == len(t), "fixture condition: tied timestamps"
        out[tag + "rows"] = np.stack([t, x, y, xw, yw], axis=1)
        out[tag + "duration"] = np.array([loc["duration"]], np.float64)
        if out[tag + "state"][0] == 1:
            continue
        xw2 = loc["x_weight2"].numpy().astype(np.float64)
        out[tag + "xw2"] = xw2
        dur = np.floor(loc["duration"])
        for axis, v, w, w2, k, tpes, limit in ((0, x, xw, xw2, 3, tpex, dur * 4 + 2), (1, y, yw, yw, 2, tpey, dur + 2)):
            gold = candidates(t, v, w, w2, k, tpes, limit, axis, ("ape", "mpe"))
            for key, arr in gold.items():
                out[tag + "xy"[axis] + "_" + key] = arr
            for metric in ("ape", "mpe"):
                sc = gold["score_" + metric]
                win = tc.first_smallest(list(sc))
                out[tag + "xy"[axis] + "_win_" + metric] = np.array([win], np.int64)
                if win >= 0:
                    check_gap(sc, win, "%s object %d axis %d %s" % (name, idx, axis, metric))
                    spl = res[metric][1 + axis] if res[metric][0] is not None else None
                    if spl is not None:                         # the reference's own pick is the recorded winner
                        tt, cc = spline_arrays(spl)
                        n = gold["n"][win]
                        assert len(tt) == n and np.array_equal(tt, gold["t"][win, :n]) and np.array_equal(cc, gold["c"][win, :n - k - 1])
            acc = gold["n"] - 2 * k <= limit
            for e in np.unique(gold["ier"][acc]):
                tally[int(e)] = tally.get(int(e), 0) + int((gold["ier"][acc] == e).sum())
            tally["rejected"] = tally.get("rejected", 0) + int((~acc).sum())
            measure(t, v, w, k, tpes, limit, gold, worst)
            cache = {}
            for j in range(len(tpes)):                          # the restatement's scores (ascending sums) against numpy's
                n = int(gold["n"][j])
                if n - 2 * k > limit:
                    continue
                for metric in ("ape", "mpe"):
                    key = (metric, gold["t"][j, :n].tobytes(), gold["c"][j, :n].tobytes())
                    if key not in cache:
                        cache[key] = tc.score(gold["t"][j], gold["c"][j], n, k, t, v, w2, metric, axis)
                    want = gold["score_" + metric][j]
                    assert np.isnan(want) == np.isnan(cache[key])
                    if not np.isnan(want):
                        worst[2] = max(worst[2], abs(cache[key] - want) / abs(want))
        for metric in ("ape", "mpe"):
            r = res[metric]
            out[tag + "none_" + metric] = np.array([r[1] is None], np.bool_)
            if r[1] is not None:
                out[tag + "fig_" + metric] = np.array([r[3], r[4]], np.float64)
    # the passes
    me = stand_in(ref, hgmod, scene)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        me.get_splines(plot=False)
    out["summary"] = np.frombuffer(log.getvalue().strip().split("\n")[-1].encode(), np.uint8)
    splines = me.splines
    for idx, (xs, ys) in enumerate(splines):
        out["s%d_none" % idx] = np.array([xs is None], np.bool_)
        if xs is not None:
            for a, spl in (("x", xs), ("y", ys)):
                out["s%d_%s_t" % (idx, a)], out["s%d_%s_c" % (idx, a)] = spline_arrays(spl)
    me.gen_trajectories()
    out["gen_idx"], out["gen_val"] = tc.dump_xyt(me.spline_data, names)
    out["measured"] = end_to_end_deviation(scene, out)
    v3 = import_later_annotator(hgmod)
    scene2 = tc.without_id(scene, 11)
    cls = type("StandIn3", (tc.Labels,), {"adjust_boxes_with_trajectories": v3.Annotator.adjust_boxes_with_trajectories})
    for tag, sx, sy in (("boxes", 2, 2), ("boxes_tight", 0.05, 0.02)):
        me = cls(scene2, hgmod.Homography, hgmod.Homography_Wrapper)
        me.splines = splines
        shifts = me.adjust_boxes_with_trajectories(max_shift_x=sx, max_shift_y=sy)
        out[tag + "_idx"], out[tag + "_val"] = tc.dump_xyt(me.data, names)
        out[tag + "_shifts"] = np.array(shifts, np.float64).reshape(-1)
        # the restatement (its own box diffs, one ulp from torch.bmm's for a few boxes) on the reference's splines
        mine = tc.Labels(scene2)
        rs = [[None, None] if xs is None else [dict(zip("tc", spline_arrays(xs)), n=len(xs._eval_args[0]), k=3),
                                               dict(zip("tc", spline_arrays(ys)), n=len(ys._eval_args[0]), k=2)] for xs, ys in splines]
        got = tc.ref_adjust_boxes(mine, rs, sx, sy)
        idx, val = tc.dump_xyt(mine.data, names)
        assert np.array_equal(idx, out[tag + "_idx"]) and len(got) == len(shifts)
        dev = max(np.max(np.max(np.abs(val - out[tag + "_val"]), axis=0) / np.max(np.abs(out[tag + "_val"]), axis=0)),
                  np.max(np.abs(np.array(got) - out[tag + "_shifts"])) / np.max(out[tag + "_shifts"]))
        out["boxes_measured"] = np.maximum(out.get("boxes_measured", np.zeros(1)), dev)
        # ... and END TO END: on the splines the restatement fitted from its own weights (a shift is a difference of nearly equal
        # numbers, so its deviation relative to the largest shift is far above that of the positions)
        mine = tc.Labels(scene2)
        got = tc.ref_adjust_boxes(mine, out["_restated_splines"], sx, sy)
        idx, val = tc.dump_xyt(mine.data, names)
        dev = max(np.max(np.max(np.abs(val - out[tag + "_val"]), axis=0) / np.max(np.abs(out[tag + "_val"]), axis=0)),
                  np.max(np.abs(np.array(got) - out[tag + "_shifts"])) / np.max(out[tag + "_shifts"]))
        out["boxes_e2e_measured"] = np.maximum(out.get("boxes_e2e_measured", np.zeros(1)), dev)
    del out["_restated_splines"]
    for run in (True, False):
        for metric in ("ape", "mpe"):
            me = stand_in(ref, hgmod, scene)
            me.splines = splines
            before = tc.dump_xyt(me.data, names)
            me.adjust_ts_with_trajectories(metric=metric, use_running_error=run, overwrite_ts_data=True)
            tag = "ts_%d_%s_" % (run, metric)
            out[tag + "idx"], out[tag + "val"] = tc.dump_xyt(me.data, names)
            out[tag + "all_ts"] = tc.lc.ts_table(me.all_ts, names)
            assert np.array_equal(before[0], out[tag + "idx"])
            check_shift_gaps(scene, splines, metric, run, name)
    return {name + "_" + k: v for k, v in out.items()}


def end_to_end_deviation(scene, out):
    """The restatement END TO END -- its own box weights, whose projection is not torch.bmm's to the last bit, then the fit of
    every winning candidate of get_splines (metric "mpe") -- against the reference -> fp64 [5]: the largest relative deviation
    of a weight, of a spline's coefficients (max |dc| / max |c|), of a residual, of a gen_trajectories value (per column, max
    |dv| / max |v|) and of a reported figure.  The knot vectors, n and ier must still be equal."""
    me = tc.Labels(scene)
    dev = np.zeros(5)
    splines = []
    for idx in range(int(out["n_ids"][0])):
        rows = tc.object_rows(me, idx)
        if rows is not None:
            want = out["o%d_rows" % idx]
            assert np.array_equal(np.stack([rows["t"], rows["x"], rows["y"]], 1), want[:, :3])
            dev[0] = max(dev[0], np.max(np.abs(np.stack([rows["xw"], rows["yw"]], 1) - want[:, 3:]) / want[:, 3:]))
        if out["s%d_none" % idx][0]:
            splines.append([None, None])
            continue
        m, dur, pair = len(rows["t"]), np.floor(rows["duration"]), []
        for a, k, v, w, tpes, limit in (("x", 3, rows["x"], rows["xw"], tc.tpe_x(), dur * 4 + 2), ("y", 2, rows["y"], rows["yw"], tc.tpe_y(), dur + 2)):
            j = int(out["o%d_%s_win_mpe" % (idx, a)][0])
            f = tc.fit(rows["t"], v, w, k, tc.smoothing(tpes[j], m), tc.ncap_of(limit, k, m))
            t, c = out["s%d_%s_t" % (idx, a)], out["s%d_%s_c" % (idx, a)]
            assert f["n"] == len(t) and f["ier"] == out["o%d_%s_ier" % (idx, a)][j] and np.array_equal(f["t"], t), (idx, a)
            dev[1] = max(dev[1], np.max(np.abs(f["c"] - c)) / np.max(np.abs(c)))
            dev[2] = max(dev[2], abs(f["fp"] - out["o%d_%s_fp" % (idx, a)][j]) / out["o%d_%s_fp" % (idx, a)][j])
            pair.append(dict(t=f["t"], c=f["c"], n=f["n"], k=k))
            if a == "x":
                fig = tc.figures(f["t"], f["c"], f["n"], k, rows["t"], v, w)
                dev[4] = max(dev[4], np.max(np.abs(np.array(fig[:2]) - out["o%d_fig_mpe" % idx]) / out["o%d_fig_mpe" % idx]))
        splines.append(pair)
    idx, val = tc.dump_xyt(tc.ref_gen_trajectories(me, splines), scene["names"])
    assert np.array_equal(idx, out["gen_idx"]) and np.array_equal(val[:, 2], out["gen_val"][:, 2])
    dev[3] = np.max(np.max(np.abs(val[:, :2] - out["gen_val"][:, :2]), axis=0) / np.max(np.abs(out["gen_val"][:, :2]), axis=0))
    out["_restated_splines"] = splines
    return dev


def check_shift_gaps(scene, splines, metric, run, name):
    """The trial errors of every (frame, camera), from scipy's splines with the restatement's arithmetic: the gap condition."""
    me = tc.Labels(scene)
    shifts = np.linspace(-0.01, 0.01, 21)
    running = [float(me.ts_bias[i]) for i in range(len(me.seq_keys))]
    n_ids = tc.lc.unused_id(me.data)
    for f_idx, frame in enumerate(me.data):
        if f_idx > me.last_frame or len(frame) == 0:
            break
        for c_idx, cam in enumerate(me.seq_keys):
            kept = [i for i in range(n_ids) if frame.get("{}_{}".format(cam, i)) is not None and splines[i][0] is not None]
            if not kept:
                continue
            xl = np.array([frame["{}_{}".format(cam, i)]["x"] for i in kept])
            errs = []
            for sh in shifts:
                t = me.all_ts[f_idx][cam] + sh + (running[c_idx] if run else 0.0)
                d = (np.array([np.float32(splines[i][0](t)) for i in kept]).astype(np.float64) - xl) ** 2
                errs.append(np.sqrt(np.mean(d)) if metric == "ape" else np.sqrt(np.max(d)))
            check_gap(errs, tc.first_smallest(errs), "%s frame %d camera %d %s run %d" % (name, f_idx, c_idx, metric, run))
            if run:
                running[c_idx] += shifts[-1]


def run_direct(out, worst, tally):
    """tc.direct_case(seed) through UnivariateSpline -> direct_n / ier / fp / t / c, rows padded with zeros."""
    from scipy.interpolate import UnivariateSpline
    rows = []
    for seed in tc.DIRECT_SEEDS:
        x, y, w, k, s = tc.direct_case(seed)
        spl = UnivariateSpline(x, y, k=k, w=w, s=s)
        tt, cc, _ = spl._eval_args
        n, ier = len(tt), int(spl._data[-1])
        rows.append((n, ier, spl.get_residual(), tt, cc[:n - k - 1]))
        tally["direct %d" % ier] = tally.get("direct %d" % ier, 0) + 1
        f = tc.fit(x, y, w, k, s, len(x) + k + 1)
        assert f["n"] == n and f["ier"] == ier and np.array_equal(f["t"], tt), ("direct", seed)
        worst[0] = max(worst[0], float(np.max(np.abs(f["c"] - cc[:n - k - 1]) / np.maximum(np.abs(cc[:n - k - 1]), 1e-300))))
        worst[1] = max(worst[1], abs(f["fp"] - rows[-1][2]) / max(abs(rows[-1][2]), 1e-300))
    width = max(r[0] for r in rows)
    out["direct_n"] = np.array([r[0] for r in rows], np.int32)
    out["direct_ier"] = np.array([r[1] for r in rows], np.int32)
    out["direct_fp"] = np.array([r[2] for r in rows], np.float64)
    out["direct_t"], out["direct_c"] = np.zeros((len(rows), width)), np.zeros((len(rows), width))
    for i, r in enumerate(rows):
        out["direct_t"][i, :r[0]], out["direct_c"][i, :len(r[4])] = r[3], r[4]


def main(out_dir):
    ref, hgmod = mr.import_reference()
    out, worst, tally = {}, [0.0, 0.0, 0.0], {}
    warnings.simplefilter("ignore")
    run_direct(out, worst, tally)
    for name, scene in tc.golden_scenes().items():
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            got = run_scene(ref, hgmod, name, scene, worst, tally)
        out.update(got)
        print("%-6s %d arrays, %d printed lines; accepted candidates by ier %s"
              % (name, len(got), log.getvalue().count("\n"), sorted(tally.items(), key=str)))
        print("       summary: " + bytes(got[name + "_summary"]).decode())
    print("restatement against scipy over the direct cases and every %d-th candidate: largest relative deviation of a coefficient "
          "%.3g, of a residual %.3g" % (STRIDE, worst[0], worst[1]))
    print("the restatement's scores against numpy's over every accepted candidate: largest relative deviation %.3g" % worst[2])
    out["score_measured"] = np.array([worst[2]], np.float64)
    print("adjust_boxes_with_trajectories restated (own box diffs) against the later annotator: largest relative deviation %.3g on "
          "the reference's splines, %.3g end to end (its own splines)" % (out["traj_boxes_measured"][0], out["traj_boxes_e2e_measured"][0]))
    for name in tc.golden_scenes():
        print("%s end to end (own box weights): largest relative deviation of a weight %.3g, of a spline's coefficients %.3g, of a "
              "residual %.3g, of a gen_trajectories value %.3g, of a reported figure %.3g"
              % ((name,) + tuple(out[name + "_measured"])))
    path = os.path.join(out_dir, "label_trajectory.npz")
    mr.save_npz(path, out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)

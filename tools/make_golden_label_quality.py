#!/usr/bin/env python3
"""Generate tests/golden/label_quality.npz by running the REFERENCE's own scoring functions (manual_annotator_state_v3.py):
calculate_total_variation, calculate_feasibility and annotator_rmse.

The later annotator is loaded unmodified from its checkout (never copied) under a private name, through
``import_later_annotator`` of tools/make_golden_label_trajectory.py; the homographies are the REFERENCE's Homography /
Homography_Wrapper objects filled from the scene's matrices.  For every scene of tests/label_quality_cases.py:golden_scenes()
the three module-level functions run on a stand-in ``ann`` (the scene's labels with the reference's ``safe`` and
``get_unused_id``).  calculate_feasibility keeps its series to itself and annotator_rmse returns nothing: a line tracer reads
the locals ``time``, ``v``, ``a``, ``theta`` of the first every time ``f_percentage`` has grown, and ``mses`` and ``rmse`` of the
second at its return (it depends on these names, :3896-3978 and :3982-4006).

Fixture conditions, asserted here on the reference's own numbers so that the tests' comparisons cannot be decided by rounding:
  * no two boxes of one object share a timestamp (np.argsort leaves ties unordered);
  * no theta lies within 1e-9 relative of +-25 degrees (the feasibility masks cannot hang on the last bit of atan2).
A scene that fails is re-scripted, never exempted.

The file holds arrays only, outputs only; the inputs are scripted in tests/label_quality_cases.py.  This script needs the
reference checkout.

    python tools/make_golden_label_quality.py [--out DIR]
"""
import contextlib
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402  (REF, the stand-ins; puts the package and tests/ on sys.path)
import make_golden_label_rewrite as mr      # noqa: E402  (import_reference, save_npz)
import make_golden_label_trajectory as mt   # noqa: E402  (import_later_annotator)
import label_quality_cases as qc            # noqa: E402  (tests/label_quality_cases.py)

MIN_GAP = 1e-9


def stand_in(v3, hgmod, scene):
    members = {name: getattr(v3.Annotator, name) for name in ("safe", "get_unused_id")}
    cls = type("StandIn", (qc.rc.Labels,), members)
    return cls(scene, hgmod.Homography, hgmod.Homography_Wrapper)


def traced_feasibility(v3, me):
    """v3.calculate_feasibility(me) -> (its result, per appended object its (time, v, a, theta))."""
    code = v3.calculate_feasibility.__code__
    got = []

    def local(frame, event, arg):
        f = frame.f_locals.get("f_percentage")
        if f is not None and len(f) > len(got):                 # appended on the line before: the locals are that object's
            got.append(tuple(np.array(frame.f_locals[k], np.float64).copy() for k in ("time", "v", "a", "theta")))
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        res = v3.calculate_feasibility(me)
    finally:
        sys.settrace(None)
    assert len(got) == len(res)
    return res, got


def traced_rmse(v3, me):
    """v3.annotator_rmse(me) -> (rmse, per-group rmse) from its locals at return."""
    code = v3.annotator_rmse.__code__
    kept = {}

    def local(frame, event, arg):
        if event == "return":
            kept.update(frame.f_locals)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        v3.annotator_rmse(me)
    finally:
        sys.settrace(None)
    return float(kept["rmse"]), [float(m) for m in kept["mses"]]


def check_fixture(name, scene, series):
    offsets, cols, _ = qc.table(scene["data"], scene["names"])
    C = len(scene["names"])
    for obj in range((len(offsets) - 1) // C):
        t = cols[offsets[obj * C]:offsets[(obj + 1) * C], 2]
        if len(set(t.tolist())) != len(t):
            raise SystemExit("fixture condition: %s object %d has tied timestamps" % (name, obj))
    for _, _, _, theta in series:
        for edge in qc.THETA_RANGE:
            if np.any(np.abs(theta - edge) <= MIN_GAP * abs(edge)):
                raise SystemExit("fixture condition: %s has a theta within 1e-9 of %d degrees" % (name, edge))


def run_scene(v3, hgmod, name, scene):
    out = {}
    x_var, x_range = v3.calculate_total_variation(stand_in(v3, hgmod, scene))
    out["x_var"], out["x_range"] = np.array(x_var, np.float64), np.array(x_range, np.float64)
    feasible, series = traced_feasibility(v3, stand_in(v3, hgmod, scene))
    check_fixture(name, scene, series)
    out["feasible"] = np.array(feasible, np.float64)
    restated = qc.ref_kinematics(qc.rc.Labels(scene))
    assert len(restated) == len(series)
    out["ids"] = np.array([k[0] for k in restated], np.int64)   # the ids are the restatement's: the reference keeps none
    for col, key in enumerate(("time", "v", "a", "theta")):
        out["off"], out[key] = qc.ragged([s[col] for s in series])
    rmse, per = traced_rmse(v3, stand_in(v3, hgmod, scene))
    out["rmse"], out["rmse_groups"] = np.array([rmse], np.float64), np.array(per, np.float64)
    _, _, counts, largest = qc.ref_annotator_rmse(qc.rc.Labels(scene))
    out["rmse_counts"], out["rmse_largest"] = np.array(counts, np.int64), np.array(largest, np.float64)
    return {name + "_" + k: v for k, v in out.items()}


def main(out_dir):
    _, hgmod = mr.import_reference()
    v3 = mt.import_later_annotator(hgmod)
    out = {}
    for name, scene in qc.golden_scenes().items():
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            got = run_scene(v3, hgmod, name, scene)
        out.update(got)
        mine = qc.restated(name, scene)
        exact = [k for k in ("x_var", "x_range", "feasible", "time", "v", "a") if np.array_equal(got[name + "_" + k], mine[name + "_" + k])]
        print("%-6s %d arrays, %d printed lines; %d objects with a series, feasible fractions %s; restatement bit-equal on %s"
              % (name, len(got), log.getvalue().count("\n"), len(got[name + "_ids"]), np.round(got[name + "_feasible"], 3).tolist(),
                 ", ".join(exact)))
        print("       " + log.getvalue().strip().split("\n")[0])
    path = os.path.join(out_dir, "label_quality.npz")
    mr.save_npz(path, out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)

#!/usr/bin/env python3
"""Generate tests/golden/label_audit.npz by running the REFERENCE's own annotator methods (seems_to_be_working.py) -- build
container only.

The reference module is loaded unmodified from its checkout (never copied) under a private name, behind the stand-ins of
tools/make_golden.py (torchvision, cv2, matplotlib); importing it builds no window.  For every scene of
tests/label_audit_cases.py:golden_scenes() its methods estimate_ts_bias, est_y_error, estimate_projection_error (with and
without reverse_curve_offset), remove_outliers, interpolate (every object below the first unused id, then id 4) and
unbias_timestamps run UNBOUND on a stand-in ``self`` that carries only the attributes they read.  estimate_ts_bias and
est_y_error keep their lists to themselves: a line tracer reads the local ``diffs`` once it has become an array (it depends on
the reference's local names diffs, cam_idx and decrement, :1860-1926 and :1963-2024).  The file holds arrays only, outputs
only; the inputs are scripted in tests/label_audit_cases.py.  This script refuses to run without the reference and is never
executed on the GPU box.

    python tools/make_golden_labels.py [--out DIR]
"""
import contextlib
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402  (REF, the stand-ins; puts the package and tests/ on sys.path)
import label_audit_cases as lc              # noqa: E402  (tests/label_audit_cases.py)

METHODS = ("safe", "get_unused_id", "estimate_ts_bias", "est_y_error", "estimate_projection_error", "remove_outliers",
           "interpolate", "unbias_timestamps")


def import_reference():
    if not os.path.isfile(os.path.join(mg.REF, "seems_to_be_working.py")):
        raise SystemExit("the reference checkout (%s) is needed to write this fixture" % mg.REF)
    mg.install_shims()
    mg.tracker_import_shims()
    shadowed = ("homography", "datareader", "timestamp_utilities")
    for k in [k for k in sys.modules if k in shadowed or k == "retinanet" or k.startswith("retinanet.")]:
        del sys.modules[k]
    sys.path.insert(0, mg.REF)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ref = mg.ref_module_from_file("_reference_annotator", "seems_to_be_working.py")
    finally:
        sys.path.remove(mg.REF)
    for k in [k for k in sys.modules if k in shadowed or k == "retinanet" or k.startswith("retinanet.")]:
        del sys.modules[k]                  # later imports of these names are not to find the reference's
    return ref


def stand_in(ref, scene):
    """lc.Labels with the reference's methods as its own."""
    cls = type("StandIn", (lc.Labels,), {name: getattr(ref.Annotator, name) for name in METHODS})
    return cls(scene)


def traced_diffs(me, method):
    """Runs me.<method>() under a line tracer -> ([(cam, prev)], [diffs array]) of every pair that had samples."""
    code = getattr(type(me), method).__code__
    got, last = {}, [None]

    def local(frame, event, arg):
        loc = frame.f_locals
        d = loc.get("diffs")
        if isinstance(d, np.ndarray) and d is not last[0]:      # the array is new: cam_idx and decrement are still its own
            last[0] = d
            cam = loc["cam_idx"]
            assert (cam, cam - loc.get("decrement", 1)) not in got
            got[(cam, cam - loc.get("decrement", 1))] = d.copy()
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        getattr(me, method)()
    finally:
        sys.settrace(None)
    pairs = list(got)
    return pairs, [got[p] for p in pairs]


def run_scene(ref, name, scene):
    out, names = {}, scene["names"]
    me = stand_in(ref, scene)
    pairs, lists = traced_diffs(me, "estimate_ts_bias")
    out["ts_pairs"], out["ts_off"], out["ts_diffs"] = lc.ragged(pairs, lists)
    out["ts_bias"] = np.array(me.ts_bias, np.float64)
    me = stand_in(ref, scene)
    pairs, lists = traced_diffs(me, "est_y_error")
    out["y_pairs"], out["y_off"], out["y_diffs"] = lc.ragged(pairs, lists)
    out["y_means"] = np.array([np.mean(a) for a in lists], np.float64).reshape(-1)
    for tag, flag in (("proj", False), ("curve", True)):
        xe, ye = stand_in(ref, scene).estimate_projection_error(reverse_curve_offset=flag)
        out[tag + "_x"], out[tag + "_y"] = np.array(xe, np.float64).reshape(-1), np.array(ye, np.float64).reshape(-1)
    me = stand_in(ref, scene)
    me.remove_outliers()
    out["outliers_idx"], out["outliers_val"] = lc.dump(me.data, names)
    me = stand_in(ref, scene)
    for i in range(me.get_unused_id()):
        me.interpolate(i, verbose=False)
    me.interpolate(4, verbose=False)
    out["interp_idx"], out["interp_val"] = lc.dump(me.data, names)
    me = stand_in(ref, scene)
    me.unbias_timestamps()
    out["unbias_idx"], out["unbias_val"] = lc.dump(me.data, names)
    out["unbias_ts"], out["unbias_bias"] = lc.ts_table(me.all_ts, names), np.array(me.ts_bias, np.float64)
    return {name + "_" + k: v for k, v in out.items()}


def main(out_dir):
    ref = import_reference()
    out = {}
    for name, scene in lc.golden_scenes().items():
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            got = run_scene(ref, name, scene)
        out.update(got)
        print("%-9s %d arrays, %d diffs, %d boxes after interpolation, %d printed lines"
              % (name, len(got), len(got[name + "_ts_diffs"]), len(got[name + "_interp_idx"]), log.getvalue().count("\n")))
    np.savez_compressed(os.path.join(out_dir, "label_audit.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)

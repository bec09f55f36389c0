#!/usr/bin/env python3
"""Time the spline trajectories (label_trajectory.py / csrc/label_spline.hip) on the generated label set of
tools/bench_label_audit.py -- 18 cameras x 3 600 frames x 300 objects by default.  Device times come from HIP events around the
launches of every chunk; the host's packing pass and the whole calls are wall clock.  Where scipy is importable the same fits
are timed through scipy's UnivariateSpline on the CPU for a sample of the objects (the reference's loop of 200 + 100 fits per
object, without its scoring) and scaled to all of them; where it is not, the file says so.  Reported, not a gate.

    python tools/bench_label_trajectory.py [--cameras 18] [--frames 3600] [--objects 300] [--sample 3] [--out profiles/label_trajectory.txt]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

import homography                            # noqa: E402
import label_audit as la                     # noqa: E402
import label_trajectory as lt                # noqa: E402
import label_trajectory_cases as tc          # noqa: E402
from bench_label_audit import big_scene, wall    # noqa: E402
from retinanet_mi355x import ops             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--objects", type=int, default=300)
    ap.add_argument("--sample", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    t = time.perf_counter()
    scene = big_scene(args.cameras, args.frames, args.objects)
    scene["hg_old"] = tc.rc.hg_spec(scene["names"])
    boxes = sum(len(fd) for fd in scene["data"])
    say("spline trajectories on %s (the name the runtime reports): %d cameras, %d frames, %d objects, %d boxes (scene built in %.1f s)"
        % (torch.cuda.get_device_name(0), args.cameras, args.frames, args.objects, boxes, time.perf_counter() - t))

    class Me(tc.Labels, la.LabelAudit, lt.LabelTrajectory):
        def __init__(self, s):
            tc.Labels.__init__(self, s, homography.Homography, homography.Homography_Wrapper)
    me = Me(scene)
    n_ids = me.get_unused_id()
    t_pack, pack = wall(lambda: lt.pack_objects(me, range(n_ids)))
    plan = lt.plan_fits(pack, 2, 3, 4, lt.tpe_x(), lt.tpe_y())
    lanes = sum(len(ch["s"]) for ch in plan["chunks"])
    say("pack_objects (host, one pass over data)           : %9.1f ms   (%d rows)" % (t_pack, len(pack["t"])))
    say("plan: %d (object, axis) groups, %d candidate fits, %d chunks of at most %d MiB of workspace, largest knot capacity %d"
        % (sum(len(ch["groups"]) for ch in plan["chunks"]), lanes, len(plan["chunks"]), lt.WORKSPACE_BYTES >> 20,
           max([0] + [ch["ncap"] for ch in plan["chunks"]])))
    # the launches, timed inside fit_objects' own sequence by wrapping the ops
    spent = {}

    def timed(name):
        real = getattr(ops, name)

        def call(*a, **k):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = real(*a, **k)
            stop.record()
            spent.setdefault(name, []).append((start, stop))
            return out
        setattr(ops, name, call)
        return real
    reals = {name: timed(name) for name in ("label_box_weights", "spline_fit", "spline_select", "spline_eval", "label_ts_shift")}
    t_fit, (results, kept, _) = wall(lambda: lt.fit_objects(me, range(n_ids), metric="mpe", keep=True))
    torch.cuda.synchronize()
    for name in ("label_box_weights", "spline_fit", "spline_select"):
        ms = [a.elapsed_time(b) for a, b in spent.get(name, [])]
        say("  %-22s %3d launches: %10.3f ms in all, longest %10.3f ms" % (name, len(ms), sum(ms), max(ms + [0.0])))
    iters = np.concatenate([ch["iters"][ch["ier"] != ops.SPLINE_UNUSED] for ch in kept]) if kept else np.zeros(1)
    ier = np.concatenate([ch["ier"] for ch in kept]) if kept else np.zeros(1)
    say("  longest lane: %d least-squares rounds + iterations on p (mean %.1f); lanes stopped at the knot limit: %d of %d; ier counts %s"
        % (iters.max(), iters.mean(), int((ier == ops.SPLINE_REJECTED).sum()), lanes,
           {int(e): int((ier == e).sum()) for e in np.unique(ier) if e <= 3}))
    say("fit_objects, every object, first call (pack + upload + launches + copy back, keeps every lane's t and c): %9.1f ms; %d of %d objects have splines"
        % (t_fit, sum(r is not None for r in results), n_ids))
    spent.clear()
    t_get, _ = wall(lambda: me.get_splines())
    say("get_splines (whole call)                          : %9.1f ms" % t_get)
    t_gen, _ = wall(lambda: me.gen_trajectories())
    ms = [a.elapsed_time(b) for a, b in spent.get("spline_eval", [])]
    say("gen_trajectories (whole call, mostly the deep copy of data): %9.1f ms   spline_eval %.3f ms" % (t_gen, sum(ms)))
    # the reference's frame loop stops at the first empty frame: time the pass on the longest run of populated frames
    full = [len(fd) > 0 for fd in scene["data"]] + [False]
    best, a = (0, 0), None
    for f, on in enumerate(full):
        if on and a is None:
            a = f
        if not on and a is not None:
            best, a = max(best, (f - a, a)), None
    n_run, a = best
    me2 = Me(scene)
    me2.data, me2.all_ts, me2.last_frame, me2.splines = me2.data[a:a + n_run], me2.all_ts[a:a + n_run], n_run, me.splines
    t_adj, rep = wall(lambda: me2.adjust_ts_with_trajectories(verbose=False))
    ms = [x.elapsed_time(y) for x, y in spent.get("label_ts_shift", [])]
    say("adjust_ts_with_trajectories (whole call, frames %d..%d: the longest run without an empty frame): %9.1f ms   label_ts_shift %.3f ms, "
        "%d (frame, camera) entries" % (a, a + n_run - 1, t_adj, sum(ms), len(rep)))
    spent.clear()
    t_box, shifts = wall(lambda: me2.adjust_boxes_with_trajectories())
    ms = [x.elapsed_time(y) for x, y in spent.get("label_box_weights", [])] + [x.elapsed_time(y) for x, y in spent.get("spline_eval", [])]
    say("adjust_boxes_with_trajectories (whole call, the same frames): %9.1f ms   its two launches %.3f ms, %d boxes moved" % (t_box, sum(ms), len(shifts)))
    for name, real in reals.items():
        setattr(ops, name, real)
    try:
        from scipy.interpolate import UnivariateSpline
    except ImportError:
        say("scipy is not importable here: the CPU loop of UnivariateSpline fits was not timed")
    else:
        warnings.simplefilter("ignore")
        ref = tc.Labels(scene)
        ids = [i for i, r in enumerate(results) if r is not None][:args.sample]
        t0, fits = time.perf_counter(), 0
        for i in ids:
            rows = tc.object_rows(ref, i)
            m = len(rows["t"])
            for v, w, k, tpes in ((rows["x"], rows["xw"], 3, tc.tpe_x()), (rows["y"], rows["yw"], 2, tc.tpe_y())):
                for tpe in tpes:
                    UnivariateSpline(rows["t"], v, k=k, w=w, s=tc.smoothing(tpe, m))
                    fits += 1
        dt = time.perf_counter() - t0
        if ids:
            say("scipy UnivariateSpline on the CPU, %d objects (%d fits, weights restated in numpy, no scoring): %.1f ms per object -> %.1f s for %d objects"
                % (len(ids), fits, dt / len(ids) * 1e3, dt / len(ids) * sum(r is not None for r in results), sum(r is not None for r in results)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

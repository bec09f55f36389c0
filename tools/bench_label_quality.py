#!/usr/bin/env python3
"""Time the label scores (label_quality.py / csrc/label_quality.hip) on a generated label set of the workload's own size -- 18
cameras x 2 700 frames x 300 objects by default -- against the plain restatement (tests/label_quality_cases.py) on the CPU of
the same machine, for the same scene.  The reference's own functions are NOT run: they need its checkout, which a machine
with the GPU need not have, so the host side of the comparison is the restatement, which makes one pass over the labels per
call where the reference makes objects x cameras x frames dict lookups.

Every figure is the median of repeated runs after a warm-up, with the smallest and the largest beside it.  Device times come
from HIP events around one launch; whole calls are host clocks around work that ends in a copy back.  Reported, not a gate.

    python tools/bench_label_quality.py [--cameras 18] [--frames 2700] [--objects 300] [--out profiles/label_quality.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tools"), os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)

import label_quality_cases as qc              # noqa: E402
import label_audit as la                      # noqa: E402
import label_quality as lq                    # noqa: E402
from bench_label_audit import big_scene       # noqa: E402
from datareader import _download, _upload     # noqa: E402
from retinanet_mi355x import ops              # noqa: E402


def spread(times):
    t = sorted(times)
    return "%9.3f ms  (min %.3f, max %.3f, n = %d)" % (t[len(t) // 2], t[0], t[-1], len(t))


def events(fn, reps):
    """Device time of every one of ``reps`` calls of fn() in ms (HIP events), after one warm-up call -> (times, last result)."""
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return times, out


def wall(fn, reps, warm=1):
    out, times = None, []
    for k in range(warm + reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = fn()
        torch.cuda.synchronize()
        if k >= warm:
            times.append((time.perf_counter() - t) * 1e3)
    return times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--frames", type=int, default=2700)
    ap.add_argument("--objects", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    t = time.perf_counter()
    scene = big_scene(args.cameras, args.frames, args.objects)
    scene["hg_old"] = qc.rc.hg_spec(scene["names"])
    names = scene["names"]
    boxes = sum(len(fd) for fd in scene["data"])
    say("label quality on %s: %d cameras, %d frames, %d objects, %d boxes (scene built in %.1f s)"
        % (torch.cuda.get_device_name(0), args.cameras, args.frames, args.objects, boxes, time.perf_counter() - t))

    class Me(qc.rc.Labels, lq.LabelQuality):
        pass
    me = Me(scene)

    # ---- the stages, apart
    t_pack, tab = wall(lambda: la.pack_tracklets(me.data, names), 3, warm=0)
    per_obj = np.diff(tab["offsets"][::args.cameras])
    say("rows per object: median %d, largest %d (sorted in LDS up to %d)" % (np.median(per_obj), per_obj.max(), ops.LABEL_SERIES_MAX_LDS_ROWS))
    say("pack_tracklets (host, one pass over data)            : " + spread(t_pack))
    t_up, (d_off, d_cols) = wall(lambda: _upload(dev, [tab["offsets"], tab["cols"]]), 5)
    say("upload, one copy (%.1f MB)                            : %s" % ((tab["cols"].nbytes + tab["offsets"].nbytes) / 1e6, spread(t_up)))
    say("device time of one launch (HIP events):")
    for what, fn in (("label_series, objects sorted in LDS", lambda: ops.label_series(d_off, d_cols, args.cameras)),
                     ("label_series, lane (82, 98)", lambda: ops.label_series(d_off, d_cols, args.cameras, (82, 98))),
                     ("label_series, lds_rows = 64: the global-memory sort", lambda: ops.label_series(d_off, d_cols, args.cameras, None, 64))):
        ms, out = events(fn, args.reps)
        ops.label_check(int(out[-1]))
        t_down, _ = wall(lambda: _download(list(out)), 5)
        say("  %-52s: %s" % (what, spread(ms)))
        say("  %-52s: %s" % ("  copy back", spread(t_down)))

    # ---- whole calls, and the restatement on the CPU for the same scene
    say("whole calls (pack + upload + launch + copy back + the host's lists) against the restatement on the CPU (the reference's own")
    say("functions are not run, they need its checkout; they would make %d x %d x %d dict lookups per function):" % (args.objects, args.cameras, args.frames))
    ref = qc.rc.Labels(scene)
    calls = (("calculate_total_variation", lambda: me.calculate_total_variation(), lambda: qc.ref_total_variation(ref), 5, 3),
             ("calculate_feasibility", lambda: me.calculate_feasibility(), lambda: qc.ref_feasibility(ref), 5, 3),
             ("quality_report (both, CCDE x / y)", lambda: me.quality_report(), None, 5, 0),
             ("annotator_rmse", lambda: me.annotator_rmse(), lambda: qc.ref_annotator_rmse(ref), 3, 1))
    for what, mine, theirs, reps, ref_reps in calls:
        t_mine, got = wall(mine, reps)
        say("  %-34s device path : %s" % (what, spread(t_mine)))
        if theirs is None:
            continue
        t_ref, want = wall(theirs, ref_reps, warm=0)
        if what == "annotator_rmse":
            same = all(abs(a - b) <= qc.rmse_bound(n, big) for a, b, n, big in zip(got[1], want[1], want[2], want[3]))
            same = "within the summation bound: %s" % same
        else:
            same = "same bytes: %s" % (np.array(got, np.float64).tobytes() == np.array(want, np.float64).tobytes())
        say("  %-34s restatement : %s   %s" % ("", spread(t_ref), same))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the label audit (label_audit.py / csrc/label_audit.hip) on a generated full-size label set -- 18 cameras x 3 600
frames x 300 objects by default -- against the plain restatement (tests/label_audit_cases.py) on the CPU of the same machine,
for the same scene.  Device times come from HIP events around the launches; packing (host) and the two copies are reported
apart.  Reported, not a gate.

    python tools/bench_label_audit.py [--cameras 18] [--frames 3600] [--objects 300] [--out profiles/label_audit.txt]
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
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)

import label_audit_cases as lc               # noqa: E402
import label_audit as la                     # noqa: E402
from datareader import _download, _upload    # noqa: E402
from retinanet_mi355x import ops             # noqa: E402


def big_scene(n_cam, n_frames, n_obj, seed=31):
    """Objects cross the whole road in about a third of the sequence; every camera sees 100 ft with 40 ft shared with its
    neighbour; 3 % of the boxes are missing and 0.5 % jump."""
    rng = np.random.RandomState(seed)
    s = lc.empty_scene(n_cam, n_frames, seed=seed)
    length = 60.0 * n_cam + 40.0
    for oid in range(n_obj):
        eb = oid % 2 == 0
        speed = length / (n_frames / 3.0) * rng.uniform(0.8, 1.25)
        f_in = int(rng.randint(0, max(1, 2 * n_frames // 3)))
        y = rng.uniform(10.0, 50.0) if eb else rng.uniform(70.0, 110.0)
        for c in range(n_cam):
            lo, hi = 60.0 * c - 15.0, 60.0 * c + 85.0
            for f in range(f_in, n_frames):
                x = -15.0 + speed * (f - f_in) if eb else length - 25.0 - speed * (f - f_in)
                if not lo <= x <= hi or rng.rand() < 0.03:
                    continue
                jump = 30.0 if rng.rand() < 0.005 else 0.0
                lc.put(s, f, c, oid, x + rng.normal(0, 0.3) + jump, y + rng.normal(0, 0.2), cls=oid)
    return s


def events(fn, reps):
    """Mean device time of fn() in ms (HIP events on the current stream), after one warm-up call."""
    out = fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps, out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--frames", type=int, default=3600)
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
    names = scene["names"]
    boxes = sum(len(fd) for fd in scene["data"])
    say("label audit on %s: %d cameras, %d frames, %d objects, %d boxes (scene built in %.1f s)"
        % (torch.cuda.get_device_name(0), args.cameras, args.frames, args.objects, boxes, time.perf_counter() - t))

    class Me(lc.Labels, la.LabelAudit):
        pass

    # ---- the stages, apart
    t_pack, tab = wall(lambda: la.pack_tracklets(scene["data"], names))
    table = lc.ts_table(scene["all_ts"], names)
    t_up, (d_off, d_cols, d_frame, d_ts) = wall(lambda: _upload(dev, [tab["offsets"], tab["cols"], tab["frame"], table]))
    track = np.repeat(np.arange(len(tab["offsets"]) - 1), np.diff(tab["offsets"]))
    gaps = int((np.diff(tab["frame"]) - 1)[track[1:] == track[:-1]].sum())
    n_visit = la.frames_visited(scene["data"], scene["last_frame"])
    say("pack_tracklets (host, one pass over data)       : %9.1f ms   (%d rows, %d tracklets)" % (t_pack, len(tab["cols"]), len(tab["offsets"]) - 1))
    say("upload, one copy (%.1f MB)                        : %9.3f ms" % ((tab["cols"].nbytes + tab["frame"].nbytes + tab["offsets"].nbytes + table.nbytes) / 1e6, t_up))
    say("device time of the launches (HIP events, mean of %d):" % args.reps)
    stages = (("label_pair_samples  key x, value t  (estimate_ts_bias)", lambda: ops.label_pair_samples(d_off, d_cols, args.cameras, 0, 2)),
              ("label_pair_samples  key x, value y  (est_y_error)", lambda: ops.label_pair_samples(d_off, d_cols, args.cameras, 0, 1)),
              ("label_pair_samples  key t, values x y (projection)", lambda: ops.label_pair_samples(d_off, d_cols, args.cameras, 2, 0, 1)),
              ("label_outliers", lambda: ops.label_outliers(d_off, d_cols, d_frame, args.frames, n_visit)),
              ("label_interpolate   %d missing frames" % gaps, lambda: ops.label_interpolate(d_off, d_cols, d_frame, d_ts, gaps)))
    for what, fn in stages:
        ms, out = events(fn, args.reps)
        ops.label_check(int(out[-1]))
        t_down, _ = wall(lambda: _download(list(out)))
        say("  %-58s: %9.3f ms   copy back %8.3f ms" % (what, ms, t_down))

    # ---- whole calls, and the restatement on the CPU for the same scene
    say("whole calls (pack + upload + launch + copy back + the host's lists / dict updates) against the restatement on the CPU:")
    calls = (("estimate_ts_bias", lambda m: m.estimate_ts_bias(), lambda m: lc.ref_ts_bias(m)),
             ("est_y_error", lambda m: m.est_y_error(), lambda m: lc.ref_y_error(m)),
             ("estimate_projection_error", lambda m: m.estimate_projection_error(), lambda m: lc.ref_projection_error(m)),
             ("estimate_projection_error(True)", lambda m: m.estimate_projection_error(True), lambda m: lc.ref_projection_error(m, True)),
             ("remove_outliers", lambda m: m.remove_outliers(), lambda m: lc.ref_outliers(m)),
             ("interpolate_all", lambda m: m.interpolate_all(), lambda m: lc.ref_interpolate(m)))
    say("  %-34s %12s %14s %8s" % ("method", "device path", "restatement", "ratio"))
    for what, mine, theirs in calls:
        a, b = Me(scene), lc.Labels(scene)
        t_mine, _ = wall(lambda: mine(a))
        t_ref, _ = wall(lambda: theirs(b))
        same = lc.dump(a.data, names)[1].tobytes() == lc.dump(b.data, names)[1].tobytes() and a.ts_bias.tobytes() == b.ts_bias.tobytes()
        say("  %-34s %9.1f ms %11.1f ms %7.1fx   same result: %s" % (what, t_mine, t_ref, t_ref / t_mine, same))
    say("(the restatement collects every tracklet once per call; the reference collects it again for every camera pair and object --")
    say(" %d x %d x %d dict lookups per estimator -- and is not run here)" % (args.cameras - 1, args.objects, 2 * args.frames))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

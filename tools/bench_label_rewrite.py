#!/usr/bin/env python3
"""Time the label re-basing (label_rewrite.py / csrc/label_rebase.hip) on the generated full-size label set of
tools/bench_label_audit.py -- 18 cameras x 3 600 frames x 300 objects by default, one box in ten manual -- against the numpy
restatement (tests/label_rewrite_cases.py) on the CPU of the same machine.  Device times come from HIP events around the
launches; the host's pass over the dicts and the copies are reported apart.  The launch of rn_label_rebase is set beside its
arithmetic floor: boxes x rounds x grid^2 candidates x 4 corners x the fp64 operations of one projection (18 multiplies and
adds, 2 divides counted as one operation each) at the FP64 vector rate.  Reported, not a gate.

    python tools/bench_label_rewrite.py [--cameras 18] [--frames 3600] [--objects 300] [--out profiles/label_rewrite.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

import label_audit_cases as lc               # noqa: E402
import label_rewrite_cases as rc             # noqa: E402
import label_audit as la                     # noqa: E402
import label_rewrite as lw                   # noqa: E402
import homography                            # noqa: E402
from bench_label_audit import big_scene, events, wall    # noqa: E402
from datareader import _download, _upload    # noqa: E402
from retinanet_mi355x import ops             # noqa: E402

# FP64 vector: half the FP32 vector rate (157.3 TFLOPS spec, an fma counted as two) -> 78.6 TFLOPS, i.e. 39.3e12 fp64
# instructions x lanes per second; without contraction every multiply and every add is an instruction of its own
FP64_OPS_PER_S = 157.3e12 / 2 / 2
OPS_PER_CORNER = 3 * 6 + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--objects", type=int, default=300)
    ap.add_argument("--manual", type=int, default=10, help="one box in this many is manual")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--restate", type=int, default=2000, help="boxes the restatement's search is timed on (scaled to all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    t = time.perf_counter()
    scene = big_scene(args.cameras, args.frames, args.objects)
    rng = np.random.RandomState(7)
    for fd in scene["data"]:
        for item in fd.values():
            item["gen"] = "Manual" if rng.randint(args.manual) == 0 else "Interpolation"
    names = scene["names"]
    scene["hg_old"], scene["hg_new"] = rc.hg_spec(names), rc.hg_spec(names, seed=41, scale=0.02)
    boxes = sum(len(fd) for fd in scene["data"])

    class Me(rc.Labels, la.LabelAudit, lw.LabelRewrite):
        def __init__(self, scene):
            rc.Labels.__init__(self, scene, homography.Homography, homography.Homography_Wrapper)
    new = rc.build_hg(scene["hg_new"], homography.Homography, homography.Homography_Wrapper)
    say("label re-basing on %s: %d cameras, %d frames, %d objects, %d boxes (scene built in %.1f s)"
        % (torch.cuda.get_device_name(0), args.cameras, args.frames, args.objects, boxes, time.perf_counter() - t))

    # ---- the stages of replace_homgraphy, apart
    me = Me(scene)
    t_visit, seen = wall(lambda: lw._visit(me, me.last_frame + 1))
    manual = [(f, k, o, c) for f, k, o, c in seen if o["gen"] == "Manual"]
    state = np.array([[float(o[k]) for k in rc.STATE_KEYS] for _, _, o, _ in manual], np.float64)
    cam = np.array([names.index(c) for _, _, _, c in manual], np.int32)
    radii = np.array(ops.label_rebase_radii(), np.float64)
    tables = rc.tables(me.hg, names) + rc.tables(new, names)
    t_up, up = wall(lambda: _upload(dev, [state, cam, radii] + tables))
    n, rounds, grid = len(state), len(radii), lw.GRID_SIZE
    say("the host's pass over the dicts (every box, in the reference's order): %9.1f ms   (%d manual boxes of %d)" % (t_visit, n, len(seen)))
    say("upload, one copy (%.2f MB)                                           : %9.3f ms" % ((state.nbytes + cam.nbytes) / 1e6, t_up))
    ms, out = events(lambda: ops.label_rebase(up[0], up[1], up[3], up[4], up[5], up[6], up[2], grid), args.reps)
    ops.label_check(int(out[-1]))
    t_down, _ = wall(lambda: _download(list(out)))
    work = n * rounds * grid * grid * 4 * OPS_PER_CORNER
    floor = work / FP64_OPS_PER_S * 1e3
    say("rn_label_rebase, %d boxes x %d rounds x %d candidates (HIP events, mean of %d): %9.3f ms   copy back %.3f ms"
        % (n, rounds, grid * grid, args.reps, ms, t_down))
    say("  arithmetic floor: %.3g fp64 operations of the projections (%d per corner) at %.1f T/s = %.3f ms; the launch is %.1fx that"
        % (work, OPS_PER_CORNER, FP64_OPS_PER_S / 1e12, floor, ms / floor))
    say("  (the floor counts a divide as one operation and leaves out the corner sums, the error and the reduction; 121 candidates")
    say("   fill 121 of the 128 lane slots of their two passes)")
    everything = [(f, k, o, c) for f, k, o, c in seen]
    xy = np.array([[o["x"], o["y"]] for _, _, o, _ in everything], np.float64)
    coef = np.array([me.poly_params[o["camera"] + ("_EB" if o["direction"] == 1 else "_WB")] for _, _, o, _ in everything], np.float64)
    d = np.array([o["direction"] for _, _, o, _ in everything], np.int32)
    up_y = _upload(dev, [xy, coef, np.full(len(xy), 72.0), d])
    ms, _ = events(lambda: ops.label_offset_y(up_y[0], up_y[1], up_y[2], up_y[3], False), args.reps)
    say("rn_label_offset_y, %d boxes (HIP events, mean of %d)                      : %9.3f ms" % (len(xy), args.reps, ms))

    # ---- whole calls, and the restatement on the CPU for the same scene
    say("whole calls (the pass over the dicts + upload + launch + copy back + deep copies + interpolate_all) against the numpy")
    say("restatement on the CPU:")
    sub = min(args.restate, n)
    t_search, _ = wall(lambda: rc.rebase_boxes(state[:sub], cam[:sub], *tables))
    say("  the restatement's search alone, %d boxes: %.1f ms -> %.1f s for all %d" % (sub, t_search, t_search / sub * n / 1e3, n))
    calls = (("replace_homgraphy", lambda m: m.replace_homgraphy(new), lambda m: rc.ref_replace_homgraphy(m, rc.build_hg(scene["hg_new"]))),
             ("replace_y", lambda m: m.replace_y(), lambda m: rc.ref_replace_y(m)),
             ("replace_y(reverse=True)", lambda m: m.replace_y(True), lambda m: rc.ref_replace_y(m, True)),
             ("replace_timestamps", lambda m: m.replace_timestamps(), lambda m: rc.ref_replace_timestamps(m)))
    say("  %-26s %12s %14s %8s" % ("method", "device path", "restatement", "ratio"))
    for what, mine, theirs in calls:
        a, b = Me(scene), rc.Labels(scene)
        t_mine, _ = wall(lambda: mine(a))
        t_ref, _ = wall(lambda: theirs(b))
        ia, va = lc.dump(a.data, names)
        ib, vb = lc.dump(b.data, names)
        say("  %-26s %9.1f ms %11.1f ms %7.1fx   same result: %s"
            % (what, t_mine, t_ref, t_ref / t_mine, ia.tobytes() == ib.tobytes() and va.tobytes() == vb.tobytes()))
    say("(the floor of every whole call is the host's pass over the dicts, the deep copies of the kept boxes and interpolate_all's")
    say(" own packing pass; the restatement forms every \"camera_id\" key of every frame as the reference does -- %d x %d x %d dict"
        % (args.cameras, args.objects, args.frames))
    say(" lookups -- and searches the candidates of a box with numpy arrays, not with three torch calls per box)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the calibration kernels on the device against their numpy restatement on the CPU (tests/calib_cases.py):
16 cameras x 3 axes of vanishing points in one launch, one scale_Z search (100 evaluations), one batch of 32 homography
fits.  Reported, not a gate.

    python tools/bench_calibrate.py [--out profiles/calibrate_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)

import calib_cases as cc                     # noqa: E402
from retinanet_mi355x import ops             # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cal = np.load(os.path.join(REPO, "tests", "golden", "calibration.npz"))
    lines = []

    def say(s):
        print(s)
        lines.append(s)
    say("calibration kernels on %s against the numpy restatement on the CPU" % torch.cuda.get_device_name(0))
    # 16 cameras x 3 axes, 2..8 lines per set
    sets = [cc.converging_lines(2 + (7 * k) % 7, (900.0 + 37 * k, -2000.0 + 91 * k), 900 + k) for k in range(48)]
    offsets = torch.from_numpy(np.cumsum([0] + [len(s) for s in sets]).astype(np.int64)).to(dev)
    flat = torch.from_numpy(np.concatenate(sets)).to(dev)
    t_dev = timed(lambda: ops.vanishing_points(flat, offsets), args.reps)
    t = time.perf_counter()
    want = [cc.vanishing_point(s) for s in sets]
    t_cpu = time.perf_counter() - t
    out = ops.vanishing_points(flat, offsets)[0].cpu().numpy()
    same = all(np.array_equal(out[i, :2], w["point"]) for i, w in enumerate(want))
    say("vanishing points, 48 sets (%d lines), one launch : %9.3f ms   restatement %9.1f ms   same bits: %s"
        % (len(flat), t_dev * 1e3, t_cpu * 1e3, same))
    # one scale_Z search
    for d in (17, 300):
        tag = "sz_d%d_" % d
        b, h, H, P0 = (cal[tag + k] for k in ("boxes", "heights", "H", "P0"))
        tb, th, tH, tP = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b, h, H, P0))
        t_dev = timed(lambda: ops.hg_scale_z(tb, th, tH, tP), args.reps)
        t = time.perf_counter()
        w = cc.scale_z(b, h, H, P0)
        t_cpu = time.perf_counter() - t
        got = ops.hg_scale_z(tb, th, tH, tP)[1].cpu().numpy()
        say("scale_Z, d = %3d, %d evaluations, one launch      : %9.3f ms   restatement %9.1f ms   same bits: %s"
            % (d, w["iters"] * 10, t_dev * 1e3, t_cpu * 1e3, got[0] == w["last_C"] and got[2] == w["best_error"]))
    # 16 cameras x (H, H_inv), 12 points each
    H = cal["sz_d17_H"]
    pairs = []
    for k in range(16):
        im, sp = cc.fit_case(12, H, 800 + k, noise=0.5)
        pairs += [(im, sp), (sp, im)]
    src = torch.from_numpy(np.concatenate([p[0] for p in pairs])).to(dev)
    dst = torch.from_numpy(np.concatenate([p[1] for p in pairs])).to(dev)
    off = torch.from_numpy(np.arange(33, dtype=np.int64) * 12).to(dev)
    t_dev = timed(lambda: ops.fit_homography(src, dst, off), args.reps)
    t = time.perf_counter()
    for s, d_ in pairs:
        cc.fit_homography(s, d_)
    t_cpu = time.perf_counter() - t
    say("homography fit, 32 problems of 12 points, one launch: %9.3f ms   restatement %9.1f ms" % (t_dev * 1e3, t_cpu * 1e3))
    say("(the reference's own find_vanishing_point takes 0.1-0.6 s per set on a CPU; its scale_Z makes 100 Python round trips)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

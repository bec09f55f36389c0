#!/usr/bin/env python3
"""Time fixed-interval smoothing on the scene of tools/bench_stitch.py (200 vehicles x 18 cameras: 3 600 fragments, 216 000 rows),
twice: unstitched (3 600 short lanes) and after ``stitch`` (200 long lanes, four waves).  Per case: each launch (device events
around ``reps`` launches after a warm-up), upload + launches + copy back, the whole ``smooth_tracks`` call with its host share,
and the numpy restatement of tests/smooth_cases.py on the same packed arrays on the CPU, whose bytes the device must reproduce.
The register and scratch figures of both kernels come from the compiler's resource-usage remark (``--resources`` compiles
csrc/smooth.hip once more for that; no GPU needed).  Reported, not a gate.

    python tools/bench_smooth.py [--vehicles 200] [--cameras 18] [--reps 20] [--out profiles/track_smooth.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

import smooth_cases as sc                    # noqa: E402
import track_smooth                          # noqa: E402
import track_stitch                          # noqa: E402
from bench_stitch import stretch             # noqa: E402
from retinanet_mi355x import ops             # noqa: E402


def resources():
    """The compiler's view of both kernels: {kernel: (VGPRs, AGPRs, scratch bytes per lane, waves per SIMD)}."""
    csrc = os.path.join(REPO, "3d-playground_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "smooth.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = "sm_filter_kernel" if "sm_filter_kernel" in m.group(1) else "sm_rts_kernel" if "sm_rts_kernel" in m.group(1) else None
            out.setdefault(name, {})
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return {k: v for k, v in out.items() if k}


def events(fn, reps):
    """Mean device time of one call in ms: events around ``reps`` calls, after one warm-up call."""
    out = fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def clock(fn, reps=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def kf_params():
    return {"Q": torch.from_numpy(sc.NOISY_Q.copy()), "R": torch.from_numpy(sc.NOISY_R.copy()), "P": torch.from_numpy(sc.NOISY_P0.copy())}


def case(name, data, dev, reps, say):
    params = track_smooth.resolve_params()
    kf = kf_params()
    model = ops.smooth_model(kf)
    t_pack, pk = clock(lambda: track_stitch.pack_tracklets(data))
    N, R = len(pk["ids"]), len(pk["cols"])
    n = np.diff(pk["offsets"])
    say("%s: %d lanes (%d waves), %d rows, %d .. %d rows per lane" % (name, N, -(-N // 64), R, n.min(), n.max()))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    args = [up(a) for a in (pk["offsets"], track_smooth.lane_order(pk["offsets"]), pk["cols"], pk["direction"], model)]
    t_f, (filt, nis, flag, st) = events(lambda: ops.smooth_filter(*args, params["gate"], params["dt_default"]), reps)
    t_r, (out, st2) = events(lambda: ops.smooth_rts(*args, params["dt_default"], filt), reps)
    say("  smooth_filter                    %9.3f ms   (%.1f ns per row, %d rows flagged)" % (t_f, t_f * 1e6 / R, int(flag.sum())))
    say("  smooth_rts                       %9.3f ms   (%.1f ns per row)" % (t_r, t_r * 1e6 / R))
    ident = [args[0], torch.arange(N, dtype=torch.int32, device=dev)] + args[2:]
    t_i, _ = events(lambda: ops.smooth_filter(*ident, params["gate"], params["dt_default"]), reps)
    say("  smooth_filter, identity order    %9.3f ms" % t_i)
    t_dev, host = clock(lambda: track_smooth.smooth_packed(pk["offsets"], pk["cols"], pk["direction"], model, params, dev), max(reps // 4, 1))
    t_build, _ = clock(lambda: track_smooth.rebuild(data, pk, host["out"]))
    t_all, (new_data, report) = clock(lambda: track_smooth.smooth_tracks(data, kf, device=dev))
    say("  upload, two launches, copy back  %9.1f ms" % (t_dev * 1e3))
    say("  smooth_tracks, whole call        %9.1f ms" % (t_all * 1e3))
    say("    host: pack_tracklets           %9.1f ms" % (t_pack * 1e3))
    say("    host: rebuild data             %9.1f ms" % (t_build * 1e3))
    say("    host share of the whole call   %9.1f %%" % (100.0 * (t_all - t_dev) / t_all))
    t0 = time.perf_counter()
    want = sc.smooth(pk["offsets"], pk["cols"], pk["direction"], model, params["gate"], params["dt_default"])
    t_cpu = time.perf_counter() - t0
    same = all(host[k].tobytes() == want[k].tobytes() for k in ("filt", "nis", "flag", "out")) and int(host["status"][0]) == want["status"] == 0
    say("  restatement (numpy, CPU)         %9.1f ms   = %.0f x the two launches; the device's bytes equal it: %s" %
        (t_cpu * 1e3, t_cpu * 1e3 / (t_f + t_r), same))
    return new_data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=200)
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resources", action="store_true", help="compile csrc/smooth.hip once more for the register and scratch figures")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    data = stretch(args.vehicles, args.cameras)
    say("%s, %d vehicles x %d cameras, %d frames" % (torch.cuda.get_device_name(0), args.vehicles, args.cameras, len(data)))
    if args.resources:
        for k, v in sorted(resources().items()):
            say("  %s: %d VGPRs, %d AGPRs, scratch %d bytes per lane, %d waves per SIMD" % (k, v["VGPRs"], v["AGPRs"], v["ScratchSize"], v["Occupancy"]))
    case("unstitched", data, dev, args.reps, say)
    stitched, report = track_stitch.stitch_tracks(data, device=dev)
    case("stitched (%d links)" % len(report["links"]), stitched, dev, args.reps, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

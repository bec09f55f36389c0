#!/usr/bin/env python3
"""Time track stitching on a generated 18-camera stretch: every vehicle changes its id at each camera hand-over, so a few
thousand fragments come out.  Each stage through its own op, the whole ``stitch_tracks`` call with its host shares (packing,
rebuilding ``data``), and the plain restatement of tests/stitch_cases.py (numpy + scipy on the CPU) in the same run.  Reported,
not a gate.

    python tools/bench_stitch.py [--vehicles 200] [--cameras 18] [--reps 5] [--out profiles/track_stitch.txt]
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

import stitch_cases as sc                    # noqa: E402
import track_stitch                          # noqa: E402
from retinanet_mi355x import ops             # noqa: E402


def clock(fn, reps=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def stretch(vehicles, cameras, seed=3):
    """``data`` as Data_Reader holds it: vehicles enter over ten minutes in eight lanes (four each way), drive at their own speed
    through ``cameras`` fields of view of 2 s each and are lost for 0.2 .. 1.5 s at every hand-over, where the id changes."""
    rng = np.random.RandomState(seed)
    frames, next_id = {}, 1
    for v in range(vehicles):
        sgn = 1 if v % 2 == 0 else -1
        y = sgn * (6.0 + 12.0 * rng.randint(0, 4)) + rng.randn() * 0.3
        speed, size = 80.0 + 40.0 * rng.rand(), (14.0 + 10.0 * rng.rand(), 6.0 + rng.rand(), 5.0 + rng.rand())
        j = int(rng.randint(0, 18000))
        x0 = 0.0 if sgn == 1 else 20000.0
        for _ in range(cameras):
            for jj in range(j, j + 60):
                ts = np.round(1623877000.0 + jj / 30.0, 4)
                x = x0 + sgn * speed * (jj - j) / 30.0 + rng.randn() * 0.3
                frames.setdefault(ts, {})[next_id] = {"timestamp": ts, "id": next_id, "class": "sedan", "x": x, "y": y + rng.randn() * 0.2,
                                                      "l": size[0], "w": size[1], "h": size[2], "direction": sgn, "v": speed,
                                                      "ts_bias": {"p1c1": 0.0}, "camera": "p1c1", "frame": str(jj)}
            lost = int(rng.randint(6, 46))
            x0 += sgn * speed * (60 + lost) / 30.0
            j += 60 + lost
            next_id += 1
    return [frames[ts] for ts in sorted(frames)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=200)
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    data = stretch(args.vehicles, args.cameras)
    params = track_stitch.resolve_params()
    scales = track_stitch.scales_of(params)
    t_pack, pk = clock(lambda: track_stitch.pack_tracklets(data))
    N, R = len(pk["ids"]), len(pk["cols"])
    cap, U = track_stitch.bounds(pk["offsets"], pk["direction"], params)
    say("%s, %d vehicles x %d cameras: %d fragments, %d rows, %d frames" % (torch.cuda.get_device_name(0), args.vehicles, args.cameras, N, R, len(data)))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    d_ids, d_off, d_cols, d_dir = up(pk["ids"]), up(pk["offsets"]), up(pk["cols"]), up(pk["direction"])
    track_stitch.stitch_packed(pk["ids"], pk["offsets"], pk["cols"], pk["direction"], params, True, dev)       # warm-up
    reps = args.reps
    t, (ep, st) = clock(lambda: ops.stitch_endpoints(d_off, d_cols, d_dir, params["fit_n"]), reps)
    say("  stitch_endpoints    %9.3f ms" % (t * 1e3))
    t, (cand, ncand) = clock(lambda: ops.stitch_candidates(ep, scales), reps)
    say("  stitch_candidates   %9.3f ms   (pass A over %d x %d pairs, compaction)" % (t * 1e3, N, N))
    t, (Wc, st) = clock(lambda: ops.stitch_compact(ep, scales, cand, ncand, cap), reps)
    n = ncand.cpu().tolist()
    say("  stitch_compact      %9.3f ms   (Wc %d x %d and %d x %d)" % (t * 1e3, n[0], n[1], n[2], n[3]))
    t, (nxt, prev, cost, st) = clock(lambda: ops.stitch_assign(ep, scales, cand, ncand, Wc), reps)
    say("  stitch_assign       %9.3f ms   (%d links)" % (t * 1e3, int((nxt >= 0).sum())))
    t, _ = clock(lambda: ops.stitch_chains(prev, d_ids), reps)
    say("  stitch_chains       %9.3f ms" % (t * 1e3))
    t, (count, prefix, st) = clock(lambda: ops.stitch_fill_count(ep, nxt, params["fill_rate"]), reps)
    say("  stitch_fill_count   %9.3f ms" % (t * 1e3))
    t, _ = clock(lambda: ops.stitch_fill_rows(ep, nxt, prefix, params["fill_rate"], U), reps)
    say("  stitch_fill_rows    %9.3f ms   (%d new rows, %d allocated)" % (t * 1e3, int(prefix[-1]), U))
    if N <= ops.STITCH_DENSE_MAX:
        t, _ = clock(lambda: ops.stitch_costs(ep, scales), reps)
        say("  stitch_costs        %9.3f ms   (the dense matrix, not on the product path)" % (t * 1e3))
    t_dev, host = clock(lambda: track_stitch.stitch_packed(pk["ids"], pk["offsets"], pk["cols"], pk["direction"], params, True, dev), reps)
    t_build, _ = clock(lambda: track_stitch.rebuild(data, pk, host, True))
    t_all, (new_data, report) = clock(lambda: track_stitch.stitch_tracks(data, device=dev))
    say("stitch_tracks, whole call          %9.1f ms" % (t_all * 1e3))
    say("  host: pack_tracklets             %9.1f ms" % (t_pack * 1e3))
    say("  upload, seven stages, copy back  %9.1f ms" % (t_dev * 1e3))
    say("  host: rebuild data               %9.1f ms" % (t_build * 1e3))
    say("  host: the rest, not attributed   %9.1f ms" % ((t_all - t_pack - t_dev - t_build) * 1e3))
    say("  host share of the whole call     %9.1f %%  -- the host's floor: dict work no kernel can take over" % (100.0 * (t_all - t_dev) / t_all))
    t0 = time.perf_counter()
    want = sc.run_all(pk["ids"], pk["offsets"], pk["cols"], pk["direction"])
    t_cpu = time.perf_counter() - t0
    say("restatement (numpy + scipy, CPU)   %9.1f ms   = %.1f x the device stages, %.2f x the whole call" %
        (t_cpu * 1e3, t_cpu / t_dev, (t_cpu + t_pack + t_build) / t_all))
    same = np.array_equal(want["next"], host["next"]) and want["fields"].tobytes() == host["fields"].tobytes()
    chains = len(set(report["root"].tolist()))
    say("links %d, chains %d (vehicles %d), same links and fill rows as the restatement: %s" % (len(report["links"]), chains, args.vehicles, same))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

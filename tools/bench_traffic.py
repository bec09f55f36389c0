#!/usr/bin/env python3
"""Time the traffic-state kernels on the scene of tools/bench_smooth.py (200 vehicles x 18 cameras: 3 600 fragments, 216 000 rows):
each launch (device events around ``reps`` launches after a warm-up), upload + launches + copy back, the whole ``traffic_fields``
and ``car_following`` calls with their host share, and the plain restatement of tests/traffic_cases.py on the same packed arrays on
the CPU, whose integers and bytes the device must reproduce.  Reported, not a gate.

    python tools/bench_traffic.py [--vehicles 200] [--cameras 18] [--reps 20] [--out profiles/traffic_state.txt]
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

import traffic_cases as tc                   # noqa: E402
import traffic_state                         # noqa: E402
import track_stitch                          # noqa: E402
from bench_smooth import clock, events       # noqa: E402
from bench_stitch import stretch             # noqa: E402
from retinanet_mi355x import ops             # noqa: E402

# the scene drives direction +1 at y = 6 .. 42 and direction -1 at y = -42 .. -6
PARAMS = {"lane_edges": {1: [0, 12, 24, 36, 48], -1: [-48, -36, -24, -12, 0]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=200)
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    data = stretch(args.vehicles, args.cameras)
    params = traffic_state.resolve_params(PARAMS)
    edges = {s: params["lane_edges"][s].tolist() for s in (1, -1)}
    t_pack, pk = clock(lambda: track_stitch.pack_tracklets(data))
    N, R = len(pk["ids"]), len(pk["cols"])
    grid = traffic_state.grid_of(pk["cols"], params)
    g = tuple(grid[k] for k in ("t0", "dt", "nt", "x0", "dx", "nx"))
    frame_off, frame_rows = traffic_state.frames_csr(pk["frame"], len(data))
    say("%s, %d vehicles x %d cameras: %d tracklets, %d rows, %d frames (at most %d rows), grid %d x %d cells of %g s x %g ft, %d lanes each way"
        % (torch.cuda.get_device_name(0), args.vehicles, args.cameras, N, R, len(data), int(np.diff(frame_off).max()), grid["nt"], grid["nx"],
           grid["dt"], grid["dx"], tc.n_lanes(edges)))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    d_off, d_cols, d_dir, d_ep, d_en, d_foff, d_frows = (up(a) for a in (pk["offsets"], pk["cols"], pk["direction"], params["lane_edges"][1],
                                                                         params["lane_edges"][-1], frame_off, frame_rows))
    t_l, (tdir, lane, st) = events(lambda: ops.traffic_lanes(d_off, d_cols, d_dir, d_ep, d_en), args.reps)
    t_c, cells = events(lambda: ops.traffic_cells(d_off, d_cols, tdir, d_ep, d_en, *g, params["max_gap"]), args.reps)
    t_f, lead = events(lambda: ops.traffic_leaders(d_off, d_cols, tdir, lane, d_foff, d_frows), args.reps)
    counters = dict(zip(ops.TRAFFIC_CELL_COUNTERS, cells[3].cpu().tolist()))
    say("  traffic_lanes                    %9.3f ms   (%.2f ns per row)" % (t_l, t_l * 1e6 / R))
    say("  traffic_cells                    %9.3f ms   (%.2f ns per segment; %d segments, %d pieces into %d occupied cells; the zeroing of T, D, n included)"
        % (t_c, t_c * 1e6 / counters["segments"], counters["segments"], counters["pieces"], int((cells[2] > 0).sum())))
    say("  traffic_leaders                  %9.3f ms   (%.2f ns per row; %d rows with a leader)" % (t_f, t_f * 1e6 / R, int(lead[5][0])))
    t_dev_f, host_f = clock(lambda: traffic_state.fields_packed(pk["offsets"], pk["cols"], pk["direction"], params, grid, dev), max(args.reps // 4, 1))
    t_dev_c, host_c = clock(lambda: traffic_state.following_packed(pk["offsets"], pk["cols"], pk["direction"], frame_off, frame_rows, params, dev),
                            max(args.reps // 4, 1))
    t_all_f, fields = clock(lambda: traffic_state.traffic_fields(data, PARAMS, dev))
    t_all_c, follow = clock(lambda: traffic_state.car_following(data, PARAMS, dev))
    say("  fields: upload, two launches, copy back     %9.1f ms" % (t_dev_f * 1e3))
    say("  following: upload, two launches, copy back  %9.1f ms" % (t_dev_c * 1e3))
    say("  traffic_fields, whole call                  %9.1f ms   (host: pack_tracklets %.1f ms)" % (t_all_f * 1e3, t_pack * 1e3))
    say("  car_following, whole call                   %9.1f ms" % (t_all_c * 1e3))
    t0 = time.perf_counter()
    w_dir, w_lane, w_status = tc.lanes(pk["offsets"], pk["cols"], pk["direction"], edges)
    t_cpu_l = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = tc.cells(pk["offsets"], pk["cols"], w_dir, edges, g, params["max_gap"])
    t_cpu_c = time.perf_counter() - t0
    t0 = time.perf_counter()
    w_lead = tc.leaders(pk["offsets"], pk["cols"], w_dir, w_lane, frame_off, frame_rows)
    t_cpu_f = time.perf_counter() - t0
    same_c = all(np.array_equal(fields[k], want[k]) for k in ("T", "D", "n")) and fields["counters"] == want["counters"] and w_status == want["status"] == 0
    same_f = all(follow[k].tobytes() == w_lead[k].tobytes() for k in ("leader", "spacing", "gap", "headway", "ttc")) \
        and np.array_equal(follow["lane"], w_lane) and np.array_equal(follow["dir"], w_dir) \
        and (follow["with_leader"], follow["overlaps"]) == (w_lead["with_leader"], w_lead["overlaps"])
    say("  restatement (Python, CPU): lanes %.0f ms, cells %.0f ms = %.0f x the launch, leaders %.0f ms = %.0f x the launch"
        % (t_cpu_l * 1e3, t_cpu_c * 1e3, t_cpu_c * 1e3 / t_c, t_cpu_f * 1e3, t_cpu_f * 1e3 / t_f))
    say("  the device's fields equal the restatement's integers: %s; its leaders and gaps equal it byte for byte: %s" % (same_c, same_f))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same_c and same_f else 1


if __name__ == "__main__":
    sys.exit(main())

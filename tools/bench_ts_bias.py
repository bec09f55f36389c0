"""estimate_ts_bias (csrc/ts_bias.hip) through the drop-in mc3d_track.estimate_ts_bias at d = 50 / 200 / 1000
detections from 4 cameras with ~5 % cross-camera duplicates, beside the numpy restatement of the reference's method on
the host (tests/ts_bias_cases.py; the reference itself adds one .item() round trip per pair of detections on top).
Medians over 50 calls after 10 warm-up calls (the host column: 30 calls after 3).  "stream (ev)": HIP events around
ops.estimate_ts_bias (no copy) -- the stream's timeline from the first launch to the end of the fifth kernel, which
includes the host's pacing of the five launches, so it is an upper bound on kernel time, not kernel time (per-kernel
durations: a rocprofv3 --kernel-trace --stats run of this script, profiles/ts_bias_kernel_stats.csv).  "drop-in (wall)":
wall clock around the whole drop-in call including its upload and its one device -> host copy.  Microseconds per call.
    python tools/bench_ts_bias.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)
import mc3d_track                                    # noqa: E402
import ts_bias_cases as tb                           # noqa: E402
from retinanet_mi355x import ops, synth              # noqa: E402

CALLS, WARMUP, N_CAM = 50, 10, 4
HOST_CALLS, HOST_WARMUP = 30, 3


def scene(d, seed):
    k = int(round(d / 1.05))
    v = synth.vehicle_states(k, seed=seed).numpy()
    v[:, 0] = 100.0 + 70.0 * np.arange(k)                                   # no chance overlaps: 70 ft apart per lane
    w = v[:d - k].copy()
    w[:, 0] += synth.uniform((d - k,), seed + 1, -1.5, 1.5)
    boxes = np.concatenate((v, w)).astype(np.float32)
    cams = np.concatenate((np.arange(k) % N_CAM, (np.arange(d - k) + 1) % N_CAM)).astype(np.int64)
    perm = np.argsort(synth.uniform((d,), seed + 2), kind="stable")
    objs = np.zeros((40, 7), np.float32)
    objs[:, :6] = synth.vehicle_states(40, seed=seed + 3).numpy()
    objs[:, 6] = synth.uniform((40,), seed + 4, 60, 100)
    return dict(boxes=boxes[perm], cams=cams[perm], objs=objs, timestamps=[1000.0 + 0.004 * c for c in range(N_CAM)],
                ts_bias=[0.0, 0.01, -0.02, 0.005], phi=tb.PHI)


class View:
    def __init__(self, objs):
        self.objs, self.mu_v, self.device = objs, torch.tensor(tb.MU_V), objs.device

    def view(self, dt=None, with_direction=False):
        return list(range(len(self.objs))), self.objs


def main():
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    print("estimate_ts_bias on %s (%s, %d CUs), %d cameras, medians of %d calls (host: %d), us per call"
          % (prop.name, prop.gcnArchName, prop.multi_processor_count, N_CAM, CALLS, HOST_CALLS))
    print("%6s %6s | %12s %14s | %14s" % ("d", "pairs", "stream (ev)", "drop-in (wall)", "numpy restated"))
    for d in (50, 200, 1000):
        c = scene(d, 800 + d)
        r = tb.restated(**c)
        boxes, cams, objs = (torch.from_numpy(c[k]).to(dev) for k in ("boxes", "cams", "objs"))
        ts = torch.tensor(c["timestamps"], dtype=torch.float64, device=dev)
        me = mc3d_track.TrackManager()
        me.filter, me.phi_nms_space, me.ts_alpha = View(objs), tb.PHI, tb.ALPHA
        me.timestamps = list(c["timestamps"])
        ev, wall, host = [], [], []
        for it in range(WARMUP + CALLS):
            bias = torch.tensor(c["ts_bias"], dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.estimate_ts_bias(boxes, cams, objs, ts, bias, tb.PHI, tb.ALPHA, tb.MU_V)
            b.record()
            torch.cuda.synchronize()
            me.ts_bias = list(c["ts_bias"])
            t0 = time.perf_counter()
            me.estimate_ts_bias(boxes, cams)
            t1 = time.perf_counter()
            if it == WARMUP:
                assert me.ts_bias == r["ts_bias"] or np.allclose(me.ts_bias, r["ts_bias"], rtol=0, atol=1e-6)
            if it >= WARMUP:
                ev.append(a.elapsed_time(b) * 1e3)
                wall.append((t1 - t0) * 1e6)
        for it in range(HOST_WARMUP + HOST_CALLS):
            t0 = time.perf_counter()
            tb.restated(**c)
            if it >= HOST_WARMUP:
                host.append((time.perf_counter() - t0) * 1e6)
        print("%6d %6d | %12.1f %14.1f | %14.1f" % (d, len(r["entries"]) // 2, statistics.median(ev), statistics.median(wall),
                                                    statistics.median(host)))


if __name__ == "__main__":
    main()

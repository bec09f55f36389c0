"""Track association (csrc/track_assoc.hip): cost + assignment + gate on the GPU at tracks x detections = 100x120,
400x450, 1000x1200 on IoU-like costs of a road-plane scene, timed with HIP events, beside the reference's path:
device -> host copies of both state arrays, the fp64 cost on the CPU (oracle/homography.py footprints, md_iou's
expression in torch), scipy.optimize.linear_sum_assignment if importable.  Microseconds per call.
    python tools/bench_track.py"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d-playground_amd"))
sys.path.insert(0, REPO)
from oracle import homography as ohg                 # noqa: E402
from retinanet_mi355x import ops, synth              # noqa: E402


def scene(n, m, seed):
    """n tracks ([n,7], direction at column 5) and m detections ([m,6]): the first min(n,m) detections are the tracks a
    little further on, the rest new vehicles; everything on a 1.1 km stretch of road."""
    pre = synth.vehicle_states(n, seed=seed).numpy()
    pre = np.concatenate([pre, synth.uniform((n, 1), seed + 9, 60, 100)], axis=1).astype(np.float32)
    k = min(n, m)
    det = np.concatenate([pre[:k, :6], synth.vehicle_states(m - k, seed=seed + 20).numpy()]).astype(np.float32)
    det[:k, 0] += synth.uniform((k,), seed + 30, -3.0, 3.0)
    det[:k, 1] += synth.uniform((k,), seed + 31, -0.6, 0.6)
    return torch.from_numpy(pre), torch.from_numpy(det)


def cpu_cost(pre, det):
    def env(s):
        sp = torch.from_numpy(ohg.state_to_space(s[:, :6].numpy()))
        return torch.stack((sp[:, 0:4, 0].min(1).values, sp[:, 0:4, 1].min(1).values,
                            sp[:, 0:4, 0].max(1).values, sp[:, 0:4, 1].max(1).values), dim=1).float()
    a, b = env(pre), env(det)
    f, s = a.shape[0], b.shape[0]
    a = a.unsqueeze(1).repeat(1, s, 1).double()
    b = b.unsqueeze(0).repeat(f, 1, 1).double()
    area_a = (a[:, :, 2] - a[:, :, 0]) * (a[:, :, 3] - a[:, :, 1])
    area_b = (b[:, :, 2] - b[:, :, 0]) * (b[:, :, 3] - b[:, :, 1])
    zeros = torch.zeros(area_a.shape, dtype=torch.float64)
    inter = torch.max(zeros, torch.min(a[:, :, 2], b[:, :, 2]) - torch.max(a[:, :, 0], b[:, :, 0])) * \
        torch.max(zeros, torch.min(a[:, :, 3], b[:, :, 3]) - torch.max(a[:, :, 1], b[:, :, 1]))
    return 1.0 - inter / (area_a + area_b - inter)


def main():
    dev = torch.device("cuda:0")
    try:
        from scipy.optimize import linear_sum_assignment as lsa
    except ImportError:
        lsa = None
    print("track association: cost + assignment + gate (phi_match 0.1), us per call")
    for n, m in ((100, 120), (400, 450), (1000, 1200)):
        pre, det = scene(n, m, seed=700 + n)
        pd, dd = pre.to(dev), det.to(dev)

        def gpu():
            return ops.match(ops.track_cost(pd, dd), 0.9, info=True)
        for _ in range(3):
            gpu()
        torch.cuda.synchronize()
        it = 20 if n < 1000 else 5
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(it):
            rm, info = gpu()
        e1.record()
        torch.cuda.synchronize()
        g_us = e0.elapsed_time(e1) / it * 1e3
        c0 = torch.cuda.Event(enable_timing=True)
        c1 = torch.cuda.Event(enable_timing=True)
        cost = ops.track_cost(pd, dd)
        c0.record()
        for _ in range(it):
            ops.track_cost(pd, dd)
        c1.record()
        torch.cuda.synchronize()
        cost_us = c0.elapsed_time(c1) / it * 1e3
        k = int(info[0])
        # the reference's path: copies, fp64 cost on the CPU, scipy
        t0 = time.perf_counter()
        ph, dh = pd.cpu(), dd.cpu()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        cc = cpu_cost(ph, dh)
        t_cost = time.perf_counter() - t0
        same = bool(torch.equal(cc, cost.cpu()))
        line = ("%4d x %4d  GPU cost+solve+gate %9.1f us (cost alone %6.1f)  matched %4d | reference path: copies %7.1f us, "
                "CPU fp64 cost %9.1f us (bit-equal to the kernel's: %s)" % (n, m, g_us, cost_us, k, t_copy * 1e6, t_cost * 1e6, same))
        if lsa is not None:
            t0 = time.perf_counter()
            r, c = lsa(cc.numpy())
            t_lsa = time.perf_counter() - t0
            got = rm.cpu().numpy()
            keep = cc.numpy()[r, c] <= 0.9
            ref = np.full(n, -1)
            ref[r[keep]] = c[keep]
            line += ", scipy %9.1f us (same matching: %s)" % (t_lsa * 1e6, bool(np.array_equal(ref, got)))
        else:
            line += ", scipy not installed"
        print(line, flush=True)


if __name__ == "__main__":
    main()

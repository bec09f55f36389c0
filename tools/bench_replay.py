"""The tracking-CSV replay (3d-playground_amd/datareader.py: plot_in; mc3d_render.Replayer; csrc/replay.hip) at the reference's
own call and at the deployment size: 6 and 18 cameras of 1080x1920, 40 objects per label instant drawn in every camera with
their five label lines, the mosaic written at 3840x2160.

    python tools/bench_replay.py [--cams 6 18] [--objects 40] [--iters 50]

Times ``replay_boxes``, the paint half (mask clear, edges, rectangles, text) and ``replay_compose`` separately with device
events, and a whole replayed frame (``Replayer.replay``: the one upload included) with a host clock around a synchronised
window.  The compose pass is priced against its byte floor: n_cam * H * W * 5 B read (3 B of frame, 2 B of mask) plus
OW * OH * 3 B written, over the 6.29 TB/s a device copy reaches on this GPU.  Needs the GPU: there is no CPU
path to time."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "3d-playground_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_TBS = 6.29                  # measured device copy rate, BASELINE.md


def scene(n_cam, H, W, objects, seed=0):
    """States on a road of 1600 x 120 ft and one top-down camera matrix per camera that puts every one of them on its frame:
    the most the painters can be asked for."""
    rs = np.random.RandomState(seed)
    st = np.stack((rs.uniform(100, 1500, objects), rs.uniform(10, 110, objects), rs.uniform(14, 60, objects), rs.uniform(5.5, 8.5, objects),
                   rs.uniform(4, 12, objects), rs.choice([-1.0, 1.0], objects), rs.uniform(60, 120, objects)), 1).astype(np.float32)
    P = np.zeros((n_cam, 3, 4))
    for c in range(n_cam):
        P[c] = [[1.1, 0.0, 0.0, 60.0 + c], [0.0, 7.5, -6.0, 80.0], [0.0, 0.0, 0.0, 1.0]]
    dts = rs.uniform(-0.02, 0.02, n_cam)
    return st, P, dts


def run(n_cam, H, W, objects, size, warmup, iters, dev):
    from mc3d_render import Replayer, replay_label_lines
    from retinanet_mi355x import ops
    st, P, dts = scene(n_cam, H, W, objects)
    frames = torch.randint(0, 256, (n_cam, H, W, 3), dtype=torch.uint8, device=dev)
    d_st, d_P = torch.from_numpy(st).to(dev), torch.from_numpy(P).to(dev)
    r = Replayer(n_cam, H, W, dev)
    lines = [[replay_label_lines(st[i], "sedan", 1000 + i, 1623877000.1234 + dt) for i in range(objects)] for dt in dts]
    rects, runs, text = r.records(lines)
    d_dt, d_rects, d_runs, d_text = r._upload(dts, rects, runs, text)
    out = torch.empty((size[1], size[0], 3), dtype=torch.uint8, device=dev)

    def events(k):
        return [torch.cuda.Event(enable_timing=True) for _ in range(k)]
    boxes_ms, paint_ms, compose_ms = [], [], []
    for it in range(warmup + iters):
        e0, e1, e2, e3 = events(4)
        e0.record()
        views, corners, side, cam = ops.replay_boxes(d_st, d_dt, d_P, None, 0, objects)
        e1.record()
        r.paint(corners, side, cam, d_rects, d_runs, d_text)
        e2.record()
        ops.replay_compose(frames, r.mask, size, out=out)
        e3.record()
        torch.cuda.synchronize()
        if it >= warmup:
            boxes_ms.append(e0.elapsed_time(e1))
            paint_ms.append(e1.elapsed_time(e2))
            compose_ms.append(e2.elapsed_time(e3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        canvas = r.replay(frames, d_st, 0, objects, dts, d_P, None, lines, size)
    torch.cuda.synchronize()
    whole_ms = (time.perf_counter() - t0) * 1e3 / iters
    assert torch.equal(canvas, out) and torch.equal(canvas, r.replay(frames, d_st, 0, objects, dts, d_P, None, lines, size))
    covered = float((r.mask.cpu().numpy() != 0).mean())
    floor_bytes = n_cam * H * W * 5 + size[0] * size[1] * 3
    floor_us = floor_bytes / (COPY_TBS * 1e12) * 1e6
    med = lambda v: float(np.median(v)) * 1e3                                                # noqa: E731  (us)
    print("bench_replay: %d cameras of %dx%d (canvas %dx%d), %d objects in every camera (%d boxes, 5 label lines each) -> %dx%d"
          % (n_cam, H, W, r.cols * W, r.rows * H, objects, n_cam * objects, size[0], size[1]))
    print("  %.2f%% of the mask pixels painted, %d iterations after %d warm-up" % (100 * covered, iters, warmup))
    print("  boxes   (rn_replay_boxes),                device events: median %8.1f us  (min %8.1f)" % (med(boxes_ms), min(boxes_ms) * 1e3))
    print("  paint   (clear + edges + rects + text),   device events: median %8.1f us  (min %8.1f)" % (med(paint_ms), min(paint_ms) * 1e3))
    print("  compose (rn_replay_compose),              device events: median %8.1f us  (min %8.1f)" % (med(compose_ms), min(compose_ms) * 1e3))
    print("    byte floor n_cam*H*W*5 B + OW*OH*3 B = %.1f MB over %.2f TB/s (measured copy rate): %.1f us -> compose runs at %.0f%% of it"
          % (floor_bytes / 1e6, COPY_TBS, floor_us, 100 * floor_us / med(compose_ms)))
    print("  whole Replayer.replay call (one upload), host clock over %d synchronised calls: %.3f ms per frame" % (iters, whole_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, nargs="+", default=[6, 18])
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--size", type=int, nargs=2, default=[3840, 2160])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_replay needs the GPU: there is nothing to time without one")
    print(torch.cuda.get_device_name(0))
    for n in a.cams:
        run(n, a.height, a.width, a.objects, tuple(a.size), a.warmup, a.iters, torch.device("cuda:0"))


if __name__ == "__main__":
    main()

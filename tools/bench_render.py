"""Output frames of the tracker (3d-playground_amd/mc3d_render.py, csrc/render.hip) at the deployment size: 18 cameras of
1080x1920, 100 tracks drawn in every camera with five label lines each, 60 detections, 50 crop windows, the banner.

    python tools/bench_render.py [--cams 18] [--tracks 100] [--iters 50]

Times the paint half (mask clear, edges, rectangles, text, the one upload) and the compose pass separately with device
events, and the whole ``Renderer.render`` call with a host clock around a synchronised window.  The compose pass is priced
against its byte floor: n_cam * H * W * 17 B (12 B of frame, 2 B of mask, 3 B out) over the 6.29 TB/s a device copy reaches
on this GPU.  The whole render is set beside the tracker's own 1.79 ms per frame (profiles/tracker_run.txt).
Needs the GPU: there is no CPU path to time."""
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
TRACKER_MS = 1.79                # profiles/tracker_run.txt: the tracker's own work per frame, 18 cameras


def scene(n_cam, H, W, tracks, dets, crops, label_len, dev, seed=0):
    """Every track in every camera (as plot() draws them), all of them on the frame: the most the painters can be asked for."""
    rs = np.random.RandomState(seed)

    def boxes(k, cams):
        # a vehicle about 160 x 70 pixels: the base rectangle and the same one 40 pixels up, as a 3D box projects
        c = np.stack((rs.uniform(100, W - 100, k), rs.uniform(100, H - 100, k)), 1)
        base = np.array([[-80, 35], [80, 35], [-60, 5], [100, 5]], np.float64)
        box = np.concatenate((base, base - [0, 40]))[None] + c[:, None, :] + rs.uniform(-4, 4, (k, 8, 2))
        return torch.from_numpy(box).to(dev), torch.from_numpy(cams.astype(np.int32)).to(dev)
    all_cams = np.repeat(np.arange(n_cam), tracks)
    tr = boxes(n_cam * tracks, all_cams)
    lines = ["sedan 1234:", "61.4mph EB", "L: 16.2ft", "W: 6.4ft", "H: 4.6ft"][:label_len]
    labels = [(i, int(all_cams[i]), lines) for i in range(n_cam * tracks)]
    de = boxes(dets, rs.randint(0, n_cam, dets))
    x0, y0 = rs.uniform(0, W - 260, crops), rs.uniform(0, H - 260, crops)
    side = rs.uniform(120, 260, crops)
    cr = (torch.from_numpy(np.stack((x0, y0, x0 + side, y0 + side), 1)).to(dev), torch.from_numpy(rs.randint(0, n_cam, crops)).to(dev))
    banners = ["Estimated time bias: %.4fs (%.1fft)" % (0.001 * c, 0.08 * c) for c in range(n_cam)]
    return dict(tracks=tr, detections=de, priors=None, crops=cr, labels=labels, banners=banners)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=18)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--tracks", type=int, default=100)
    ap.add_argument("--dets", type=int, default=60)
    ap.add_argument("--crops", type=int, default=50)
    ap.add_argument("--label-len", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_render needs the GPU: there is nothing to time without one")
    from mc3d_render import Renderer
    from retinanet_mi355x import ops
    dev = torch.device("cuda:0")
    n, H, W = a.cams, a.height, a.width
    frames = torch.randn((n, 3, H, W), device=dev)
    sc = scene(n, H, W, a.tracks, a.dets, a.crops, a.label_len, dev)
    r = Renderer(n, H, W, dev)
    out = torch.empty((r.rows * H, r.cols * W, 3), dtype=torch.uint8, device=dev)

    def events(k):
        return [torch.cuda.Event(enable_timing=True) for _ in range(k)]
    paint_ms, compose_ms = [], []
    for it in range(a.warmup + a.iters):
        e0, e1, e2 = events(3)
        e0.record()
        present = r.paint(**sc)
        e1.record()
        ops.render_compose(frames, r.mask, present, r.cols, out=out)
        e2.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            paint_ms.append(e0.elapsed_time(e1))
            compose_ms.append(e1.elapsed_time(e2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        canvas = r.render(frames, **sc)
    torch.cuda.synchronize()
    whole_ms = (time.perf_counter() - t0) * 1e3 / a.iters
    first = r.render(frames, **sc).clone()
    assert torch.equal(first, r.render(frames, **sc)) and torch.equal(first, out)          # the same bytes every time

    covered = float((r.mask.cpu().numpy() != 0).mean())
    floor_us = n * H * W * 17 / (COPY_TBS * 1e12) * 1e6
    med = lambda v: float(np.median(v))                                                     # noqa: E731
    print("bench_render: %d cameras of %dx%d, %d tracks in every camera (%d boxes, %d label lines each), %d detections, %d crops"
          % (n, H, W, a.tracks, n * a.tracks, a.label_len, a.dets, a.crops))
    print(torch.cuda.get_device_name(0))
    print("  canvas %dx%d uint8 RGB (%.1f MB), %.2f%% of the mask pixels painted, %d iterations after %d warm-up"
          % (canvas.shape[0], canvas.shape[1], canvas.numel() / 1e6, 100 * covered, a.iters, a.warmup))
    print("  paint   (clear + edges + rects + text + upload), device events: median %8.1f us  (min %8.1f)"
          % (med(paint_ms) * 1e3, min(paint_ms) * 1e3))
    print("  compose (rn_render_compose),                     device events: median %8.1f us  (min %8.1f)"
          % (med(compose_ms) * 1e3, min(compose_ms) * 1e3))
    print("    byte floor n_cam*H*W*17 B = %.1f MB over %.2f TB/s (measured copy rate): %.1f us -> compose runs at %.0f%% of it (%.2f TB/s)"
          % (n * H * W * 17 / 1e6, COPY_TBS, floor_us, 100 * floor_us / (med(compose_ms) * 1e3),
             n * H * W * 17 / (med(compose_ms) * 1e-3) / 1e12))
    print("  whole Renderer.render call, host clock over %d synchronised calls: %.3f ms per frame" % (a.iters, whole_ms))
    print("    beside the tracker's own %.2f ms per frame (profiles/tracker_run.txt): + %.0f%%" % (TRACKER_MS, 100 * whole_ms / TRACKER_MS))


if __name__ == "__main__":
    main()

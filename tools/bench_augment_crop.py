#!/usr/bin/env python3
"""Crop-detector training batches at the trainer's size: a batch of 12 x 1080p, CROP = 112.

Split into the host draws (``draw_crop`` and ``pack_crop_params``: labels, records, tables), the packed upload, and the device
chain (``ops.augment_crops`` alone, everything already on the device: five launches, timed with events over 2000 repeats after 3
warm-up calls), and ``augment.augment_crop_batch`` end to end.  Beside it the reference's chain for the same records on one host
thread through Pillow, where it is installed.  No speed is asserted.
    python tools/bench_augment_crop.py
    python tools/bench_augment_crop.py --device-only 200      # the device chain alone, 200 times: for a kernel trace"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d-playground_amd"))
from retinanet_mi355x import augment, ops   # noqa: E402

VPS = [[-310.5, 12.25], [2100.75, -55.5], [48.0, 3000.5]]


def host_chain(frame, p):
    """One image through the reference's crop chain on the CPU with Pillow -> milliseconds, or None without Pillow."""
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return None
    H, W = frame.shape[:2]
    t0 = time.perf_counter()
    im = Image.fromarray(frame).resize((p["rw"], p["rh"]), Image.BILINEAR)
    t = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div(255)
    new = torch.rand([3, H, W])
    h, w = min(t.shape[1], H), min(t.shape[2], W)
    new[:, :h, :w] = t[:, :h, :w]
    im = Image.fromarray(new.mul(255).byte().permute(1, 2, 0).contiguous().numpy())
    if p["flip"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    im = im.rotate(p["angle"], Image.BILINEAR)
    x, y, w, h = p["win"]
    im = im.crop((x, y, x + w, y + h)).resize((p["crop"], p["crop"]), Image.BILINEAR)
    if p["apply"]:
        for op in p["order"]:
            if op < 3:
                im = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(p["factors"][op])
    t = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div(255)
    t = (t - torch.tensor(ops.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(ops.IMAGENET_STD).view(3, 1, 1)
    return (time.perf_counter() - t0) * 1e3


def main():
    dev = torch.device("cuda:0")
    B, H, W, cs = 12, 1080, 1920, 112
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    labels = []
    for _ in range(B):                                         # ten boxes of 60 .. 400 pixels per frame
        c = rng.uniform([300, 250], [1600, 800], size=(10, 1, 2))
        pts = c + rng.uniform(-1, 1, size=(10, 8, 2)) * rng.uniform(30, 200, size=(10, 1, 1))
        box = np.concatenate([pts.min(1), pts.max(1)], 1)
        labels.append(torch.from_numpy(np.concatenate([pts.reshape(10, 16), box, np.ones((10, 1))], 1)))

    def draws():
        np.random.seed(0)
        torch.manual_seed(0)
        return [augment.draw_crop(labels[i], "p1c1", VPS, (W, H), cs)[0] for i in range(B)]
    drawn = draws()
    t0 = time.perf_counter()
    for _ in range(5):
        packed = augment.pack_crop_params(draws(), W, H, cs)
    ms_host = (time.perf_counter() - t0) / 5 * 1e3
    for p in drawn:
        p["apply"] = 1                                        # time the longer path: jitter applied on every image
    rec, tx, ty, cx, cy, K, win_max = augment.pack_crop_params(drawn, W, H, cs)
    wins = [p["win"][2:] for p in drawn]
    print("B = %d x %dx%d, CROP = %d; windows %s; K = %d taps, win_max = %d" % (B, H, W, cs, wins, K, win_max), flush=True)
    print("host draws, labels, records and tables: %.2f ms per batch" % ms_host, flush=True)
    host = torch.from_numpy(frames).pin_memory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        f = host.to(dev, non_blocking=True)
        torch.cuda.synchronize()
    print("upload of the frames (%.1f MB, pinned): %.2f ms per batch" % (frames.nbytes / 1e6, (time.perf_counter() - t0) / 5 * 1e3), flush=True)
    params = (torch.from_numpy(rec.view(np.uint8).reshape(B, -1)).to(dev),) + tuple(torch.from_numpy(t).to(dev) for t in (tx, ty, cx, cy))
    for _ in range(3):
        ops.augment_crops(f, params, K, win_max, cs, seed=1)
    torch.cuda.synchronize()
    if "--device-only" in sys.argv:
        for _ in range(int(sys.argv[sys.argv.index("--device-only") + 1])):
            ops.augment_crops(f, params, K, win_max, cs, seed=1)
        torch.cuda.synchronize()
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(2000):
        ops.augment_crops(f, params, K, win_max, cs, seed=1)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 2000
    print("device chain (five launches; includes the output and workspace allocations): %.3f ms per batch, %.3f ms per image"
          % (ms, ms / B), flush=True)
    for _ in range(2):
        augment.augment_crop_batch(list(frames), labels, ["p1c1"] * B, [VPS] * B, cs, dev, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        augment.augment_crop_batch(list(frames), labels, ["p1c1"] * B, [VPS] * B, cs, dev, seed=1)
    torch.cuda.synchronize()
    ms_all = (time.perf_counter() - t0) / 5 * 1e3
    print("end to end (draws, labels, tables, stacking, one packed upload, device chain): %.2f ms per batch, %.2f ms per image"
          % (ms_all, ms_all / B), flush=True)
    host_chain(frames[0], drawn[0])
    times = [host_chain(frames[i], drawn[i]) for i in range(B)]
    if times[0] is None:
        print("the same chain on the host through Pillow: not measured (Pillow is not installed)", flush=True)
    else:
        print("the same chain on the host (Pillow, one thread of %d CPUs, as the reference's DataLoader(workers 0)): %.1f ms per batch, "
              "%.1f ms per image" % (len(os.sched_getaffinity(0)), sum(times), sum(times) / B), flush=True)


if __name__ == "__main__":
    main()

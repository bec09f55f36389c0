#!/usr/bin/env python3
"""Training-batch augmentation at the trainer's size: a batch of 8 x 1080p.

Device: ``ops.augment_frames`` alone (frames, records and tables already on the device; five launches), and
``augment.augment_batch`` end to end (draws and label transforms on the host, one packed upload, the device chain).
Host: the same chain for one image on this box's CPU -- Pillow where it is installed (what torchvision's PIL backend calls),
else the numpy restatement of tests/augment_cases.py (slower than Pillow; said in the output).
Algorithmic bytes per pixel on the device: 3 read + 3 written in each of the three uint8 passes, 3 read in the sum pass,
3 read + 12 written in the finish pass = 36.  No speed is asserted.
    python tools/bench_augment.py"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d-playground_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from retinanet_mi355x import augment, ops   # noqa: E402

VPS = [[-310.5, 12.25], [2100.75, -55.5], [48.0, 3000.5]]


def host_chain(frame, p, noise):
    """One image through the reference's chain on the CPU -> (milliseconds, which implementation)."""
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        import augment_cases as ac
        t0 = time.perf_counter()
        ac.chain(frame, p, noise)
        return (time.perf_counter() - t0) * 1e3, "numpy restatement"
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
    if p["apply"]:
        for op in p["order"]:
            if op < 3:
                im = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(p["factors"][op])
    t = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div(255)
    t = (t - torch.tensor(ops.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(ops.IMAGENET_STD).view(3, 1, 1)
    t = torch.roll(t, (-p["dy"], -p["dx"]), (1, 2))
    return (time.perf_counter() - t0) * 1e3, "Pillow"


def main():
    dev = torch.device("cuda:0")
    B, H, W = 8, 1080, 1920
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    labels = [torch.from_numpy(rng.uniform(100, 900, size=(10, 21))) for _ in range(B)]
    np.random.seed(0)
    torch.manual_seed(0)
    drawn = [augment.draw(labels[i], "p1c1", VPS, (W, H))[0] for i in range(B)]
    for p in drawn:
        p["apply"] = 1                                        # time the longer path: jitter applied on every image
    rec, tx, ty = augment.pack_params(drawn, W, H)
    f = torch.from_numpy(frames).to(dev)
    params = (torch.from_numpy(rec.view(np.uint8).reshape(B, -1)).to(dev), torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev))
    for _ in range(3):
        ops.augment_frames(f, params, seed=1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ops.augment_frames(f, params, seed=1)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    nbytes = B * H * W * 36
    print("device chain, B = %d x %dx%d: %.3f ms per batch, %.3f ms per image, %.0f GB/s of algorithmic traffic (%.0f MB; "
          "includes the output and workspace allocations)" % (B, H, W, ms, ms / B, nbytes / ms / 1e6, nbytes / 1e6), flush=True)
    for _ in range(2):
        augment.augment_batch(list(frames), labels, ["p1c1"] * B, [VPS] * B, dev, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 5
    for _ in range(n):
        augment.augment_batch(list(frames), labels, ["p1c1"] * B, [VPS] * B, dev, seed=1)
    torch.cuda.synchronize()
    ms_all = (time.perf_counter() - t0) / n * 1e3
    print("end to end (draws, labels, tables, one packed upload of %.1f MB, device chain): %.2f ms per batch, %.2f ms per image"
          % (frames.nbytes / 1e6, ms_all, ms_all / B), flush=True)
    noise = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    host_chain(frames[0], drawn[0], noise)
    times = [host_chain(frames[i], drawn[i], noise) for i in range(min(B, 4))]
    print("the same chain on the host (%s, one thread of %d CPUs, as the reference's DataLoader(workers 0)): %.1f ms per image"
          % (times[0][1], len(os.sched_getaffinity(0)), sum(t for t, _ in times) / len(times)), flush=True)


if __name__ == "__main__":
    main()

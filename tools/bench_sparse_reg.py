"""Tile activity flags of the regression tower's backward, two measurements on the GPU.

1. What the flags cost when nothing can be skipped: one tower layer's backward (3x3, 256 -> 256, the five pyramid levels of a 1080p
   batch of 8; wino_wgrad_group(fuse_dgrad_input) + wino_conv_group(V_ready), the next layer's flags written) with a DENSE random
   gradient, every flag set, against the same call without flags.  Five rounds each, alternating: the difference has to be read
   against the spread of the rounds.
2. The active-tile fraction of one training step of the benchmark (ResNet-50, 8 x 1080 x 1920, synth.labels_dir(8, 10, .., seed=1)),
   read back from the five flag arrays of the engine, with the share of 128-row GEMM blocks and 16-row K-steps that stay.

    python tools/bench_sparse_reg.py [--no-step]
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "3d-playground_amd"))
import numpy as np
import torch
from retinanet_mi355x import conv as cv

dev = torch.device("cuda:0")
B, C = 8, 256
levels = [(135, 240), (68, 120), (34, 60), (17, 30), (9, 15)]


def timeit(run, iters=10):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        run()
    torch.cuda.synchronize()
    return (time.time() - t0) / iters * 1e3


def dense_cost():
    xs = [torch.randn(B, h, w, C, device=dev) for h, w in levels]
    gs = [torch.randn_like(x) for x in xs]
    w = torch.randn(C, C, 3, 3, device=dev) * (2.0 / (9 * C)) ** 0.5
    _, V = cv.wino_conv_group(xs, cv.wino_weights(w, 0), keep_v=True)
    Ud = cv.wino_weights(w, 1)
    wp = cv.pack_weights(w, 0)
    dw, cs, dU = torch.zeros_like(wp), torch.zeros(C, device=dev), torch.zeros((36, C, C), device=dev)
    outs = [torch.empty_like(x) for x in xs]
    T = sum(B * ((h + 3) // 4) * ((w_ + 3) // 4) for h, w_ in levels)
    ones = cv.tile_flags(dev, T)
    ones[:T] = 1
    fout = cv.tile_flags(dev, T)

    def run(flags):
        v = cv.wino_wgrad_group(gs, xs, dw, cs, V=V, dU=dU, fuse_dgrad_input=True, flags=flags)
        cv.wino_conv_group(gs, Ud, outs=outs, masks=xs, mask_mode=2, V_ready=v, flags_out=None if flags is None else fout)
    off, on = [], []
    for _ in range(5):
        off.append(timeit(lambda: run(None)))
        on.append(timeit(lambda: run(ones)))
    print("dense gradient, one tower layer's backward (T = %d tiles), ms per call, five alternating rounds of 10 calls" % T)
    print("  flags off: %s   median %.3f  spread %.3f" % (" ".join("%.3f" % t for t in off), np.median(off), max(off) - min(off)))
    print("  flags on : %s   median %.3f  spread %.3f" % (" ".join("%.3f" % t for t in on), np.median(on), max(on) - min(on)))
    print("  on - off (medians): %+.3f ms (%+.2f %%)" % (np.median(on) - np.median(off), 100.0 * (np.median(on) / np.median(off) - 1.0)))


def step_fractions():
    from retinanet_mi355x import modules, synth
    H, W = 1080, 1920
    net = modules.resnet50(num_classes=8)
    net.load_state_dict(synth.state_dict("resnet50", 8, 12, seed=2))
    net = net.to(dev)
    net.train()
    net.freeze_bn()
    img = synth.frames(B, H, W, seed=0).to(dev)
    ann = synth.labels_dir(B, 10, H, W, 8, seed=1).to(dev)
    sum(l.mean() for l in net([img, ann])).backward()
    torch.cuda.synchronize()
    T = sum(B * ((h + 3) // 4) * ((w_ + 3) // 4) for h, w_ in levels)
    print("active tiles of one benchmark step (T = %d), read back from the engine's flag arrays" % T)
    print("  %-28s %-12s %-18s %-18s" % ("depth", "tiles", "128-row GEMM blocks", "16-row K-steps"))
    for d, f in enumerate(net._engine._reg_flags):
        f = f.cpu().numpy()
        blk = lambda r: f[:(f.size // r) * r].reshape(-1, r).max(axis=1)[:(T + r - 1) // r].mean()
        print("  %-28s %-12s %-18s %-18s" % ("%d (%s)" % (d, ["output", "conv4", "conv3", "conv2", "conv1"][d]),
                                            "%.1f %%" % (100.0 * f[:T].mean()), "%.1f %%" % (100.0 * blk(128)), "%.1f %%" % (100.0 * blk(16))))


if __name__ == "__main__":
    dense_cost()
    if "--no-step" not in sys.argv:
        step_fractions()

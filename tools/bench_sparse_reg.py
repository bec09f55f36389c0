"""Tile activity flags of the regression tower's backward, two measurements on the GPU.

1. What the flags cost when nothing can be skipped: one tower layer's backward (3x3, 256 -> 256, the five pyramid levels of a 1080p
   batch of 8; wino_wgrad_group(fuse_dgrad_input) + wino_conv_group(V_ready), the next layer's flags written) with a DENSE random
   gradient, every flag set, against the same call without flags.  Five rounds each, alternating: the difference has to be read
   against the spread of the rounds.
2. The active-tile fraction of one training step of the benchmark (ResNet-50, 8 x 1080 x 1920, synth.labels_dir(8, 10, .., seed=1)),
   read back from the five flag arrays of the engine, with the share of 128-row GEMM blocks and 16-row K-steps that stay, and the
   lengths of the work lists the engine built from them (cv.tile_lists).
3. With the flags of that step, depth by depth: one tower layer's backward dense / with early exits / over the work lists, and the list
   builder's own cost.

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


def layer_setup():
    xs = [torch.randn(B, h, w, C, device=dev) for h, w in levels]
    w = torch.randn(C, C, 3, 3, device=dev) * (2.0 / (9 * C)) ** 0.5
    _, V = cv.wino_conv_group(xs, cv.wino_weights(w, 0), keep_v=True)
    wp = cv.pack_weights(w, 0)
    return xs, V, cv.wino_weights(w, 1), torch.zeros_like(wp), torch.zeros(C, device=dev), torch.zeros((36, C, C), device=dev)


def with_step_flags(step_flags):
    """One 256 -> 256 tower layer's backward on a gradient that is non-zero exactly in the flagged tiles' inner pixels of a real step."""
    xs, V, Ud, dw, cs, dU = layer_setup()
    outs = [torch.empty_like(x) for x in xs]
    T = sum(B * ((h + 3) // 4) * ((w_ + 3) // 4) for h, w_ in levels)
    fout = cv.tile_flags(dev, T)
    print("one tower layer's backward with the flags of a benchmark step (ms per call, median of five rounds of 10 calls)")
    print("  %-6s %-10s %-10s %-10s %-12s" % ("depth", "dense", "early exit", "lists", "list builder"))
    for d, f in enumerate(step_flags):
        flags = f.clone()
        gs, off = [], 0
        for (h, w_), x in zip(levels, xs):                         # the centre pixels of the flagged tiles carry the gradient
            th, tw = (h + 3) // 4, (w_ + 3) // 4
            m = flags[off:off + B * th * tw].view(B, th, tw).float()
            g = torch.zeros_like(x)
            g[:, 1::4, 1::4, :] = m[:, :g[:, 1::4].shape[1], :g[:, :, 1::4].shape[2], None] * torch.randn(B, 1, 1, C, device=dev)
            gs.append(g)
            off += B * th * tw
        bufl = torch.empty(cv.tile_lists_numel(flags.numel()), dtype=torch.int32, device=dev)

        def run(mode):
            fl = None if mode == 0 else flags
            v = cv.wino_wgrad_group(gs, xs, dw, cs, V=V, dU=dU, fuse_dgrad_input=True, flags=fl, lists=bufl if mode == 2 else None)
            cv.wino_conv_group(gs, Ud, outs=outs, masks=xs, mask_mode=2, V_ready=v, flags_out=None if fl is None else fout)
        t = [[], [], [], []]
        for _ in range(5):
            for mode in range(3):
                t[mode].append(timeit(lambda: run(mode)))
            t[3].append(timeit(lambda: cv.tile_lists(flags, buf=bufl)))
        print("  %-6d %-10.3f %-10.3f %-10.3f %-12.4f" % ((d,) + tuple(float(np.median(x)) for x in t)))


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
    lists = getattr(net._engine, "_reg_lists", None) or []
    if lists:
        print("  work lists of that step (tiles, 16-row units, 128-row blocks): " +
              "  ".join("%d: %d / %d / %d" % ((d,) + tuple(b[:3].tolist())) for d, b in enumerate(lists)))
    return [f.clone() for f in net._engine._reg_flags]


if __name__ == "__main__":
    dense_cost()
    if "--no-step" not in sys.argv:
        with_step_flags(step_fractions())

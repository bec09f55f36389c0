"""The fused backward of a 1x1 stride-1 layer (conv.bwd_1x1_fused) against the pair of launches it replaces (conv.wgrad + conv.dgrad), per
shape: HIP events around each form, median of 20 after 3 warm-ups, operand sets rotated so that no launch finds its inputs in the
256 MiB Infinity Cache.  A record (profiles/bwd_fused_1x1.txt), not a gate.

    python tools/bench_bwd_fused.py [--shapes 8x270x480 2x270x480 8x135x240]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-playground_amd"))
from retinanet_mi355x import conv as cv  # noqa: E402

CIN, COUT = 64, 256


def sign_words(t):
    b = (t.flatten() > 0).view(-1, 32).to(torch.int64)
    w = (b << torch.arange(32, device=t.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def median_ms(fn, nset, iters=20, warm=3):
    ts = []
    for i in range(warm + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i % nset)
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["8x270x480", "2x270x480", "8x135x240"])
    ap.add_argument("--masks", nargs="*", type=int, default=[2, 0], help="0 none, 1 fp32 activations, 2 sign bits")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cv.set_fp32_mfma("split3")
    weight = torch.randn(COUT, CIN, 1, 1, device=dev) * 0.05
    wd = cv.pack_weights(weight, 1)
    print("%-12s %-5s %10s %10s %8s   %s" % ("shape", "mask", "pair ms", "fused ms", "ratio", "fused: GB/s of algorithmic bytes (dy + x + dx once)"))
    for sh in args.shapes:
        N, H, W = (int(v) for v in sh.split("x"))
        bytes_once = 4.0 * N * H * W * (COUT + 2 * CIN)
        nset = max(2, int(2 * 2 ** 28 // bytes_once) + 1)               # the sets in rotation exceed twice the cache
        sets = []
        for _ in range(nset):
            dy = torch.randn(N, H, W, COUT, device=dev)
            x = torch.randn(N, H, W, CIN, device=dev).clamp_(min=0)
            x._rn_sign = sign_words(x)
            cv.amax_words(dy), cv.amax_words(x)
            sets.append((dy, x))
        dw, cs = torch.zeros(COUT, CIN, device=dev), torch.zeros(COUT, device=dev)
        for mm in args.masks:
            def mask_of(x):                                            # mode 1: the same activations without their sign bits
                if mm == 1 and not hasattr(x, "_plain"):
                    x._plain = x.clone()
                return None if mm == 0 else (x._plain if mm == 1 else x)

            def pair(i):
                dy, x = sets[i]
                cv.wgrad(dy, x, dw, COUT, 1, 1, 0, colsum=cs)
                cv.dgrad(dy, wd, (H, W), CIN, 1, 1, 0, mask=mask_of(x), mask_mode=2)

            def fused(i):
                dy, x = sets[i]
                cv.bwd_1x1_fused(dy, x, wd, dw, cs, mask=mask_of(x), mask_mode=mm or None)

            p = median_ms(pair, nset)
            f = median_ms(fused, nset)
            print("%-12s %-5d %10.4f %10.4f %8.3f   %.0f   (pair min/max %.4f/%.4f, fused %.4f/%.4f)" % (
                sh, mm, p[0], f[0], f[0] / p[0], bytes_once / f[0] / 1e6, p[1], p[2], f[1], f[2]))
        del sets


if __name__ == "__main__":
    main()

"""How sparse is the gradient that enters the regression tower?  CPU only (no GPU, no library).

The loss has a regression term for the positive anchors only, so dL/d(regression output) is zero except at the pixels that own a
positive anchor, and every 3x3 data gradient widens the non-zero region by one pixel.  For the benchmark's own labels
(synth.labels_dir(8, 10, 1080, 1920, 8, seed=1), the oracle's anchors, IoU >= 0.5) this counts, per depth of the tower's backward
(0 = regressionModel.output .. 4 = conv1), the Winograd tiles whose 6x6 input patch holds a pixel that CAN be non-zero, and the share
of 32- / 128- / 256-row blocks of the tile-ordered V / Z / M that hold such a tile.  The ReLU masks are ignored (the real region is
smaller); rounding residue of the Winograd arithmetic is ignored too (the real flags are larger: DESIGN.md 4.4).

    python tools/reg_sparsity.py [--boxes 10] [--batch 8] [--height 1080] [--width 1920] > profiles/reg_sparsity.txt
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "3d-playground_amd"))
from oracle import anchors as oanchors, losses as olosses   # noqa: E402
from retinanet_mi355x import synth                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args()
    B, H, W = a.batch, a.height, a.width
    ann = synth.labels_dir(B, a.boxes, H, W, 8, seed=1)
    anc = torch.from_numpy(oanchors.anchors_for_image(H, W))[0]
    grids = [oanchors.level_grid(H, W, l) for l in oanchors.PYRAMID_LEVELS]
    positives, maps = [], [[] for _ in grids]
    for b in range(B):
        rows = ann[b][ann[b][:, 20] != -1]
        pos = torch.zeros(anc.shape[0], dtype=torch.bool)
        if rows.shape[0]:
            pos = olosses.assign(anc, olosses.envelope_boxes(rows[:, :16]))[2] == 1
        positives.append(int(pos.sum()))
        off = 0
        for li, (gh, gw) in enumerate(grids):
            n = 9 * gh * gw
            maps[li].append(pos[off:off + n].view(gh, gw, 9).any(dim=2))
            off += n
    print("labels: synth.labels_dir(%d, %d, %d, %d, 8, seed=1); anchors per image %d" % (B, a.boxes, H, W, anc.shape[0]))
    print("positives per image: %s" % positives)
    print("%-6s %-14s %-12s %-12s %-12s %s" % ("depth", "active tiles", "32-row", "128-row", "256-row", "work lists: tiles / 16-row units / 128-row blocks"))
    cur = [torch.stack(m).float()[:, None] for m in maps]       # [B,1,gh,gw] per level: pixels that can be non-zero
    for depth in range(5):
        flags = []
        for m in cur:
            gh, gw = m.shape[2:]
            TH, TW = (gh + 3) // 4, (gw + 3) // 4
            pad = torch.zeros(B, 1, 4 * TH + 2, 4 * TW + 2)
            pad[:, :, 1:1 + gh, 1:1 + gw] = m
            flags.append(F.max_pool2d(pad, 6, 4).reshape(-1))    # the tile's 6x6 patch, tiles in (image, row, column) order
        f = torch.cat(flags).numpy()
        line = "%-6d %-14s" % (depth, "%.1f %%" % (100.0 * f.mean()))
        for rows_ in (32, 128, 256):
            n = (f.size + rows_ - 1) // rows_
            g = np.zeros(n * rows_)
            g[:f.size] = f
            line += " %-12s" % ("%.1f %%" % (100.0 * g.reshape(n, rows_).max(axis=1).mean()))
        cnt = lambda r: int(np.pad(f, (0, -f.size % r)).reshape(-1, r).max(axis=1).sum())
        line += " %d / %d / %d" % (cnt(1), cnt(16), cnt(128))       # the lengths of cv.tile_lists' lists for these flags
        print(line)
        cur = [F.max_pool2d(m, 3, 1, 1) for m in cur]           # a 3x3 data gradient: one pixel wider
    print("tiles: %d" % f.size)


if __name__ == "__main__":
    main()

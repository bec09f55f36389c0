"""Host side of tests/test_reg_need_host.py and tests/test_gpu_sparse_reg_fwd.py: the need sets of the regression tower's forward
 restated in numpy.  No GPU, no torch.

P0: the 4x4 output tiles of a pyramid level that hold a pixel with a positive anchor (best IoU >= 0.5 against the image's valid labels).
D: the 3x3 dilation on the tile grid of one image of one level -- never across a grid edge, an image or a level.
F[0] = P0 (the output layer's result), F[k] = D^(k+1)(P0) for k = 1..4 (conv4 .. conv1's results), and E = D(P0), the tiles whose input
transform the output layer keeps for its weight gradient.  Everything is held per level as a bool array [N, TH, TW]; `flat` lays the
levels out in the tile order of the Winograd transforms (levels concatenated; image, tile row, tile column)."""
import numpy as np

import sparse_reg_list_cases as sc


def grid(hw):
    return (hw[0] + 3) // 4, (hw[1] + 3) // 4


def dilate(maps):
    """D, per level [N, TH, TW] bool."""
    out = []
    for m in maps:
        p = np.pad(m, ((0, 0), (1, 1), (1, 1)))
        d = np.zeros_like(m)
        for a in range(3):
            for b in range(3):
                d |= p[:, a:a + m.shape[1], b:b + m.shape[2]]
        out.append(d)
    return out


def need_sets(p0):
    """p0: per level [N, TH, TW] bool -> ([F[0] .. F[4]], E)."""
    e = dilate(p0)
    f, cur = [p0], e
    for _ in range(4):
        cur = dilate(cur)
        f.append(cur)
    return f, e


def flat(maps, length):
    out = np.zeros(length, dtype=np.uint8)
    v = np.concatenate([m.reshape(-1) for m in maps])
    out[:v.size] = v
    return out


def tiles_of_pixels(pixel_maps):
    """Per level [N, H, W] bool (a pixel that holds something) -> [N, TH, TW] bool (the tiles that hold such a pixel)."""
    out = []
    for m in pixel_maps:
        n, H, W = m.shape
        TH, TW = grid((H, W))
        p = np.zeros((n, 4 * TH, 4 * TW), dtype=bool)
        p[:, :H, :W] = m
        out.append(p.reshape(n, TH, 4, TW, 4).any(axis=(2, 4)))
    return out


def backward_flags(p0, steps=5):
    """The LARGEST flag sets the backward of DESIGN.md 4.4 can reach from a gradient that is non-zero only in the tiles of p0, every pixel of
    an active tile taken as non-zero at every depth: B[0] from the rule of the producers (sc.rule_flags), B[k+1] from the same rule applied to
    the stored result of depth k, which is non-zero at most in the active tiles of B[k].  -> per depth a list of per-level [N, TH, TW]."""
    out, cur = [], p0
    for _ in range(steps):
        px = [np.repeat(np.repeat(m, 4, axis=1), 4, axis=2) for m in cur]
        length = sum(m.size for m in cur)
        f = sc.rule_flags(px, length)
        nxt, base = [], 0
        for m in cur:
            nxt.append(f[base:base + m.size].reshape(m.shape) != 0)
            base += m.size
        out.append(nxt)
        cur = nxt
    return out


def positive_pixels(anchors, ann, hws, per_pixel=9, directional=True):
    """anchors [A, 4] in level order (pixels row-major, per_pixel anchors each), ann [B, N, 27 | 5] -> per level [B, H, W] bool: the pixel
    has a positive anchor.  IoU in float32 in calc_iou's operation order (the kernels' arithmetic, one rounding per operation)."""
    f = np.float32
    a = np.asarray(anchors, dtype=f).reshape(-1, 4)
    ann = np.asarray(ann, dtype=f)
    B = ann.shape[0]
    pos = np.zeros((B, a.shape[0]), dtype=bool)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    for j in range(B):
        rows = ann[j][ann[j][:, 20 if directional else 4] != -1]
        best = np.full(a.shape[0], -1, dtype=f)
        for r in rows:
            if directional:
                xs, ys = r[0:16:2], r[1:16:2]
                x1, y1, x2, y2 = xs.min(), ys.min(), xs.max(), ys.max()
            else:
                x1, y1, x2, y2 = r[:4]
            area = f(f(x2 - x1) * f(y2 - y1))
            iw = np.maximum(np.minimum(a[:, 2], x2) - np.maximum(a[:, 0], x1), f(0))
            ih = np.maximum(np.minimum(a[:, 3], y2) - np.maximum(a[:, 1], y1), f(0))
            inter = iw * ih
            ua = np.maximum((area_a + area) - inter, f(1e-8))
            best = np.maximum(best, np.where(inter > 0, inter / ua, f(0)))
        if len(rows):
            pos[j] = best >= f(0.5)
    out, off = [], 0
    for H, W in hws:
        cnt = H * W * per_pixel
        out.append(pos[:, off:off + cnt].reshape(B, H, W, per_pixel).any(axis=3))
        off += cnt
    assert off == a.shape[0]
    return out

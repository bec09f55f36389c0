"""Host side of tests/test_gpu_sparse_reg_lists.py: the rules of the tile work lists restated in numpy, and the flag
patterns the list builder is held to.  No GPU, no torch."""
import numpy as np


def lists_of(flags):
    """flags: uint8 [Tpad], Tpad a multiple of 256 -> (tiles, units, blocks): the ascending indices of the non-zero flags, of the aligned
    16-row units and of the 128-row blocks that hold one."""
    f = np.asarray(flags) != 0
    assert f.ndim == 1 and f.size % 256 == 0
    return (np.flatnonzero(f).astype(np.int32), np.flatnonzero(f.reshape(-1, 16).any(axis=1)).astype(np.int32),
            np.flatnonzero(f.reshape(-1, 128).any(axis=1)).astype(np.int32))


def tiles_of(shape):
    return shape[0] * ((shape[1] + 3) // 4) * ((shape[2] + 3) // 4)


def rule_flags(nonzero_maps, length):
    """The producers' rule: a non-zero pixel sets its own tile; column 0 / 3 of a tile the left / right neighbour, rows likewise, the four
    corner pixels the diagonal neighbours -- inside the level's TH x TW and the same image.  nonzero_maps: per level a bool array
    [N, H, W], in group order -> uint8 [length]."""
    out = np.zeros(length, dtype=np.uint8)
    base = 0
    for nz in nonzero_maps:
        n_, H, W = nz.shape
        TH, TW = (H + 3) // 4, (W + 3) // 4
        f = out[base:base + n_ * TH * TW].reshape(n_, TH, TW)
        for n, h, w in np.argwhere(nz):
            th, tw = h // 4, w // 4
            for a in (-1, 0, 1):
                for b in (-1, 0, 1):
                    ok_r = a == 0 or (h % 4 == 0 and th > 0 if a < 0 else h % 4 == 3 and th + 1 < TH)
                    ok_c = b == 0 or (w % 4 == 0 and tw > 0 if b < 0 else w % 4 == 3 and tw + 1 < TW)
                    if ok_r and ok_c:
                        f[n, th + a, tw + b] = 1
        base += n_ * TH * TW
    return out


def builder_patterns(T, Tpad, plane):
    """Flag arrays for the list builder.  T tiles in Tpad rows; plane = (first row, TH, TW) of one image's tile plane inside them."""
    assert T <= Tpad and Tpad % 256 == 0
    first, TH, TW = plane
    z = lambda: np.zeros(Tpad, dtype=np.uint8)
    pats = {"no_flag": z()}
    f = z(); f[:T] = 1
    pats["every_flag"] = f
    f = z(); f[first] = 1; f[first + (TH - 1) * TW + TW - 1] = 1      # one tile in the first and one in the last row of a plane
    pats["first_and_last_row_of_a_plane"] = f
    f = z()
    for b in range((T + 127) // 128):                                  # one active tile per 128-row block, at a different place in each
        f[min(128 * b + (37 * b + 5) % 128, T - 1)] = 1
    pats["one_tile_per_block"] = f
    f = z(); f[128 * ((T - 1) // 128):T] = 1                           # only the last block that holds tiles (the padding follows it)
    pats["last_block_only"] = f
    f = z(); f[T - 1] = 1
    pats["last_tile_only"] = f
    f = z(); f[:T:7] = 3; f[1:T:16] = 255                              # any non-zero byte counts as a flag
    pats["non_unit_bytes"] = f
    return pats

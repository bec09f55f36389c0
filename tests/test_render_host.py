"""CPU: the drawing rules restated in tests/render_cases.py against rasters typed by hand; the font table, the mosaic
layout and the label strings of mc3d_render; the new entry points in the binding; the tracker's refusals with
``params["render"]`` present."""
import numpy as np
import pytest
import torch

import render_cases as rc
import track_cases as tc
import tracker_cases as trc


def _raster(rows):
    return np.array([[ch == "#" for ch in row] for row in rows])


def _edge(ax, ay, bx, by, t):
    """One edge through paint_edges: corners 0 and 1 carry it, every other corner is not finite."""
    box = np.full((8, 2), np.nan)
    box[0], box[1] = (ax, ay), (bx, by)
    return rc.paint_edges(rc.new_mask(1, 9, 9), box[None], [0], t, 2)[0] == 4


def test_known_rasters():
    # thickness 1: 4 d^2 <= 1 -- only pixels on the segment
    assert np.array_equal(_edge(1, 4, 7, 4, 1), _raster([".........",
                                                         ".........",
                                                         ".........",
                                                         ".........",
                                                         ".#######.",
                                                         ".........",
                                                         ".........",
                                                         ".........",
                                                         "........."]))
    assert np.array_equal(_edge(1.9, 1.2, 6.5, 6.9, 1), _raster([".........",
                                                                 ".#.......",
                                                                 "..#......",
                                                                 "...#.....",
                                                                 "....#....",
                                                                 ".....#...",
                                                                 "......#..",
                                                                 ".........",
                                                                 "........."]))
    # 1:2 from (0, 2) to (8, 6): the pixels between the lattice points lie 1/sqrt(5) off the line, inside 1/2
    assert np.array_equal(_edge(0, 2, 8, 6, 1), _raster([".........",
                                                         ".........",
                                                         "##.......",
                                                         ".###.....",
                                                         "...###...",
                                                         ".....###.",
                                                         ".......##",
                                                         ".........",
                                                         "........."]))
    # a zero-length edge is a disc: thickness 3 takes d^2 <= 2.25, the neighbours and the diagonals; thickness 2 only d^2 <= 1
    assert np.array_equal(_edge(4, 4, 4, 4, 3), _raster([".........",
                                                         ".........",
                                                         ".........",
                                                         "...###...",
                                                         "...###...",
                                                         "...###...",
                                                         ".........",
                                                         ".........",
                                                         "........."]))
    assert np.array_equal(_edge(4, 4, 4, 4, 2), _raster(["........."] * 3 + ["....#....", "...###...", "....#...."] + ["........."] * 3))


def test_rule_is_symmetric_and_skips_bad_edges():
    assert np.array_equal(_edge(0, 2, 8, 6, 3), _edge(8, 6, 0, 2, 3))
    for bad in (np.nan, np.inf, -np.inf, 8192.0, -8193.0):
        assert not _edge(bad, 2, 8, 6, 3).any()
    assert _edge(8191.9, 2, 0, 2, 1)[2].all() and _edge(-8192.9, 2, 8, 2, 1)[2].all()     # truncation comes first
    assert rc.anchor_of([[3.9, -2.5]] * 7 + [[-0.5, 7.9]]) == (0, 7) and rc.anchor_of([[np.nan, 1]] * 8) is None


def test_rects_and_text_restated():
    m = rc.paint_rects(rc.new_mask(1, 6, 8), [[1, 1, 6, 5, 0, 1, -1, 0], [6, 4, 20, 20, 0, 0, -1, 1], [3, 3, 3, 9, 0, 0, -1, 2]])[0]
    assert np.array_equal(m & 1, _raster(["........", ".#####..", ".#...#..", ".#...#..", ".#####..", "........"]))
    assert np.array_equal((m >> 1) & 1, _raster(["........"] * 4 + ["......##"] * 2)) and not (m & 4).any()
    from mc3d_render import FONT
    text = np.frombuffer(b"A\x07", np.uint8)
    m = rc.paint_text(rc.new_mask(1, 10, 14), [[1, 9, 0, -1, 1, 0, 0, 0, 2]], text, FONT)[0]
    want = _raster(["..............", "..###...###...", ".#...#.#...#..", ".#...#.....#..", ".#...#....#...", ".#####...#....",
                    ".#...#........", ".#...#...#....", "..............", ".............."])
    assert np.array_equal(m == 1, want)                                   # 'A', and '?' for a byte outside 32..126
    big = rc.paint_text(rc.new_mask(1, 20, 28), [[2, 18, 0, -1, 2, 0, 0, 0, 2]], text, FONT)[0]
    assert np.array_equal(big == 1, np.kron(want, np.ones((2, 2), bool)))                      # scale 2: every pixel a 2x2 block
    fat = rc.paint_text(rc.new_mask(1, 10, 14), [[1, 9, 0, -1, 1, 1, 0, 0, 2]], text, FONT)[0] == 1
    grown = np.zeros_like(want)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            grown[max(dy, 0):10 + min(dy, 0), max(dx, 0):14 + min(dx, 0)] |= want[max(-dy, 0):10 - max(dy, 0), max(-dx, 0):14 - max(dx, 0)]
    assert np.array_equal(fat, grown)


def test_compose_restated_known_values():
    frames = np.zeros((1, 3, 1, 8), np.float32)
    u8 = np.array([0, 1, 127, 128, 90, 254, 255, 200], np.float32)
    for ch in range(3):
        frames[0, ch, 0] = (u8 / np.float32(255) - np.float32(rc.MEAN[ch])) / np.float32(rc.STD[ch])
    B = rc.BIT
    mask = np.array([[[0, 1 << B["track"], 1 << B["in_crop"], 0, 1 << B["label"], (1 << B["label"]) | (1 << B["label_text"]),
                       1 << B["banner_edge"], (1 << B["banner_edge"]) | (1 << B["banner_text"])]]], np.uint16)
    plain = rc.compose(frames, np.zeros_like(mask), False, 1)
    assert np.array_equal(plain[0, :, 0], u8.astype(np.uint8)) and np.array_equal(plain[0, :, 1], plain[0, :, 2])
    out = rc.compose(frames, mask, True, 1)[0]
    assert out[0].tolist() == [0, 0, 0] and out[1].tolist() == [0, 255, 255]        # TRACK (0, 200, 25) dimmed to (0, 60, 7.5), saturated
    assert out[2].tolist() == [127] * 3 and out[3].tolist() == [38] * 3             # inside a crop / 0.3 * 128 = 38.4
    assert out[4].tolist() == [95] * 3 and out[5].tolist() == [0] * 3                # 0.7 * (0.3 * 90) + 0.3 * 255 = 95.4
    assert out[6].tolist() == [255] * 3 and out[7].tolist() == [0] * 3


def test_font_table():
    from mc3d_render import FONT
    assert FONT.shape == (95, 8) and FONT.dtype == np.uint8
    assert not FONT[0].any() and all(FONT[g].any() for g in range(1, 95))
    assert len({FONT[g].tobytes() for g in range(95)}) == 95
    assert not (FONT & 1).any() and not FONT[:, 7].any() and FONT.max() < 64     # column 5 and row 7 are blank


def test_mosaic_layout():
    from mc3d_render import mosaic_layout
    assert mosaic_layout(2) == (1, 2) and mosaic_layout(18) == (4, 5) and mosaic_layout(1) == (1, 1)
    for n in range(1, 19):
        rows, cols = mosaic_layout(n)
        tiles = [(i // cols, i % cols) for i in range(n)]
        assert len(set(tiles)) == n and all(r < rows and c < cols for r, c in tiles) and rows * cols - n < cols
        assert (rows, cols) == rc.layout(n)


def test_label_lines():
    from mc3d_render import banner_text, label_lines
    lines = label_lines([400.0, 12.0, 16.25, 6.35, 4.55, 1.0, 88.0], "sedan", 7)
    assert lines == ["sedan 7:", "60.0mph EB", "L: 16.2ft", "W: 6.4ft", "H: 4.6ft"]     # 162.5 rounds to even, as numpy's round
    assert label_lines([0, 0, 16.75, 2.5, 0.25, -1.0, -88.0], "semi", 12, 2) == ["semi 12:", "60.0mph WB"]
    assert label_lines([0, 0, 16.75, 2.5, 0.25, -1.0, 110.0], "semi", 12)[2:] == ["L: 16.8ft", "W: 2.5ft", "H: 0.2ft"]
    assert label_lines([0, 0, 1, 1, 1, 0.5, 0.0], "x", 0, 1) == ["x 0:"] and label_lines([0] * 5 + [1, 0], "x", 0, 9)[1] == "0.0mph EB"
    assert banner_text(0.0123449, 80.0) == "Estimated time bias: 0.0123s (1.0ft)" and banner_text(0, 80.0).startswith("Estimated time bias: 0.0000s")


def test_entry_points_are_bound_and_registered():
    from retinanet_mi355x import _hip, ops, torch_ops
    counts = dict(rn_render_edges=10, rn_render_rects=9, rn_render_text=12, rn_render_compose=15)
    for name, n in counts.items():
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n, name
        op = name[3:]
        assert op in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, op) and hasattr(ops, op)
    assert ops.RENDER_BITS == rc.BIT
    mask = torch.zeros((1, 4, 4), dtype=torch.uint16)
    with pytest.raises(RuntimeError):
        ops.render_edges(torch.zeros((1, 8, 2), dtype=torch.float64), torch.zeros(1, dtype=torch.int32), 1, 2, mask)
    with pytest.raises(RuntimeError):
        ops.render_compose(torch.zeros((1, 3, 4, 4)), mask, False, 1)
    lib = _hip.load()                                            # host-side argument checks of the C entry points
    assert lib.rn_render_edges(None, None, 0, 0, 2, 16, 1, 4, 4, None) == 10001           # thickness 0
    assert lib.rn_render_edges(None, None, 0, 1, 2, 18, 1, 4, 4, None) == 10001           # a mask that is not 4-byte aligned
    assert lib.rn_render_edges(None, None, 0, 1, 2, 16, 1, 4, 4, None) == 0               # n = 0: nothing launched
    assert lib.rn_render_rects(None, 0, None, 0, 16, 1, 4, 20000, None) == 10001          # W above RN_RENDER_MAX_DIM
    assert lib.rn_render_text(None, 0, None, 0, None, None, 0, 16, 1, 4, 4, None) == 0


def test_constructor_refusals_with_render_params():
    from mc3d_tracker import MC_Crop_Tracker
    det, cd = trc.StandInDetector(), trc.StandInCropDetector()
    loaders = [trc.ScriptedLoader(c) for c in range(3)]

    class HG:
        correspondence = {c: {} for c in trc.CAMERAS}
    params = dict(trc.PARAMS, cam_centers=dict(trc.CAM_CENTERS), ts=trc.ts_table(), render=dict(out=None))
    with pytest.raises(NotImplementedError, match="PLOT=False"):
        MC_Crop_Tracker(loaders, det, tc.kf_init(), HG(), tc.class_dict(), params=params, cd=cd)
    with pytest.raises(NotImplementedError, match="PLOT=False"):
        MC_Crop_Tracker(loaders, det, tc.kf_init(), HG(), tc.class_dict(), params=params, cd=cd, PLOT=False, OUT="frames")
    with pytest.raises(ValueError, match="render"):
        MC_Crop_Tracker(loaders, det, tc.kf_init(), HG(), tc.class_dict(), params=dict(params, render=dict(colour="red")), cd=cd, PLOT=False)
    with pytest.raises(ValueError, match="every"):
        MC_Crop_Tracker(loaders, det, tc.kf_init(), HG(), tc.class_dict(), params=dict(params, render=dict(every=0)), cd=cd, PLOT=False)

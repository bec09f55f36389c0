"""Drop-in for the reference's ``timestamp_utilities`` time stamp reader, on the device.

``parse_frame_timestamp`` keeps the reference's surface (timestamp_utilities.py:46-115): it returns ``(timestamp, None)``
or ``(None, mask pixels of the failing cell)``.  The strip is thresholded, cut into cells and looked up by
``ops.parse_frame_timestamps`` (csrc/ts_parse.hip); the value is then formed as the reference forms it, ``str(key)`` of
the matched table entries joined around the decimal point and handed to ``ast.literal_eval``, so a stamp of ten cells or
fewer is an ``int`` here too.  The batched form the loaders want -- B cameras, up to four (geometry, table) sets tried in
turn, ``prev + 1/30.0`` when nobody reads a frame -- is ``TimestampReader``; its fp64 values equal the literal's bit for bit.

The three file readers are host code as in the reference.  Its pickled tables are not shipped: ``make_checksums`` builds a
table from ten glyph masks.  One difference: a strip that runs past the frame's edge is dark there (the same six sums as
numpy's clamped slice), and the mask pixels returned for it have the cell's full ``h x w``, where the reference's are
clipped.
"""
import ast
import pickle

import numpy as np
import torch

from retinanet_mi355x import ops

DEFAULT_CHECKSUMS = "./resources/timestamp_pixel_checksum_6.pkl"
DEFAULT_GEOMETRY = "./resources/timestamp_geometry_4K.pkl"


def _unpickle(path):
    with open(path, "rb") as fh:
        return pickle.load(fh)


def get_precomputed_checksums(abs_path=None):
    """The checksum table: a dict key -> 3x2 counts, from ``abs_path`` or the reference's default location."""
    return _unpickle(DEFAULT_CHECKSUMS if abs_path is None else abs_path)


def get_timestamp_geometry(abs_path=None):
    """The geometry dict (x0, y0, w, h, n, h13, h23, h12, w12), from ``abs_path`` or the reference's default location."""
    return _unpickle(DEFAULT_GEOMETRY if abs_path is None else abs_path)


def get_timestamp_pixel_limits():
    """(y1, y2, x1, x2) of the default geometry's strip: ``frame[y1:y2, x1:x2, :]`` is what ``timestamp_pixels`` takes."""
    g = get_timestamp_geometry()
    return g["y0"], g["y0"] + g["h"], g["x0"], g["x0"] + g["n"] * g["w"]


def make_checksums(glyph_masks, geometry):
    """A checksum table from glyph masks: ``glyph_masks`` is a mapping key -> [h,w] array or a sequence of ten such arrays
    (digit 0 first); a pixel counts when it is non-zero.  -> dict key -> int 3x2 array: the white pixels of the row bands
    [0,h13), [h13,h23), [h23,h) by the column halves [0,w12), [w12,w).  ValueError for a mask of another size and for
    two glyphs with equal checksums (the reader could not tell them apart)."""
    h, w, h13, h23, w12 = (int(geometry[k]) for k in ("h", "w", "h13", "h23", "w12"))
    items = list(glyph_masks.items()) if hasattr(glyph_masks, "items") else list(enumerate(glyph_masks))
    table = {}
    for key, m in items:
        m = np.asarray(m.cpu() if torch.is_tensor(m) else m) != 0
        if m.shape != (h, w):
            raise ValueError("glyph %r is %s, the geometry's cell is %s" % (key, m.shape, (h, w)))
        rows, cols = (slice(0, h13), slice(h13, h23), slice(h23, h)), (slice(0, w12), slice(w12, w))
        table[key] = np.array([[int(m[r, c].sum()) for c in cols] for r in rows], dtype=np.int64)
    flat = [tuple(v.reshape(6)) for v in table.values()]
    if len(set(flat)) != len(flat):
        raise ValueError("two glyphs have the same six-area checksum under this geometry")
    return table


def _device_frames(pixels, device):
    t = pixels if torch.is_tensor(pixels) else torch.from_numpy(np.ascontiguousarray(pixels))
    if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
        raise ValueError("a frame is uint8 [H,W,3], got %s %s" % (t.dtype, tuple(t.shape)))
    return t if t.is_cuda else t.to(device)


def parse_frame_timestamp(timestamp_geometry, precomputed_checksums, frame_pixels=None, timestamp_pixels=None, device="cuda"):
    """The reference's call: one frame (or its strip), one geometry, one table; numpy arrays or tensors.
    -> (timestamp, None), or (None, uint8 [h,w] mask pixels of the first cell without an exact checksum match)."""
    g = dict((k, int(timestamp_geometry[k])) for k in ops.TS_GEOMETRY_KEYS)
    if frame_pixels is not None:
        if not torch.is_tensor(frame_pixels) or not frame_pixels.is_cuda:         # a host frame: only the strip travels
            frame_pixels = frame_pixels[g["y0"]:g["y0"] + g["h"], g["x0"]:g["x0"] + g["n"] * g["w"], :]
            g["x0"] = g["y0"] = 0
        pixels = frame_pixels
    elif timestamp_pixels is not None:
        pixels = timestamp_pixels
        g["x0"] = g["y0"] = 0
    else:
        raise ValueError("One of `frame_pixels` or `timestamp_pixels` must be specified.")
    geo, tab = ops.pack_timestamp_sets([(g, precomputed_checksums)])
    if pixels.shape[0] == 0 or pixels.shape[1] == 0:                              # the strip lies outside the frame: all dark
        pixels = np.zeros((1, 1, 3), np.uint8)
    f = _device_frames(pixels, device)
    _, status, _, digits, fail_cell, mask = ops.parse_frame_timestamps(f, (geo, torch.from_numpy(tab).to(f.device)), want_mask=True)
    if int(status[0]) != ops.TS_READ:
        j = int(fail_cell[0])
        return None, mask[0, :, j * g["w"]:(j + 1) * g["w"]].cpu().numpy()
    keys = list(precomputed_checksums.keys())
    row = digits[0].cpu().tolist()
    text = "".join("." if j == 10 else str(keys[row[j]]) for j in range(g["n"]))
    return ast.literal_eval(text), None


class TimestampReader:
    """What MC_Crop_Tracker.__next__ (MC3D_crop_tracker.py:211-215) and Camera_Wrapper.__next__ (datareader.py:55-68) do
    with their lists, for ``n_cameras`` frames per call: the tables are uploaded once, the previous stamps stay on the device
    (zeros at the start, as the tracker's list), and a frame that no set reads takes ``prev + 1/30.0``.
    ``reader(frames)`` with uint8 [n_cameras,H,W,3] device frames -> (timestamps fp64 [n_cameras], status i32 [n_cameras]).
    ``sets``: up to four (geometry, checksums) pairs in the order they are tried."""

    def __init__(self, sets, n_cameras, swap_rb=False, device="cuda"):
        self.geometry, table = ops.pack_timestamp_sets(sets)
        self.device = torch.device(device)
        self.table = torch.from_numpy(table).to(self.device)
        self.prev = torch.zeros(int(n_cameras), dtype=torch.float64, device=self.device)
        self.swap_rb = bool(swap_rb)
        self.set_index = None

    def __call__(self, frames_u8):
        times, status, self.set_index, _, _, _ = ops.parse_frame_timestamps(frames_u8, (self.geometry, self.table), prev=self.prev,
                                                                              swap_rb=self.swap_rb)
        self.prev = times
        return times, status

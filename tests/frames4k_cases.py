"""4K frame intake (csrc/ts_parse.hip, csrc/ingest.hip: rn_parse_frame_timestamps, rn_frame_ingest_half): the numpy
restatement of both steps and the builders of the test cases.  CPU only, no torch.

Restated rules (one place each, as in the kernels):
  gray     (3735 B + 19235 G + 9798 R + 16384) >> 15 of a B,G,R pixel -- OpenCV's published 8-bit BGR2GRAY; white is gray > 127
  halving  (a + b + c + d + 2) >> 2 per channel of a 2x2 block -- OpenCV's resize for an exact 2x reduction of 8-bit data
Neither is pinned against cv2 (the package is absent); everything else of the time stamp reader -- slicing, the six areas,
the table search, the point at cell 10, the literal -- is pinned by tests/golden/frames4k.npz, which tools/make_golden.py
makes by running the reference's own parse_frame_timestamp on golden_cases() behind a cv2 stand-in made of the two rules above.

The font is synthetic: seven-segment digits scaled to the cell plus a digit-dependent run of marker pixels; every
(font, geometry) pair used must give ten pairwise different six-area checksums, which `table()` asserts.
"""
import collections

import numpy as np

GRAY_B, GRAY_G, GRAY_R, GRAY_ROUND, GRAY_SHIFT = 3735, 19235, 9798, 16384, 15
THRESHOLD = 127
READ, FAILED, FELL_BACK = 0, 1, 2
MAX_CELLS = 16
GEOMETRY_KEYS = ("x0", "y0", "w", "h", "n", "h13", "h23", "w12")


# ----------------------------------------------------------------------------- restatement: time stamps
def gray(pixels, swap_rb=False):
    """uint8 [...,3] -> int gray values; the channel order is B,G,R unless swap_rb."""
    p = pixels.astype(np.int64)
    b, g, r = (p[..., 2], p[..., 1], p[..., 0]) if swap_rb else (p[..., 0], p[..., 1], p[..., 2])
    return (GRAY_B * b + GRAY_G * g + GRAY_R * r + GRAY_ROUND) >> GRAY_SHIFT


def mask_strip(frame, geom, swap_rb=False):
    """The 0 / 255 threshold strip [h, n*w] of frame[y0:y0+h, x0:x0+n*w]; outside the frame it is dark."""
    x0, y0, w, h, n = (int(geom[k]) for k in ("x0", "y0", "w", "h", "n"))
    out = np.zeros((h, n * w), np.uint8)
    cut = frame[y0:y0 + h, x0:x0 + n * w]
    out[:cut.shape[0], :cut.shape[1]] = np.where(gray(cut, swap_rb) > THRESHOLD, 255, 0)
    return out


def six_counts(cell_mask, geom):
    h13, h23, w12 = int(geom["h13"]), int(geom["h23"]), int(geom["w12"])
    m = cell_mask != 0
    return [int(m[r, c].sum()) for r in (slice(0, h13), slice(h13, h23), slice(h23, None)) for c in (slice(0, w12), slice(w12, None))]


def read_set(frame, geom, table, swap_rb=False):
    """One (geometry, table) set on one frame -> (table index per cell [16] (-1: the point, beyond n, no equal entry),
    first failing cell or -1, mask strip)."""
    w, n = int(geom["w"]), int(geom["n"])
    strip = mask_strip(frame, geom, swap_rb)
    rows = [[int(v) for v in np.asarray(cs).reshape(6)] for cs in table.values()]
    idx, fail = [-1] * MAX_CELLS, -1
    for j in range(n):
        if j == 10:
            continue
        cs = six_counts(strip[:, j * w:(j + 1) * w], geom)
        hits = [k for k, row in enumerate(rows) if row == cs]
        if hits:
            idx[j] = hits[0]
        elif fail < 0:
            fail = j
    return idx, fail, strip


def value(keys, idx, n):
    """The digits as one integer over 10^max(n-11,0): one fp64 division of two exact operands."""
    D = 0
    for j in range(n):
        if j != 10:
            D = D * 10 + int(str(keys[idx[j]]))
    return np.float64(D) / np.float64(10 ** max(n - 11, 0))


def parse_frames(frames, sets, prev=None, swap_rb=False):
    """rn_parse_frame_timestamps restated.  frames: sequence of uint8 [H,W,3]; sets: (geometry, table) pairs.
    -> dict(times fp64 [B], status, set_index, digits i8 [B,16], fail_cell, mask uint8 [B,h,n*w] of the first set)."""
    B = len(frames)
    out = dict(times=np.zeros(B, np.float64), status=np.zeros(B, np.int32), set_index=np.full(B, -1, np.int32),
               digits=np.full((B, MAX_CELLS), -1, np.int8), fail_cell=np.full(B, -1, np.int32), mask=[])
    for b, frame in enumerate(frames):
        used = -1
        for g, (geom, table) in enumerate(sets):
            idx, fail, strip = read_set(frame, geom, table, swap_rb)
            if g == 0:
                out["mask"].append(strip)
                out["fail_cell"][b] = fail
                out["digits"][b] = idx
            if fail < 0:
                used = g
                out["digits"][b] = idx
                out["times"][b] = value(list(table.keys()), idx, int(geom["n"]))
                break
        out["set_index"][b] = used
        if used >= 0:
            out["status"][b] = READ
        elif prev is not None:
            out["status"][b] = FELL_BACK
            out["times"][b] = np.float64(prev[b]) + np.float64(1 / 30.0)
        else:
            out["status"][b] = FAILED
            out["times"][b] = np.nan
    out["mask"] = np.stack(out["mask"])
    return out


# ----------------------------------------------------------------------------- restatement: 2x reduction
def reduce_half(frames):
    """uint8 [B,2H,2W,3] -> uint8 [B,H,W,3]: (a + b + c + d + 2) >> 2 per channel of every 2x2 block."""
    f = frames.astype(np.int32)
    s = f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2]
    return ((s + 2) >> 2).astype(np.uint8)


# ----------------------------------------------------------------------------- the font
SEGMENTS = {0: "abcdef", 1: "bc", 2: "abged", 3: "abgcd", 4: "fgbc", 5: "afgcd", 6: "afgedc", 7: "abc", 8: "abcdefg", 9: "abfgcd"}


def glyph(d, w, h, font=0):
    """Digit d as a bool [h,w] mask: seven segments with a one-pixel margin on the right and at the bottom, plus a run of
    d + 1 marker pixels (font 0: along the bottom row from the left; font 1: down the right column from the top, and
    the segments mirrored left to right)."""
    m = np.zeros((h, w), bool)
    W, H = w - 1, h - 1                                                   # the drawn box
    mid = H // 2
    seg = dict(a=(slice(0, 1), slice(0, W)), g=(slice(mid, mid + 1), slice(0, W)), d=(slice(H - 1, H), slice(0, W)),
               f=(slice(0, mid + 1), slice(0, 1)), b=(slice(0, mid + 1), slice(W - 1, W)),
               e=(slice(mid, H), slice(0, 1)), c=(slice(mid, H), slice(W - 1, W)))
    for s in SEGMENTS[d]:
        m[seg[s]] = True
    if font == 1:
        m[:, :W] = m[:, :W][:, ::-1].copy()
    for k in range(d + 1):
        if font == 0:
            m[h - 1, k % w] = True
            if k >= w:
                m[h - 2 - (k - w) % (h - 2), w - 1] = True
        else:
            m[k % h, w - 1] = True
    return m


def point(w, h):
    m = np.zeros((h, w), bool)
    m[h - 2:, w // 2:w // 2 + 1] = True
    return m


def geometry(w, h, n, x0=0, y0=0, h13=None, h23=None, w12=None):
    """A geometry dict with the reference's keys (h12 is read by the reference and never used)."""
    return dict(x0=x0, y0=y0, w=w, h=h, n=n, h13=h // 3 if h13 is None else h13, h23=(2 * h) // 3 if h23 is None else h23,
                h12=h // 2, w12=w // 2 if w12 is None else w12)


def table(geom, font=0, order=None):
    """The checksum table of a font under a geometry, keyed by the int digit in `order` (default 0..9): key -> int 3x2.
    Asserts the condition of every case: ten pairwise different checksums."""
    w, h = int(geom["w"]), int(geom["h"])
    t = collections.OrderedDict()
    for d in (range(10) if order is None else order):
        t[d] = np.array(six_counts(glyph(d, w, h, font), geom), np.int64).reshape(3, 2)
    assert len(set(tuple(v.reshape(6)) for v in t.values())) == len(t), ("checksums collide", w, h, font)
    return t


def render(text, geom, H, W, font=0, fg=(255, 255, 255), bg=(0, 0, 0)):
    """A uint8 [H,W,3] B,G,R frame of colour bg carrying `text` (n characters, '.' at index 10) in colour fg at the geometry's
    strip; what falls outside the frame is cut off."""
    x0, y0, w, h, n = (int(geom[k]) for k in ("x0", "y0", "w", "h", "n"))
    assert len(text) == n and all((ch == ".") == (j == 10) for j, ch in enumerate(text)), text
    strip = np.concatenate([point(w, h) if ch == "." else glyph(int(ch), w, h, font) for ch in text], axis=1)
    frame = np.empty((H, W, 3), np.uint8)
    frame[:] = np.array(bg, np.uint8)
    ys, xs = np.nonzero(strip)
    keep = (ys + y0 < H) & (xs + x0 < W)
    frame[ys[keep] + y0, xs[keep] + x0] = np.array(fg, np.uint8)
    return frame


def stamp_text(digits, n):
    """The first n - (n > 10) digits of `digits` with the point put at index 10."""
    k = n - 1 if n > 10 else n
    s = "".join(str(int(d)) for d in digits[:k])
    return s if n <= 10 else s[:10] + "." + s[10:]


def rng_bytes(shape, seed):
    """Deterministic bytes (a 64-bit LCG's high byte), independent of numpy's generators."""
    n = int(np.prod(shape))
    out = np.empty(n, np.uint8)
    x = (seed * 0x9E3779B97F4A7C15 + 0x1234567) % (1 << 64)
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out[i] = x >> 56
    return out.reshape(shape)


def random_digits(count, k, seed):
    """[count, k] decimal digits, the first of each row 1-9 (a leading zero is no Python literal)."""
    d = rng_bytes((count, k), seed).astype(np.int64) * 10 // 256
    d[:, 0] = 1 + d[:, 0] * 9 // 10
    return d


def edge_colours():
    """B,G,R triples with unequal channels whose gray is exactly 127 and exactly 128, as close to the rule's rounding
    boundary as a triple with B = 40 comes: (the largest sum below 128 << 15, the smallest at or above it)."""
    g, r = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    s = GRAY_B * 40 + GRAY_G * g + GRAY_R * r + GRAY_ROUND
    edge = (THRESHOLD + 1) << GRAY_SHIFT
    ok = (g != r) & (g != 40) & (r != 40)
    lo = np.where(ok & (s < edge), s, -1).argmax()
    hi = np.where(ok & (s >= edge), s, 1 << 40).argmin()
    dark, white = (40, int(g.flat[lo]), int(r.flat[lo])), (40, int(g.flat[hi]), int(r.flat[hi]))
    assert gray(np.array(dark, np.uint8)) == THRESHOLD and gray(np.array(white, np.uint8)) == THRESHOLD + 1
    return dark, white


# ----------------------------------------------------------------------------- the cases the reference runs (golden)
G59 = dict(w=5, h=9)
G711 = dict(w=7, h=11)
DIGITS = [1, 6, 2, 0, 3, 9, 8, 4, 5, 7, 2, 5, 0, 9, 3, 1]


def _case(name, frame, geom, tab):
    return dict(name=name, frame=frame, geom=geom, table=tab)


def golden_cases():
    """Ordered list of dict(name, frame uint8 [H,W,3], geom, table): one reference call each."""
    cases = []
    for cell in (G59, G711):
        for n in (10, 11, 13, 16):
            # inside a larger frame, odd x0: the strip's byte offset is no multiple of 4
            geom = geometry(cell["w"], cell["h"], n, x0=7, y0=3)
            cases.append(_case("in_%dx%d_n%d" % (cell["w"], cell["h"], n),
                               render(stamp_text(DIGITS, n), geom, cell["h"] + 9, 7 + n * cell["w"] + 6), geom, table(geom)))
    geom = geometry(7, 11, 13, x0=5, y0=4)
    text = stamp_text(DIGITS, 13)
    cases.append(_case("edge_exact", render(text, geom, 4 + 11, 5 + 13 * 7), geom, table(geom)))
    cases.append(_case("edge_past_right", render(text, geom, 4 + 11, 5 + 13 * 7 - 3), geom, table(geom)))
    cases.append(_case("edge_past_bottom", render(text, geom, 4 + 11 - 2, 5 + 13 * 7), geom, table(geom)))
    geom = geometry(7, 11, 13, x0=1, y0=0, h13=0, w12=7)                   # empty areas: the top band and the right halves
    cases.append(_case("empty_areas", render(text, geom, 12, 96), geom, table(geom)))
    geom = geometry(7, 11, 13, x0=3, y0=2)
    tab = table(geom)
    good = render(text, geom, 16, 100)
    noisy = good.copy()
    noisy[2:13, 3 + 70:3 + 77] = rng_bytes((11, 7, 3), 5)                  # cell 10 is never looked at
    cases.append(_case("noise_in_point", noisy, geom, tab))
    for name, cells in (("flip_cell3", (3,)), ("flip_cell12", (12,)), ("flip_cells_5_8", (8, 5))):
        bad = good.copy()
        for j in cells:
            y, x = 2 + 4, 3 + 7 * j + 3                                      # inside the drawn box, off every segment
            bad[y, x] = 255 - bad[y, x]
        cases.append(_case(name, bad, geom, tab))
    twice = collections.OrderedDict()                                       # entries 2 and 5 hold the same counts: the lower index
    for k, d in enumerate((7, 3, 1, 0, 9, 1, 2, 4, 5, 6, 8)):              # wins, so glyph 1 reads as 1 and not as "4"
        twice[d if k != 5 else "4"] = tab[d]
    cases.append(_case("duplicate_entry", good, geom, twice))
    dark, white = edge_colours()
    cases.append(_case("gray_127_128", render(text, geom, 16, 100, fg=white, bg=dark), geom, tab))
    cases.append(_case("gray_128_127", render(text, geom, 16, 100, fg=dark, bg=white), geom, tab))  # inverted: nothing matches
    return cases


def save_golden(path, results):
    """results: per case (time or None, error pixels or None), from the reference.  Writes inputs and results, data only."""
    out = {}
    for c, (t, err) in zip(golden_cases(), results):
        g, tag = c["geom"], c["name"] + "_"
        out[tag + "frame"] = c["frame"]
        out[tag + "geom"] = np.array([g[k] for k in GEOMETRY_KEYS + ("h12",)], np.int32)
        out[tag + "keys"] = np.array([str(k) for k in c["table"].keys()])
        out[tag + "table"] = np.stack([np.asarray(v, np.int64).reshape(6) for v in c["table"].values()])
        out[tag + "time"] = np.array(np.nan if t is None else float(t), np.float64)
        out[tag + "is_int"] = np.array(isinstance(t, int))
        pix = np.zeros((g["h"], g["w"]), np.uint8)                          # the reference's pixels are clipped at the frame's edge: padded dark
        if err is not None:
            pix[:err.shape[0], :err.shape[1]] = err
        out[tag + "err"] = pix
        out[tag + "failed"] = np.array(t is None)
    np.savez_compressed(path, **out)


# ----------------------------------------------------------------------------- 2x reduction inputs
def residue_blocks(H2, W2):
    """uint8 [1,H2,W2,3] whose 2x2 block sums run through 0..6 and 1014..1020 (every residue mod 4 at both ends of the
    range) and repeat; the three channels are shifted against each other."""
    sums = list(range(0, 7)) + list(range(1014, 1021))
    f = np.zeros((1, H2, W2, 3), np.uint8)
    k = 0
    for y in range(0, H2, 2):
        for x in range(0, W2, 2):
            for c in range(3):
                s = sums[(k + 5 * c) % len(sums)]
                q, r = divmod(s, 4)
                vals = [q + (i < r) for i in range(4)]
                vals = vals[k % 4:] + vals[:k % 4]
                f[0, y, x, c], f[0, y, x + 1, c], f[0, y + 1, x, c], f[0, y + 1, x + 1, c] = vals
            k += 1
    return f

"""The drawing rules of csrc/render.hip and mc3d_render.py restated plainly in numpy (integer rules in int64 / Python ints,
the compose pass in np.float32 with one operation per line), and the cases of tests/test_render_host.py and
tests/test_gpu_render.py.  Nothing here imports the code under test except the constants a caller passes in."""
import math

import numpy as np

F32 = np.float32
EDGES = ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (2, 7), (3, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))
BIT = dict(prior=0, crop_edge=1, track=2, det=3, in_crop=4, label=5, label_text=6, banner_edge=7, banner_text=8)
LO, HI = -8192, 8191
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PRIOR, TRACK, DET = (255.0, 255.0, 0.0), (0.0, 200.0, 25.0), (255.0, 0.0, 0.0)


def new_mask(n_cam, H, W):
    return np.zeros((n_cam, H, W), np.uint16)


def trunc(v):
    """int(v) when v is finite and int(v) lies in [LO, HI], else None."""
    v = float(v)
    if not math.isfinite(v):
        return None
    t = int(v)
    return t if LO <= t <= HI else None


# ------------------------------------------------------------------------------------------------ edges
def segment_cover(xs, ys, ax, ay, bx, by, t):
    """4 d^2 <= t^2 for the pixels (xs, ys) (int64 arrays) against the segment A-B, without division."""
    ex, ey = bx - ax, by - ay
    wx, wy = xs - ax, ys - ay
    len2 = ex * ex + ey * ey
    dot = wx * ex + wy * ey
    at_a = 4 * (wx * wx + wy * wy) <= t * t
    ux, uy = xs - bx, ys - by
    at_b = 4 * (ux * ux + uy * uy) <= t * t
    cross = wx * ey - wy * ex
    inside = 4 * cross * cross <= t * t * len2
    if len2 == 0:
        return at_a
    return np.where(dot <= 0, at_a, np.where(dot >= len2, at_b, inside))


def paint_edges(mask, corners, cam, thickness, bit):
    """Every pixel of the edge's bounding box, widened by the thickness and clipped to the frame, is put to the rule (a pixel
    further out is more than thickness away from the segment)."""
    n_cam, H, W = mask.shape
    t = int(thickness)
    for box, c in zip(np.asarray(corners, np.float64).reshape(-1, 8, 2), np.asarray(cam).reshape(-1)):
        if not 0 <= int(c) < n_cam:
            continue
        for a, b in EDGES:
            pts = [trunc(box[a, 0]), trunc(box[a, 1]), trunc(box[b, 0]), trunc(box[b, 1])]
            if None in pts:
                continue                                   # the whole edge is skipped
            x0, x1 = max(min(pts[0], pts[2]) - t, 0), min(max(pts[0], pts[2]) + t + 1, W)
            y0, y1 = max(min(pts[1], pts[3]) - t, 0), min(max(pts[1], pts[3]) + t + 1, H)
            if x0 >= x1 or y0 >= y1:
                continue
            ys, xs = np.meshgrid(np.arange(y0, y1, dtype=np.int64), np.arange(x0, x1, dtype=np.int64), indexing="ij")
            mask[int(c), y0:y1, x0:x1][segment_cover(xs, ys, *pts, t)] |= np.uint16(1 << bit)
    return mask


# ------------------------------------------------------------------------------------------------ rectangles and text
def anchor_of(box):
    """(int(min x), int(max y)) of a box's eight corners; None when a corner is not finite or out of range."""
    box = np.asarray(box, np.float64).reshape(8, 2)
    if any(trunc(v) is None for v in box.reshape(-1)):
        return None
    return trunc(box[:, 0].min()), trunc(box[:, 1].max())


def _origin(x, y, anchor, anchors):
    if anchor < 0:
        return int(x), int(y)
    if anchors is None or anchor >= len(anchors):
        return None
    o = anchor_of(anchors[anchor])
    return None if o is None else (int(x) + o[0], int(y) + o[1])


def paint_rects(mask, rects, anchors=None):
    """rects [n,8]: x0, y0, x1, y1, cam, mode, anchor, bit."""
    n_cam, H, W = mask.shape
    for x0, y0, x1, y1, c, mode, anchor, bit in np.asarray(rects, np.int64).reshape(-1, 8).tolist():
        if not 0 <= c < n_cam:
            continue
        o = _origin(0, 0, anchor, anchors)
        if o is None:
            continue
        x0, x1, y0, y1 = x0 + o[0], x1 + o[0], y0 + o[1], y1 + o[1]
        for y in range(max(y0, 0), min(y1, H)):
            for x in range(max(x0, 0), min(x1, W)):
                if mode == 0 or y in (y0, y1 - 1) or x in (x0, x1 - 1):
                    mask[c, y, x] |= np.uint16(1 << bit)
    return mask


def glyph_pixel(text, font, s, px, py):
    """Is (px, py), relative to the run's upper left corner, a glyph pixel of the run at scale s?"""
    if px < 0 or py < 0 or py >= 8 * s or px >= 6 * s * len(text):
        return False
    i = px // (6 * s)
    ch = int(text[i])
    if not 32 <= ch <= 126:
        ch = ord("?")
    col, row = (px - 6 * s * i) // s, py // s
    return bool((int(font[ch - 32][row]) >> (5 - col)) & 1)


def paint_text(mask, runs, text, font, anchors=None):
    """runs [n,9]: x, y, cam, anchor, scale, dilate, bit, start, length over the bytes of ``text``."""
    n_cam, H, W = mask.shape
    for x, y, c, anchor, s, dil, bit, start, length in np.asarray(runs, np.int64).reshape(-1, 9).tolist():
        if not 0 <= c < n_cam or length <= 0:
            continue
        o = _origin(x, y, anchor, anchors)
        if o is None:
            continue
        left, top = o[0], o[1] - 8 * s
        chars = text[start:start + length]
        for py in range(max(top - dil, 0), min(o[1] + dil, H)):
            for px in range(max(left - dil, 0), min(left + 6 * s * length + dil, W)):
                if any(glyph_pixel(chars, font, s, px - left + u, py - top + v) for v in range(-dil, dil + 1) for u in range(-dil, dil + 1)):
                    mask[c, py, px] |= np.uint16(1 << bit)
    return mask


# ------------------------------------------------------------------------------------------------ compose
def compose(frames, mask, crops_present, cols, mean=MEAN, std=STD):
    """frames fp32 [n,3,H,W], mask uint16 [n,H,W] -> uint8 [rows*H, cols*W, 3].  np.float32, one operation per line."""
    frames = np.asarray(frames, F32)
    n, _, H, W = frames.shape
    rows = -(-n // cols)
    out = np.zeros((rows * H, cols * W, 3), np.uint8)
    m = np.asarray(mask).astype(np.int64)

    def has(name):
        return (m >> BIT[name]) & 1 == 1
    for ch in range(3):
        x = frames[:, ch]
        t = x * F32(std[ch])
        t = t + F32(mean[ch])
        t = t * F32(255)
        t = t + F32(0.5)
        t = np.floor(t)
        t = np.minimum(np.maximum(t, F32(0)), F32(255))
        v = t / F32(255)
        v = np.where(has("prior"), F32(PRIOR[ch]), v)
        v = np.where(has("crop_edge"), F32(255), v)
        v = np.where(has("track"), F32(TRACK[ch]), v)
        v = np.where(has("det"), F32(DET[ch]), v)
        if crops_present:
            dimmed = F32(0.3) * v
            v = np.where(has("in_crop"), v, dimmed)
        a = np.where(has("label_text"), F32(0), v)
        b = np.where(has("label_text"), F32(0), np.where(has("label"), F32(1), v))
        a7 = F32(0.7) * a
        b3 = F32(0.3) * b
        blend = a7 + b3
        v = np.where(has("label") | has("label_text"), blend, v)
        v = np.where(has("banner_edge"), F32(1), v)
        v = np.where(has("banner_text"), F32(0), v)
        v = np.minimum(np.maximum(v, F32(0)), F32(1))
        v = v * F32(255)
        v = v + F32(0.5)
        assert v.dtype == F32
        byte = v.astype(np.uint8)                              # truncation
        for i in range(n):
            r, c = i // cols, i % cols
            out[r * H:(r + 1) * H, c * W:(c + 1) * W, ch] = byte[i]
    return out


def layout(n):
    rows = int(np.round(np.sqrt(n)))
    return rows, int(math.ceil(n / rows))


def render_restated(n_cam, H, W, font, frames, tracks=None, detections=None, priors=None, crops=None, labels=None, banners=None,
                    fancy_crop=True):
    """``mc3d_render.Renderer.render`` from its arguments (numpy): the reference's layers (MC3D_crop_tracker.py:764-891) in
    the geometry of DESIGN.md 4.8 (6x8 cells, 12-pixel lines, the banner at (20, 30) and scale 2).  Line weights 1 / 3 / 1 for priors / tracks / detections; labels [(box, cam, [lines])]."""
    mask = new_mask(n_cam, H, W)
    for pair, thick, bit in ((priors, 1, "prior"), (tracks, 3, "track"), (detections, 1, "det")):
        if pair is not None:
            paint_edges(mask, pair[0], pair[1], thick, BIT[bit])
    if crops is not None:
        for box, c in zip(np.asarray(crops[0]).astype(np.int32).reshape(-1, 4).tolist(), np.asarray(crops[1]).reshape(-1).tolist()):
            if fancy_crop:
                paint_rects(mask, [box + [c, 0, -1, BIT["in_crop"]]])
            else:
                paint_rects(mask, [[box[0], box[1], box[2] + 1, box[3] + 1, c, 1, -1, BIT["crop_edge"]]])
    anchors = None if tracks is None else np.asarray(tracks[0], np.float64).reshape(-1, 8, 2)
    for box, c, lines in (labels or []) if tracks is not None else []:
        if not lines:
            continue
        longest = max(len(line) for line in lines)
        paint_rects(mask, [[0, 0, 6 * longest + 10 + 1, 12 * len(lines) + 1, c, 0, box, BIT["label"]]], anchors)
        for k, line in enumerate(lines):
            raw = line.encode("latin-1", "replace")
            paint_text(mask, [[0, 12 * (k + 1), c, box, 1, 0, BIT["label_text"], 0, len(raw)]], raw, font, anchors)
    for c, line in enumerate(banners or []):
        raw = line.encode("latin-1", "replace")
        paint_text(mask, [[20, 30, c, -1, 2, 1, BIT["banner_edge"], 0, len(raw)]], raw, font)
        paint_text(mask, [[20, 30, c, -1, 2, 0, BIT["banner_text"], 0, len(raw)]], raw, font)
    return compose(frames, mask, crops is not None and fancy_crop, layout(n_cam)[1]), mask


# ------------------------------------------------------------------------------------------------ cases
EDGE_SHAPE = (3, 37, 67)                       # odd both ways: the two-pixel mask words straddle rows and cameras


def octant(ax, ay, bx, by):
    """0..7 for a segment that is neither axis-parallel nor diagonal, else None."""
    dx, dy = bx - ax, by - ay
    if dx == 0 or dy == 0 or abs(dx) == abs(dy):
        return None
    return (dx > 0) * 4 + (dy > 0) * 2 + (abs(dx) > abs(dy))


def edges_case():
    """(corners [n,8,2], cam [n], notes): boxes for EDGE_SHAPE.  Cameras 0 and 2 are drawn into, camera 1 receives nothing;
    one box names a camera that does not exist."""
    n_cam, H, W = EDGE_SHAPE
    rs = np.random.RandomState(7)
    boxes, cams = [], []

    def add(box, cam):
        boxes.append(np.asarray(box, np.float64).reshape(8, 2))
        cams.append(cam)
    for k in range(6):                                                   # scattered corners, some off every side
        add(np.stack((rs.uniform(-12, W + 12, 8), rs.uniform(-12, H + 12, 8)), 1), 0 if k % 2 == 0 else 2)
    add([[10, 5], [40, 5], [10, 30], [40, 30], [10, 5], [40, 5], [10, 30], [40, 30]], 0)       # horizontal, vertical, zero length
    add([[20.2, 20.9]] * 8, 2)                                           # every edge is a disc
    add([[-0.7, -0.7], [66.9, -0.7], [-0.7, 36.9], [66.9, 36.9], [-0.7, 10.5], [66.9, 10.5], [-0.7, 30.2], [66.9, 30.2]], 2)   # truncation
    add([[-30, 18], [100, 20], [33, -25], [35, 70], [-20, -20], [90, 60], [-15, 50], [80, -10]], 0)   # ends off every side
    bad = np.stack((rs.uniform(5, W - 5, 8), rs.uniform(5, H - 5, 8)), 1)
    for corner, value in ((5, np.nan), (0, np.inf), (6, 9000.0), (3, -9000.0)):
        b = bad.copy()
        b[corner, corner % 2] = value                                    # only the edges at that corner vanish
        add(b, 0 if corner % 2 else 2)
    shared = np.stack((rs.uniform(0, W, 8), rs.uniform(0, H, 8)), 1)
    add(shared, 2)
    add(shared + 0.4, 2)                                                 # two boxes sharing pixels
    add(shared, 7)                                                       # no such camera
    corners, cam = np.stack(boxes), np.asarray(cams, np.int32)
    seen = set()
    for box in corners:
        for a, b in EDGES:
            pts = [trunc(box[a, 0]), trunc(box[a, 1]), trunc(box[b, 0]), trunc(box[b, 1])]
            if None not in pts:
                seen.add(octant(*pts))
    assert seen >= set(range(8)), seen
    return corners, cam


def rects_case():
    """(rects, anchors) for EDGE_SHAPE: over the border, empty, inverted, off-frame, anchored (also to a bad box), outline."""
    anchors = np.array([[[12.5, 9.0], [30.0, 8.0], [14.0, 20.7], [31.0, 22.0], [12.9, 3.0], [30.0, 2.0], [14.0, 14.0], [31.0, 15.0]],
                        [[np.nan, 9.0]] + [[20.0, 10.0]] * 7,
                        [[60.3, 30.0], [70.0, 31.0], [61.0, 33.9], [71.0, 34.0], [60.9, 25.0], [70.0, 26.0], [61.0, 28.0], [71.0, 29.0]]])
    rects = [[-5, -4, 9, 6, 0, 0, -1, 4], [60, 30, 80, 50, 0, 0, -1, 4], [5, 5, 5, 9, 0, 0, -1, 5], [9, 9, 4, 12, 0, 0, -1, 5],
             [70, 5, 80, 9, 0, 0, -1, 5], [3, 40, 9, 50, 0, 0, -1, 5], [0, 0, 20, 11, 0, 0, 0, 5], [0, 0, 20, 11, 2, 0, 1, 5],
             [0, 0, 30, 13, 2, 0, 2, 5], [20, 10, 41, 25, 2, 1, -1, 1], [-3, 30, 4, 40, 2, 1, -1, 1], [1, 1, 2, 2, 1, 1, -1, 7],
             [0, 0, 67, 37, 1, 1, -1, 15], [33, 0, 34, 37, 1, 0, -1, 0], [2, 2, 9, 9, 5, 0, -1, 3], [-2, -9, 5, 3, 0, 1, 0, 6]]
    return np.asarray(rects, np.int32), anchors


TEXT_SHAPE = (3, 45, 203)


def text_case():
    """(runs, text, anchors) for TEXT_SHAPE: every byte once at scale 1 in rows of 32 over cameras 0 and 1; scale 2 with and
    without dilation, runs clipped right and bottom, anchored runs and a run anchored to a bad box in camera 2."""
    text = bytes(range(256)) + b"Clipped at the right edge" + b"gjpqy|_" + b"anchored"
    runs = []
    for k in range(8):
        runs.append([3 + k, 9 + 9 * (k % 4), k // 4, -1, 1, 0, BIT["label_text"], 32 * k, 32])
    runs.append([100, 17, 2, -1, 2, 1, BIT["banner_edge"], 256, 25])     # clipped right, dilated
    runs.append([100, 17, 2, -1, 2, 0, BIT["banner_text"], 256, 25])
    runs.append([-4, 52, 2, -1, 2, 1, BIT["banner_edge"], 281, 7])       # clipped left and bottom
    runs.append([2, 30, 2, -1, 1, 1, 9, 281, 7])
    runs.append([0, 12, 2, 0, 1, 0, BIT["label_text"], 288, 8])          # anchored
    runs.append([0, 12, 2, 1, 1, 0, BIT["label_text"], 288, 8])          # anchored to a box with a NaN corner: nothing
    runs.append([5, 9, 1, -1, 3, 0, 10, 40, 0])                          # empty
    anchors = np.array([[[120.7, 20.0], [150.0, 21.0], [125.0, 27.9], [151.0, 26.0]] * 2, [[np.nan, 1.0]] * 8])
    return np.asarray(runs, np.int32), np.frombuffer(text, np.uint8), anchors


def all_masks(n_cam, H, W, seed):
    """A mask plane holding each of the 512 combinations of the nine layer bits at least once, shuffled."""
    n = n_cam * H * W
    assert n >= 512
    rs = np.random.RandomState(seed)
    m = np.concatenate((np.arange(512), rs.randint(0, 512, n - 512)))
    return rs.permutation(m).astype(np.uint16).reshape(n_cam, H, W)


def random_frames(n_cam, H, W, seed):
    """Normalised frames that leave [0, 255] on both sides after the inverse of the ingest, so that the clamp is met."""
    return np.random.RandomState(seed).uniform(-2.4, 2.9, (n_cam, 3, H, W)).astype(F32)

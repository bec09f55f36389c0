"""The replay of a tracking CSV over camera frames (3d-playground_amd/datareader.py: Camera_Wrapper, test_integrity, plot_in;
mc3d_render.Replayer; csrc/replay.hip) restated plainly in numpy and Python, and the cases of tests/test_replay_host.py and
tests/test_gpu_replay.py.  Reference: datareader.py:24-89, 253-399, 586-653.

  walk                   the loop of plot_in over scripted camera time stamps: label instants, camera stamps, dt
  shift / boxes          the constant-velocity shift in np.float32 and the projection through oracle/homography.py
  label_lines / layout   plot_labels' strings, the column-major tile of a camera
  compose_pixels / canvas / resample / compose
                         the integer layers, the mosaic and the project's own integer bilinear rule
  paint / replay_frame   one output frame painted with render_cases' painters from given image corners
  absdiff / running      the window sum of test_integrity and the fp64 running frame
  integrity              test_integrity's loop over scripted stamps and frames
Held to the reference's own plot_in by tests/golden/replay.npz (tools/make_golden_replay.py).  Nothing here imports the code
under test except constants a caller passes in."""
import math

import numpy as np

import datareader_cases as dc
import render_cases as rc

BIT = dict(primary=0, secondary=1, label=2, label_text=3)
PRIMARY, SECONDARY = (0, 0, 255), (0, 255, 0)          # RGB; the reference's BGR (255,0,0) and (0,255,0)
THICKNESS = 2
RTOL, ATOL = 1e-9, 1e-8                                 # the project's projection bound (tests/test_gpu_datareader.py)

# the golden scene: three cameras, the third without an entry in the file's ts_bias (the KeyError branch)
GOLDEN_CAMERAS = ("p1c1", "p1c3", "p2c1")
GOLDEN_CSV = dict(seed=21, n_frames=12, n_objs=6, n_cams=3)


# ------------------------------------------------------------------------------------------------ the loop
class ScriptedCamera:
    """What plot_in needs of a Camera_Wrapper: ``name``, ``ts``, ``__next__`` over a list of stamps."""

    def __init__(self, name, stamps):
        self.name, self.stamps, self.k, self.ts = name, [float(s) for s in stamps], 0, None

    def __next__(self):
        if self.k >= len(self.stamps):
            raise StopIteration
        self.ts = self.stamps[self.k]
        self.k += 1


def script(data, n=40):
    """Camera stamps [3, n] for a loaded file: camera 0 leads and jumps 0.13 s (over two label instants) after its fifth frame;
    camera 1 starts 0.08 s behind (it lags by more than 1/60 s and is advanced several times at once); camera 2 runs at
    another rate.  Long enough that the labels run out first."""
    t0 = float(dc._first_ts(data[0]))
    a = [t0 + 0.004 + k / 30.0 + (0.13 if k >= 5 else 0.0) for k in range(n)]
    b = [t0 - 0.08 + k / 30.0 for k in range(n)]
    c = [t0 + 0.011 + k / 25.0 for k in range(n)]
    return np.array([a, b, c], np.float64)


def walk(data, cameras, max_frames=None):
    """plot_in :308-399 over ``cameras`` (each already holding its first stamp) -> [(label instant, [camera ts], [dt])]."""
    def label(i):
        nxt = dc._first_ts(data[i + 1]) if i + 1 < len(data) else None
        return data[i], dc._first_ts(data[i]), nxt
    i = 0
    ts_data, ts, next_ts = label(i)
    out = []
    try:
        while max_frames is None or len(out) < max_frames:
            max_time = max(cam.ts for cam in cameras)
            for cam in cameras:
                while cam.ts + 1 / 60.0 < max_time:
                    next(cam)
            if next_ts is None:
                break
            while max_time > next_ts:
                i += 1
                ts_data, ts, next_ts = label(i)
                if next_ts is None:
                    break
            first = ts_data[next(iter(ts_data))]
            dts = [cam.ts + first["ts_bias"].get(cam.name, 0) - ts for cam in cameras]
            out.append((i, [cam.ts for cam in cameras], dts))
            next(cameras[0])
    except StopIteration:
        pass
    return out


# ------------------------------------------------------------------------------------------------ boxes and labels
def state7(frame):
    """:338 -> fp32 [n,7] = (x, y, l, w, h, direction, v) of a label instant's objects, in dict order."""
    return np.array([[o["x"], o["y"], o["l"], o["w"], o["h"], o["direction"], o["v"]] for o in frame.values()],
                    np.float64).reshape(-1, 7).astype(np.float32)


def shift(st, dt):
    """:345 in torch's fp32 arithmetic: the Python scalar enters as fp32; one rounding per operation, left to right."""
    st = np.array(st, np.float32)
    s = st[:, 6] * np.float32(dt)
    s = s * st[:, 5]
    st[:, 0] = st[:, 0] + s
    return st


def boxes(st, dts, names, all_names, P, P2=None):
    """rn_replay_boxes restated -> (views fp32 [C*n,7], corners fp64 [C*n,8,2], side int32, cam int32)."""
    n = len(st)
    views = np.concatenate([shift(st, dt) for dt in dts]).reshape(-1, 7)
    cam = np.repeat(np.arange(len(dts), dtype=np.int32), n)
    _, im, _ = dc.project(views, [names[c] for c in cam], list(all_names), P, P2)
    return views, im.reshape(-1, 8, 2), (views[:, 1] > np.float32(60)).astype(np.int32), cam


def label_lines(view, cls, oid, time):
    """plot_labels :262-268; the numbers are fp32 tensor elements there."""
    return ["{} {}:".format(cls, oid), "L: {:.1f}ft".format(float(np.float32(view[2]))), "W: {:.1f}ft".format(float(np.float32(view[3]))),
            "H: {:.1f}ft".format(float(np.float32(view[4]))), "{}".format(time)]


def frame_lines(frame, st, ts, dts):
    """[camera][object] -> the five lines."""
    return [[label_lines(st[i], o["class"], o["id"], ts + dt) for i, o in enumerate(frame.values())] for dt in dts]


def layout(n):
    rows = int(np.round(np.sqrt(n)))
    return rows, int(math.ceil(n / rows))


def tile_of(i, n):
    """(tile row, tile column) of camera i of n: column-major, as :371-374 index their canvas."""
    rows, _ = layout(n)
    return i % rows, i // rows


# ------------------------------------------------------------------------------------------------ compose
def compose_pixels(frames, mask, swap_rb=False):
    """uint8 [C,H,W,3] + mask -> composed RGB int64 [C,H,W,3]; layers lowest to highest, integers."""
    v = np.asarray(frames).astype(np.int64)
    if swap_rb:
        v = v[..., ::-1].copy()
    m = np.asarray(mask).astype(np.int64)

    def has(name):
        return ((m >> BIT[name]) & 1 == 1)[..., None]
    v = np.where(has("primary"), np.array(PRIMARY, np.int64), v)
    v = np.where(has("secondary"), np.array(SECONDARY, np.int64), v)
    v = np.where(has("label"), (7 * v + 3 * 255 + 5) // 10, v)
    v = np.where(has("label_text"), 0, v)
    return v


def canvas(pixels):
    """[C,H,W,3] -> the canvas [rows*H, cols*W, 3]; unused tiles zero."""
    C, H, W, _ = pixels.shape
    rows, cols = layout(C)
    out = np.zeros((rows * H, cols * W, 3), np.int64)
    for i in range(C):
        r, c = tile_of(i, C)
        out[r * H:(r + 1) * H, c * W:(c + 1) * W] = pixels[i]
    return out


def axis_taps(O, S):
    """Per output index of O samples over S: (i0, i1, w0, w1) with w0 + w1 = 2 O, in Python integers."""
    i0, i1, w0, w1 = [], [], [], []
    for X in range(O):
        num = min(max((2 * X + 1) * S - O, 0), 2 * O * (S - 1))
        a = num // (2 * O)
        i0.append(a)
        i1.append(min(a + 1, S - 1))
        w1.append(num - 2 * O * a)
        w0.append(2 * O - w1[-1])
    return (np.array(v, np.int64) for v in (i0, i1, w0, w1))


def resample(cv, OW, OH):
    """The project's bilinear rule with half-pixel centres in exact integers: [CH,CW,3] int64 -> uint8 [OH,OW,3]."""
    CH, CW, _ = cv.shape
    x0, x1, wx0, wx1 = axis_taps(OW, CW)
    y0, y1, wy0, wy1 = axis_taps(OH, CH)
    assert 4 * OW * OH * 255 + 2 * OW * OH < 2 ** 63
    s = (wy0[:, None, None] * (wx0[None, :, None] * cv[y0][:, x0] + wx1[None, :, None] * cv[y0][:, x1]) +
         wy1[:, None, None] * (wx0[None, :, None] * cv[y1][:, x0] + wx1[None, :, None] * cv[y1][:, x1]))
    return ((s + 2 * OW * OH) // (4 * OW * OH)).astype(np.uint8)


def compose(frames, mask, size=None, swap_rb=False):
    cv = canvas(compose_pixels(frames, mask, swap_rb))
    return cv.astype(np.uint8) if size is None else resample(cv, int(size[0]), int(size[1]))


def paint(n_cam, H, W, font, corners, side, cam, lines):
    """The replay's mask plane from image corners [C*n,8,2]: boxes by side, then every label block (rectangle c1 .. c1 + (6 L
    + 10, 12 lines) inclusive, line k on the baseline c1.y + 12 k), anchored at box c * n + i."""
    mask = rc.new_mask(n_cam, H, W)
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 2)
    side, cam = np.asarray(side).reshape(-1), np.asarray(cam).reshape(-1)
    rc.paint_edges(mask, corners[side == 0], cam[side == 0], THICKNESS, BIT["primary"])
    rc.paint_edges(mask, corners[side != 0], cam[side != 0], THICKNESS, BIT["secondary"])
    for c, per_cam in enumerate(lines):
        n = len(per_cam)
        for i, ls in enumerate(per_cam):
            longest = max(len(line) for line in ls)
            rc.paint_rects(mask, [[0, 0, 6 * longest + 10 + 1, 12 * len(ls) + 1, c, 0, c * n + i, BIT["label"]]], corners)
            for k, line in enumerate(ls):
                raw = line.encode("latin-1", "replace")
                rc.paint_text(mask, [[0, 12 * (k + 1), c, c * n + i, 1, 0, BIT["label_text"], 0, len(raw)]], raw, font, corners)
    return mask


def replay_frame(frames, font, corners, side, cam, lines, size=None, swap_rb=False):
    C, H, W, _ = np.asarray(frames).shape
    return compose(frames, paint(C, H, W, font, corners, side, cam, lines), size, swap_rb)


# ------------------------------------------------------------------------------------------------ integrity and running frame
def window(H, W, y0=100, y1=500, x0=100, x1=500):
    return max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)


def absdiff(a, b, y0=100, y1=500, x0=100, x1=500):
    y0, y1, x0, x1 = window(a.shape[0], a.shape[1], y0, y1, x0, x1)
    if y0 >= y1 or x0 >= x1:
        return 0
    return int(np.abs(a[y0:y1, x0:x1].astype(np.int64) - b[y0:y1, x0:x1].astype(np.int64)).sum())


def doubled(a, b):
    """:617 -> np.mean(|a - b| over the window) < 0.2, numpy as the reference calls it; an empty window is never doubled."""
    y0, y1, x0, x1 = window(a.shape[0], a.shape[1])
    if y0 >= y1 or x0 >= x1:
        return False
    return bool(np.mean(np.abs(a[y0:y1, x0:x1, :].astype(float) - b[y0:y1, x0:x1, :].astype(float))) < 0.2)


def running(frames):
    """:74-77 over a list of uint8 frames -> the fp64 running frame after each."""
    out, r = [], None
    for f in frames:
        r = f.astype(np.float64) if r is None else 0.95 * r + 0.05 * f
        out.append(np.array(r, np.float64))
    return out


def integrity(stamps, frames, n=1000):
    """test_integrity :593-645 over scripted (stamp, frame) pairs -> the five counts."""
    counts = dict(doubled_ts=0, doubled_frame=0, doubled_both=0, skipped_ts=0, correct=0)
    k = 0
    prev_ts, prev = stamps[0], frames[0]
    for i in range(1, n):
        k += 1
        if k >= len(stamps):
            break
        ts, frame = stamps[k], frames[k]
        DTS, DF = ts - prev_ts == 0, doubled(frame, prev)
        STS = False
        if DTS and DF:
            counts["doubled_both"] += 1
        elif DTS:
            counts["doubled_ts"] += 1
        elif DF:
            counts["doubled_frame"] += 1
        elif ts - prev_ts > 0.05:
            counts["skipped_ts"] += 1
            STS = True
        else:
            counts["correct"] += 1
        if DTS or DF or STS:
            k += 2
            if k >= len(stamps):
                break
        prev_ts, prev = stamps[k], frames[k]
    return counts


# ------------------------------------------------------------------------------------------------ cases
def boxes_case(n, seed=3):
    """fp32 [n,7] states with y below, at (from three rows on) and above 60, both directions, and zero, fast and slow speeds."""
    rs = np.random.RandomState(seed)
    st = np.stack((rs.uniform(100, 400, n), rs.uniform(5, 115, n), rs.uniform(12, 60, n), rs.uniform(5, 9, n), rs.uniform(4, 13, n),
                   rs.choice([-1.0, 1.0], n), rs.uniform(0, 130, n)), 1).astype(np.float32)
    for k, y in enumerate((np.nextafter(np.float32(60), np.float32(0)), np.nextafter(np.float32(60), np.float32(61)), 60.0)):
        if k < n:
            st[n - 1 - k, 1] = y                                   # the last rows: a caller's offset keeps them
    if n > 3:
        st[n - 4, 6] = 0.0
    return st


def integrity_case(H=104, W=108, seed=9):
    """(stamps, frames) with one doubled frame, one doubled stamp, one of both and one skip, two frames consumed after each."""
    rs = np.random.RandomState(seed)
    fresh = lambda: rs.randint(0, 256, (H, W, 3)).astype(np.uint8)                 # noqa: E731
    stamps, frames = [100.0], [fresh()]

    def add(dt, same=False):
        stamps.append(stamps[-1] + dt)
        frames.append(frames[-1].copy() if same else fresh())
    for _ in range(3):
        add(1 / 30.0)
    add(1 / 30.0, same=True)                      # doubled frame
    for _ in range(4):
        add(1 / 30.0)
    add(0.0)                                      # doubled stamp
    for _ in range(4):
        add(1 / 30.0)
    add(0.0, same=True)                           # both
    for _ in range(4):
        add(1 / 30.0)
    add(0.1)                                      # skip
    for _ in range(4):
        add(1 / 30.0)
    return stamps, frames

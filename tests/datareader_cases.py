"""Inputs and a plain restatement for Data_Reader (3d-playground_amd/datareader.py; reference datareader.py:91-251, 401-584).

  tracking_csv(...)      a seeded generator of input files in the template of write_results_csv: irregular timestamps,
                         births, deaths, gaps, objects on both sides of y = 60, a per-row camera, and on request the
                         parser's edges (junk header lines, an unparsable row, a repeated (ts, id), an empty camera cell)
  load / walk / reinterpolate / file_rows / csv_text
                         the reference's load, resampling and rewrite restated in plain Python and NumPy, the projection
                         through oracle/homography.py.  The oracle on the GPU box, where the reference does not exist; held to
                         the reference's own output by tests/test_datareader_host.py (tests/golden/datareader.npz)
  GOLDEN_CASES           what tools/make_golden_datareader.py runs the reference on
"""
import csv
import io
import re

import numpy as np

from oracle import homography as ohg
from retinanet_mi355x import synth

FIELDS = ("x", "y", "l", "w", "h", "v")
CLASSES = ("sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer")
HEADER = ["Frame #", "Timestamp", "Object ID", "Object class", "BBox xmin", "BBox ymin", "BBox xmax", "BBox ymax", "vel_x",
          "vel_y", "Generation method", "fbrx", "fbry", "fblx", "fbly", "bbrx", "bbry", "bblx", "bbly", "ftrx", "ftry", "ftlx",
          "ftly", "btrx", "btry", "btlx", "btly", "fbr_x", "fbr_y", "fbl_x", "fbl_y", "bbr_x", "bbr_y", "bbl_x", "bbl_y",
          "direction", "camera", "acceleration", "speed", "veh rear x", "veh center y", "theta", "width", "length", "height"]
NAMES = ["p%dc%d" % (p, c) for p in (1, 2, 3) for c in range(1, 7)]
MIN_DIVISOR = 0.1                      # every fixture keeps the projection's homogeneous divisor above this

# case -> (input key, Data_Reader kwargs, frequency or None (no resampling), wrapper)
GOLDEN_CASES = {
    "plain": ("irregular", {}, None, False),
    "hz30": ("irregular", {}, 30, False),
    "hz10": ("irregular", {}, 10, False),
    "hz120": ("irregular", {}, 120, False),
    "wrapper": ("irregular", {}, 30, True),
    "metric": ("metres", {"metric": True}, 30, False),
    "working": ("working", {}, 30, False),
}


def case_inputs(g, case):
    key, kw, freq, wrapper = GOLDEN_CASES[case]
    names = [str(n) for n in g["names"]]
    P = g["working_P"] if case == "working" else g["P"]
    return g["in_" + key].tobytes().decode(), names[:len(P)], P, (g["P2"] if wrapper else None), kw, freq


def cameras(n=18):
    """-> (names, P [n,3,4], P2 [n,3,4]): the fixture cameras of tests/golden_cases.py:homography_inputs."""
    P, _ = synth.camera_matrices(18, seed=5)
    P2, _ = synth.camera_matrices(18, seed=55)
    return NAMES[:n], P[:n], P2[:n]


# ------------------------------------------------------------------------------------------------ generator
def csv_text(rows, header_lines=()):
    """Rows of cells -> the text csv.writer makes of them (\\r\\n line ends)."""
    f = io.StringIO()
    out = csv.writer(f, delimiter=",")
    for r in list(header_lines) + list(rows):
        out.writerow(r)
    return f.getvalue()


def _r(v):
    return repr(float(v))                                       # the shortest text that reads back to the same double


def tracking_rows(seed, n_frames, n_objs, n_cams=6, rate=25.0, scale=1.0, frame_objs=None):
    """-> (header row, data rows) of a tracking file.  Timestamps step by 1 / rate with +-40 % jitter and six decimals (the
    loader rounds to four); object k lives over a seeded frame range with seeded gaps, drives at its own speed in its own lane,
    eastbound below y = 60 and westbound above; its camera is the one of the first n_cams fixture cameras whose homogeneous
    divisor over the box's corners is largest (the smaller of the two matrix sets').  scale divides every length (scale = 3.281: a file in
    metres).  frame_objs: {frame: [object, ...]} overrides who is present (in that order)."""
    u = synth.uniform((n_objs, 8), seed).astype(np.float64)
    jit = synth.uniform((n_frames,), seed + 1).astype(np.float64)
    gap = synth.uniform((n_frames, max(n_objs, 1)), seed + 2)
    t, rows = 1623877000.0 + 0.123456, []
    header = HEADER + ["ts_bias for cameras {}".format(NAMES[:n_cams])]
    bias = [round(0.01 * c, 3) for c in range(n_cams)]
    names, P, P2 = cameras(n_cams)
    for f in range(n_frames):
        t += (0.6 + 0.8 * jit[f]) / rate
        if frame_objs is not None:
            present = frame_objs.get(f, [])
        else:
            present = []
            for k in range(n_objs):
                birth, life = int(u[k, 0] * n_frames * 0.5), 3 + int(u[k, 1] * n_frames)
                if birth <= f < birth + life and gap[f, k] > 0.12:
                    present.append(k)
            if f % 2:
                present = present[::-1]                         # the id order differs from frame to frame
        for k in present:
            direction = 1 if u[k, 2] < 0.5 else -1
            speed = 60.0 + 60.0 * u[k, 3]
            x = (100.0 + 250.0 * u[k, 4]) + direction * speed * (t - 1623877000.0)
            y = (8.0 + 44.0 * u[k, 5]) if direction == 1 else (68.0 + 44.0 * u[k, 5])
            l, w, h = 14.0 + 40.0 * u[k, 6], 5.5 + 3.0 * u[k, 7], 4.0 + 8.0 * u[k, 1]
            st = np.array([[x, y, l, w, h, direction]] * n_cams, np.float32)
            cam = names[int(np.argmax(divisors(st, names, names, P, P2).reshape(2, n_cams, 8).min(axis=(0, 2))))]
            cells = [""] * 45
            cells[0], cells[1], cells[2], cells[3] = str(f), "%.6f" % t, str(100 + k), CLASSES[k % len(CLASSES)]
            cells[10] = "3D Detector"
            cells[35], cells[36], cells[37], cells[38] = str(float(direction)), cam, "0", _r(speed / scale)
            cells[39], cells[40], cells[41] = _r(x / scale), _r(y / scale), "0"
            cells[42], cells[43], cells[44] = _r(w / scale), _r(l / scale), _r(h / scale)
            rows.append(cells + [str(bias)])
    return header, rows


def tracking_csv(seed=1, n_frames=24, n_objs=7, edges=False, **kw):
    """The file as text.  edges: junk lines in front of the header, a row with a letter in a number cell, a repeated (ts, id)
    whose later row differs, a row with an empty camera cell, a short row."""
    header, rows = tracking_rows(seed, n_frames, n_objs, **kw)
    lines = []
    if edges:
        lines = [["Video sequence name", "whatever"], [], ["Frame #"[:-1], "not yet"]]
        bad = list(rows[2])
        bad[39] = "12.5ft"
        dup = list(rows[0])
        dup[39] = _r(float(dup[39]) + 1.0)
        nocam = list(rows[1])
        nocam[36] = ""
        nocam[2] = "999"
        rows = rows[:3] + [bad, ["7", "1.0"]] + rows[3:6] + [dup, nocam] + rows[6:]
    return csv_text([header] + rows, lines)


# ------------------------------------------------------------------------------------------------ restatement
def load(text, metric=False):
    """datareader.py:142-230 -> (cameras, data)."""
    cams, data, in_headers = None, {}, True
    for row in csv.reader(io.StringIO(text, newline="")):
        if in_headers:
            if len(row) > 0 and row[0] == "Frame #":
                in_headers = False
                cams = re.findall(r"(p\dc\d)", row[45])
            continue
        try:
            v = {"x": float(row[39]), "y": float(row[40]), "w": float(row[42]), "l": float(row[43]), "h": float(row[44])}
            direction = int(float(row[35]))
            v["v"] = float(row[38])
            oid = int(float(row[2]))
            ts = np.round(float(row[1]), 4)
            camera = row[36] if row[36] != "" else "p1c1"
            if metric:
                v = {k: x * 3.281 for k, x in v.items()}
            off = [float(c) for c in row[45].strip("[").strip("]").split(",")]
            off = dict([(cams[i], off[i]) for i in range(len(off))])
        except Exception:
            continue
        datum = dict(v, timestamp=ts, id=oid, direction=direction, ts_bias=off, camera=camera, frame=row[0])
        datum["class"] = row[3]
        data.setdefault(ts, {})[oid] = datum
    return cams, [data[k] for k in sorted(data)]


def _first_ts(frame):
    return frame[next(iter(frame))]["timestamp"]


def walk(data, frequency):
    """datareader.py:406-444 -> [(a, output_time), ...]."""
    out = []
    if len(data) == 0:
        return out
    a, ts = 0, _first_ts(data[0])
    next_ts = _first_ts(data[1]) if len(data) > 1 else None
    output_time = ts
    while next_ts is not None:
        out.append((a, output_time))
        output_time += 1.0 / frequency
        while output_time > next_ts:
            a += 1
            ts = _first_ts(data[a])
            next_ts = _first_ts(data[a + 1]) if a + 1 < len(data) else None
            if next_ts is None:
                break
        if output_time < ts:
            print("Time Error!")
    return out


def reinterpolate(data, frequency):
    """datareader.py:411-447 -> the new data."""
    new = []
    for a, t in walk(data, frequency):
        cur, nxt, frame = data[a], data[a + 1], {}
        ts, next_ts = _first_ts(cur), _first_ts(nxt)
        for oid in cur:
            if oid in nxt:
                obj = dict(cur[oid])
                r1 = (t - ts) / (next_ts - ts)
                r2 = 1 - r1
                for k in FIELDS:
                    obj[k] = obj[k] * r1 + nxt[oid][k] * r2
                obj["timestamp"] = t
                frame[oid] = obj
        new.append(frame)
    return new


def dump(data):
    """(instant index, id, timestamp, six fields) of every datum as fp64 [n,9]: what the golden records of the reference's
    ``data`` after reinterpolate."""
    return np.array([[i, oid, o["timestamp"]] + [o[k] for k in FIELDS] for i, frame in enumerate(data) for oid, o in frame.items()],
                    np.float64).reshape(-1, 9)


def states(data):
    """datareader.py:530-535 for every datum -> (items, state fp32 [n,7], keep bool [n])."""
    items = [o for frame in data for o in frame.values()]
    st = np.array([[o["x"], o["y"], o["l"], o["w"], o["h"], o["direction"], o["v"]] for o in items], np.float64).reshape(-1, 7)
    st = st.astype(np.float32)
    return items, st, st[:, 0] != 0


def project(st, cams, names, P, P2=None):
    """datareader.py:538-550 -> (space fp32 [n,4,2], im fp64 [n,8,2], box fp64 [n,4])."""
    idx = np.array([list(names).index(c) for c in cams], np.int64)
    space = ohg.state_to_space(st[:, :6])
    if len(st) == 0:
        return space[:, :4, :2], np.zeros((0, 8, 2)), np.zeros((0, 4))
    im = ohg.space_to_im(space, P[idx]) if P2 is None else ohg.wrapper_space_to_im(space, P[idx], P2[idx])
    box = np.stack((im[:, :, 0].min(1), im[:, :, 1].min(1), im[:, :, 0].max(1), im[:, :, 1].max(1)), 1)
    return space[:, :4, :2], im, box


def divisors(st, cams, names, P, P2=None):
    """The homogeneous divisor of every projected corner (through both matrix sets when there are two)."""
    idx = np.array([list(names).index(c) for c in cams], np.int64)
    hom = np.concatenate((ohg.state_to_space(st[:, :6]).astype(np.float64), np.ones((len(st), 8, 1))), 2)
    w = np.einsum("nj,nkj->nk", P[idx][:, 2], hom)
    return w if P2 is None else np.concatenate((w, np.einsum("nj,nkj->nk", P2[idx][:, 2], hom)))


def file_rows(data, names, P, P2=None):
    """datareader.py:516-584 -> the rows, cells as the objects csv.writer is handed."""
    items, st, keep = states(data)
    items, st = [o for o, k in zip(items, keep) if k], st[keep]
    space, im, box = project(st, [o["camera"] for o in items], names, P, P2)
    rows = []
    for i, o in enumerate(items):
        s = st[i]
        row = ["-", o["timestamp"], o["id"], o["class"], box[i, 0].item(), box[i, 1].item(), box[i, 2].item(), box[i, 3].item(), 0, 0,
               "3D Detector"] + list(im[i].reshape(-1)) + list(space[i].reshape(-1))
        row += [s[5], o["camera"], 0, s[6], s[0], s[1], np.pi / 2.0 if s[5] == -1 else 0, s[3], s[2], s[4],
                [o["ts_bias"][k] for k in o["ts_bias"].keys()]]
        rows.append(row)
    return rows


def file_text(data, cams, names, P, P2=None):
    return csv_text([HEADER + ["ts_bias for cameras {}".format(cams)]] + file_rows(data, names, P, P2))


def run(text, names, P, P2=None, metric=False, frequency=None):
    """Load, resample (frequency not None), write -> (data, file text)."""
    cams, data = load(text, metric=metric)
    if frequency is not None:
        data = reinterpolate(data, frequency)
    return data, file_text(data, cams, names, P, P2)


# ------------------------------------------------------------------------------------------------ comparison
STRING_COLS = tuple(range(0, 4)) + (8, 9, 10) + tuple(range(27, 46))
NUMERIC_COLS = tuple(range(4, 8)) + tuple(range(11, 27))


def parse(text):
    return list(csv.reader(io.StringIO(text, newline="")))


def compare_text(got, want, rtol, atol):
    """Header and the string cells equal, the BBox and image cells numerically close -> the largest numeric deviation."""
    g, w = parse(got), parse(want)
    assert len(g) == len(w), (len(g), len(w))
    assert g[0] == w[0]
    worst = 0.0
    for k, (a, b) in enumerate(zip(g[1:], w[1:])):
        assert len(a) == len(b) == 46, (k, len(a), len(b))
        for c in STRING_COLS:
            assert a[c] == b[c], (k, c, a[c], b[c])
        x, y = np.array([float(a[c]) for c in NUMERIC_COLS]), np.array([float(b[c]) for c in NUMERIC_COLS])
        assert np.allclose(x, y, rtol=rtol, atol=atol), (k, x, y)
        worst = max(worst, float(np.abs(x - y).max()))
    return worst

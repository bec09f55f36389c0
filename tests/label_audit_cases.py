"""Scripted multi-camera label sets and a plain Python restatement of the label audit (label_audit.py /
csrc/label_audit.hip): estimate_ts_bias, est_y_error, estimate_projection_error, remove_outliers, interpolate (every
object) and unbias_timestamps of the reference's annotator.  No GPU, no package import: tools/make_golden_labels.py runs the
reference's own methods on ``golden_scenes()`` (-> tests/golden/label_audit.npz), the tests rebuild the same scenes here, and
the restatement is the oracle of the fuzz scenes.  Python floats are fp64 with one rounding per operation, which is what the
kernels compute.

Restated, not copied: the tracklets are collected once per scene (the reference collects them again for every pair and
object), the samples of one (pair, object) come from ``samples`` for all three estimators, the outlier walk keeps a set of
deleted rows.  What the restatement does differently from the reference on purpose is what label_audit.py documents:
remove_outliers takes the id bound once and raises RuntimeError when an id goes extinct, est_y_error raises ValueError where
the reference has nothing to carry.

golden_scenes():
  "audit"    6 cameras, 200 frames, ids 0..11 and 14 (12 is the first unused id: 14 is ignored).  Pair (1, 0) holds the edges:
             tracklets of 130 / 65, 64 / 63, 2 / 2, 1 / 10 rows (and none at all in camera 2); id 4 a zig-zag x (several
             crossings, the last wins); id 5 sample points that hit rows exactly, with an interpolated time and x of exactly
             0.0; id 6 repeated x (the 1e-08 guard); id 7 ran == 0; id 8 a passed guard with hi < lo.  Camera 3 shares objects
             with camera 1 only (first partner at decrement 2), camera 5 holds one row of id 9 and the ignored id: no partner.
             Curvature polynomials are non-zero in both directions and missing for one camera ("Error 1458").
  "outliers" a jump in x, a one-sided jump in y (up is deleted from behind, down from ahead), a chain (deleting row f saves row
             f + 1), a box in frame 0 judged against the last frame, an empty frame past last_frame that ends the walk ahead of
             a later jump.
  "interp"   gaps of 1 and of 70 frames, uneven all_ts, two cameras for one object, a tracklet without a gap, a single row, an
             id above the gap (left alone by interpolate_all, filled by interpolate(4)).
  "few"      5 cameras, 2 ids: estimate_projection_error steps its partner by the number of ids (camera 4 pairs with 3 and
             with 1), which the other scenes, with more ids than cameras, never reach."""
import copy

import numpy as np

CLASSES = ("sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer")
POINTS = 5
GUARD, FOUND_CUR, FOUND_PREV = 1, 2, 4


class Cam():
    def __init__(self, name):
        self.name = name


class Labels():
    """A stand-in ``self`` with the attributes the annotator's batch passes read."""

    def __init__(self, scene):
        self.data = copy.deepcopy(scene["data"])
        self.cameras = [Cam(n) for n in scene["names"]]
        self.seq_keys = list(scene["names"])
        self.all_ts = copy.deepcopy(scene["all_ts"])
        self.ts_bias = np.array(scene["ts_bias"], np.float64)
        self.poly_params = copy.deepcopy(scene["poly_params"])
        self.last_frame = scene["last_frame"]
        self.hg = None


def camera_names(n):
    return ["p{}c{}".format(1 + i // 6, 1 + i % 6) for i in range(n)]


def empty_scene(n_cam, n_frames, seed, last_frame=None, jitter=0.004):
    rng = np.random.RandomState(seed)
    names = camera_names(n_cam)
    offset = np.concatenate(([0.0], rng.uniform(-0.05, 0.05, n_cam - 1))) if n_cam else np.zeros(0)
    all_ts = [{n: float(f / 30.0 + offset[c] + (rng.uniform(0, jitter) if f else 0.0)) for c, n in enumerate(names)}
              for f in range(n_frames)]
    poly = {}
    for c, n in enumerate(names):
        poly[n + "_EB"] = [1e-5 * (c + 1), -2e-3 * (c + 1), 0.25 + 0.1 * c]
        poly[n + "_WB"] = [-2e-5 * (c + 1), 1e-3 * (c + 1), -0.5 + 0.05 * c]
    return dict(names=names, data=[{} for _ in range(n_frames)], all_ts=all_ts, ts_bias=[0.1 * c for c in range(n_cam)],
                poly_params=poly, last_frame=n_frames if last_frame is None else last_frame)


def put(scene, f, c, oid, x, y, t=None, cls=0, gen=None):
    name = scene["names"][c]
    item = {"x": float(x), "y": float(y), "l": 15.0 + oid, "w": 6.0 + 0.1 * c, "h": 5.0 + 0.01 * f,
            "direction": 1 if y < 60 else -1, "id": oid, "class": CLASSES[cls % len(CLASSES)],
            "timestamp": scene["all_ts"][f][name] if t is None else float(t), "camera": name}
    if gen is not None:
        item["gen"] = gen
    scene["data"][f]["{}_{}".format(name, oid)] = item


def track(scene, c, oid, f0, n, x0, dx, y, zig=0.0, dy=0.01, step=1):
    for k in range(n):
        put(scene, f0 + k * step, c, oid, x0 + dx * k + zig * ((k * 7) % 5 - 2), y + dy * k, cls=oid)


def scene_audit():
    s = empty_scene(6, 200, seed=5)
    for c in (0, 1, 2):
        s["all_ts"][0][s["names"][c]] = 0.0                    # an interpolated time of exactly 0.0 (id 5)
    del s["poly_params"]["p1c5_EB"]                             # a failed curvature lookup
    track(s, 0, 0, 0, 130, 0.0, 1.0, 30.0)                      # 130 and 65 rows
    track(s, 1, 0, 100, 65, 100.5, 1.0, 31.0)
    track(s, 0, 1, 10, 64, 50.0, 1.0, 42.0)                     # 64 and 63 rows
    track(s, 1, 1, 55, 63, 95.25, 1.0, 41.5)
    for k, (a, b) in enumerate(((100.0, 101.0), (104.0, 103.0))):   # 2 and 2 rows
        put(s, 20 + k, 0, 2, a, 80.0)
        put(s, 20 + k, 1, 2, b, 81.0)
    put(s, 30, 0, 3, 100.0, 20.0)                               # 1 row against 10: the guard fails; camera 2 has none
    track(s, 1, 3, 30, 10, 95.0, 1.0, 20.5)
    track(s, 0, 4, 0, 81, 60.0, 1.0, 90.0)                      # id 4: zig-zag in camera 1
    track(s, 1, 4, 40, 40, 100.0, 1.0, 91.0, zig=3.0)
    for f in range(9):                                          # id 5: points that hit rows, zeros
        put(s, f, 0, 5, float(f), 25.0 + f)
        put(s, f, 2, 5, float(f), 26.0 + f)
        if f % 2 == 0:
            put(s, f, 1, 5, float(f), 25.5 + f)
    for k, x in enumerate((200.0, 201.0, 201.0, 202.0, 203.0, 204.0)):   # id 6: repeated x
        put(s, 50 + k, 0, 6, x, 33.0 + k)
    for k, x in enumerate((201.0, 201.0, 202.0, 203.0)):
        put(s, 51 + k, 1, 6, x, 33.5 + k)
    track(s, 0, 7, 60, 21, 140.0, 1.0, 70.0)                    # id 7: ran == 0
    put(s, 70, 1, 7, 150.0, 70.5)
    put(s, 71, 1, 7, 150.0, 71.5)
    track(s, 1, 8, 80, 5, 300.0, 1.0, 35.0)                     # id 8: hi < lo behind a passed guard
    track(s, 0, 8, 90, 11, 310.0, 1.0, 36.0)
    track(s, 1, 9, 100, 60, 150.0, 2.0, 45.0)                   # id 9: cameras 1, 2, one row in 5
    track(s, 2, 9, 120, 60, 190.5, 2.0, 45.5)
    put(s, 150, 5, 9, 250.0, 45.0)
    track(s, 1, 10, 20, 70, 260.0, -1.5, 95.0)                  # id 10 (WB): cameras 1 and 3 only
    track(s, 3, 10, 40, 65, 231.0, -1.5, 96.0, zig=0.5)
    track(s, 3, 11, 100, 80, 300.0, 1.0, 50.0)                  # id 11: cameras 3 and 4
    track(s, 4, 11, 130, 66, 330.5, 1.0, 51.0)
    track(s, 5, 14, 10, 12, 500.0, 1.0, 30.0)                   # above the first unused id (12): ignored
    track(s, 4, 14, 10, 12, 500.5, 1.0, 30.0)
    return s


def scene_outliers():
    s = empty_scene(3, 30, seed=6, last_frame=20)

    def run(c, oid, frames, x_of, y_of):
        for f in frames:
            if f != 24:                                         # frame 24 stays empty: the walk ends there
                put(s, f, c, oid, x_of(f), y_of(f), cls=oid)
    run(0, 0, range(0, 28), lambda f: 2.0 * f + (40.0 if f == 10 else 0.0), lambda f: 30.0)             # x jump, the chain
    run(0, 1, range(2, 29), lambda f: 100.0 + f, lambda f: 30.0 + (8.0 if 5 <= f < 15 else 0.0))          # y up, y down
    run(1, 2, [0, 1, 2, 3, 29], lambda f: 50.0 + f, lambda f: 80.0)                                     # frame 0 against frame 29
    run(1, 0, range(5, 12), lambda f: 2.0 * f, lambda f: 31.0 + (5.0 if f == 8 else 0.0))                 # exactly 5: kept
    run(2, 1, range(20, 30), lambda f: 100.0 + f + (50.0 if f == 26 else 0.0), lambda f: 30.0)            # past the break
    run(2, 2, [7, 9, 11], lambda f: 400.0 * f, lambda f: 10.0)                                          # no neighbouring frames
    run(2, 5, range(3, 8), lambda f: 10.0 + 30.0 * f, lambda f: 10.0)                                   # id 5 > first unused (3)
    return s


def scene_interp():
    s = empty_scene(3, 120, seed=7, jitter=0.02)
    for f in (0, 2, 3, 74, 75):
        put(s, f, 0, 0, 10.0 + 1.5 * f, 30.0 + 0.1 * f)
    for f in (5, 9):
        put(s, f, 1, 0, 12.0 + 1.5 * f, 31.0)
    track(s, 2, 1, 10, 11, 80.0, 1.0, 90.0)
    put(s, 50, 1, 2, 5.0, 5.0)
    for f in (100, 104, 119):
        put(s, f, 2, 4, 3.0 * f, 100.0 - 0.5 * f)
    return s


def scene_few():
    s = empty_scene(5, 40, seed=8)
    for c in range(5):                                          # two objects, five cameras that all see them
        track(s, c, 0, 2 * c, 30, 10.0 + 0.1 * c, 2.0, 30.0 + 0.3 * c, zig=0.2)
        track(s, c, 1, 5 + c, 25, 90.0 - 0.2 * c, -2.5, 85.0 - 0.2 * c)
    return s


def golden_scenes():
    return {"audit": scene_audit(), "outliers": scene_outliers(), "interp": scene_interp(), "few": scene_few()}


# ------------------------------------------------------------------------------------------------ fuzz
def fuzz_scene(seed):
    """A random scene: objects drive along x through cameras whose views overlap, every camera measures with its own noise and
    clock; some boxes are missing (gaps) and some jump (outliers)."""
    rng = np.random.RandomState(1000 + seed)
    n_cam, n_frames, n_obj = int(rng.randint(3, 6)), int(rng.randint(24, 60)), int(rng.randint(3, 9))
    s = empty_scene(n_cam, n_frames, seed=2000 + seed, last_frame=int(rng.randint(n_frames // 2, n_frames + 5)))
    ids = list(range(n_obj))
    if rng.rand() < 0.3:
        ids[-1] += 2                                            # an id above a gap
    for j, oid in enumerate(ids):
        eb = rng.rand() < 0.6
        v = rng.uniform(2.0, 5.0) * (1 if eb else -1)
        x_start = rng.uniform(-20.0, 40.0) if eb else rng.uniform(60.0 * n_cam - 40.0, 60.0 * n_cam + 20.0)
        y_lane = rng.uniform(10.0, 50.0) if eb else rng.uniform(70.0, 110.0)
        f_in = int(rng.randint(0, n_frames // 3))
        for c in range(n_cam):
            lo, hi = 60.0 * c - 15.0, 60.0 * c + 85.0           # 40 of overlap between neighbours
            for f in range(f_in, n_frames):
                x = x_start + v * (f - f_in)
                if not lo <= x <= hi or rng.rand() < 0.08:
                    continue
                jump_x = 30.0 if rng.rand() < 0.01 else 0.0
                jump_y = 9.0 if rng.rand() < 0.01 else 0.0
                put(s, f, c, oid, x + rng.normal(0, 0.3) + jump_x, y_lane + rng.normal(0, 0.2) + jump_y, cls=j)
    if rng.rand() < 0.2 and n_frames > 30:
        for f in range(n_frames - 4, n_frames):
            s["data"][f] = {}                                   # trailing empty frames: the last_frame break
    return s


# ------------------------------------------------------------------------------------------------ restatement
def unused_id(data):
    used = {item["id"] for fd in data for item in fd.values()}
    n = 0
    while n in used:
        n += 1
    return n


def tracklets(data, names, ids=None):
    """{(camera index, id): [(frame, x, y, timestamp, key), ...]} for the ids the reference visits (or ``ids``)."""
    ids = set(range(unused_id(data)) if ids is None else ids)
    at = {n: c for c, n in reversed(list(enumerate(names)))}
    out = {}
    for f, fd in enumerate(data):
        for key, item in fd.items():
            if item["id"] in ids:
                out.setdefault((at[item["camera"]], item["id"]), []).append(
                    (f, float(item["x"]), float(item["y"]), float(item["timestamp"]), key))
    return out


def _last_crossing(K, pt):
    hit = 0
    for i in range(1, len(K)):
        if (K[i] - pt) * (K[i - 1] - pt) <= 0:
            hit = i
    return hit


def _at(K, V, i, pt):
    ratio = (pt - K[i - 1]) / (K[i] - K[i - 1] + 1e-08)
    return V[i - 1] + (V[i] - V[i - 1]) * ratio


def samples(cur, prev, kc, vcs):
    """The five samples of one (pair, object): tracklets as lists of (frame, x, y, t, key); kc / vcs pick the key and value
    columns (0 x, 1 y, 2 t).  -> None when the guard fails, else per point (found cur, found prev, cur values, prev values)."""
    if len(cur) <= 1 or len(prev) <= 1:
        return None
    K1, K0 = [r[1 + kc] for r in cur], [r[1 + kc] for r in prev]
    if not max(K0) > min(K1):
        return None
    lo, hi = max(min(K1), min(K0)), min(max(K1), max(K0))
    ran = hi - lo
    out = []
    for q in range(POINTS):
        pt = lo + ran / (POINTS - 1) * q
        i1, i0 = _last_crossing(K1, pt), _last_crossing(K0, pt)
        out.append((i1 > 0, i0 > 0,
                    [_at(K1, [r[1 + v] for r in cur], i1, pt) if i1 else None for v in vcs],
                    [_at(K0, [r[1 + v] for r in prev], i0, pt) if i0 else None for v in vcs]))
    return out


def sample_block(scene_or_labels, kc, v0, v1=-1):
    """What ops.label_pair_samples returns for the scene: (flags uint8 [P, n, 5], values fp64 [P, n, 5, 4])."""
    data, names = _data_names(scene_or_labels)
    n, C = unused_id(data), len(names)
    tr = tracklets(data, names)
    flags = np.zeros((C * (C - 1) // 2, n, POINTS), np.uint8)
    values = np.zeros((C * (C - 1) // 2, n, POINTS, 4), np.float64)
    vcs = [v0] + ([v1] if v1 >= 0 else [])
    for cam in range(1, C):
        for prev in range(cam):
            for obj in range(n):
                got = samples(tr.get((cam, obj), []), tr.get((prev, obj), []), kc, vcs)
                for q, (f1, f0, a, b) in enumerate(got or []):
                    p = cam * (cam - 1) // 2 + prev
                    flags[p, obj, q] = GUARD | (FOUND_CUR if f1 else 0) | (FOUND_PREV if f0 else 0)
                    for k in range(len(vcs)):
                        values[p, obj, q, 2 * k] = a[k] if f1 else 0.0
                        values[p, obj, q, 2 * k + 1] = b[k] if f0 else 0.0
    return flags, values


def _data_names(x):
    if isinstance(x, dict):
        return x["data"], x["names"]
    return x.data, [c.name for c in x.cameras]


def ref_ts_bias(me):
    """-> (pairs [(cam, prev)], diffs per pair, used per camera); sets me.ts_bias."""
    data, names = _data_names(me)
    tr, n = tracklets(data, names), unused_id(data)
    me.ts_bias[0] = 0
    pairs, lists, used = [], [], [None] * len(names)
    for cam in range(1, len(names)):
        for prev in range(cam - 1, -1, -1):
            diffs = []
            for obj in range(n):
                for f1, f0, a, b in samples(tr.get((cam, obj), []), tr.get((prev, obj), []), 0, [2]) or []:
                    if f1 and f0 and a[0] and b[0]:
                        diffs.append(a[0] - b[0])
            if diffs:
                arr = np.array(diffs)
                mean, std = np.mean(arr), np.std(arr)
                me.ts_bias[cam] = me.ts_bias[prev] - mean
                pairs.append((cam, prev))
                lists.append(arr)
                used[cam] = (prev, mean, std, len(arr))
                break
    return pairs, lists, used


def ref_y_error(me):
    """-> (pairs, |y2 - y1| per pair with samples, all_diffs, stats per pair (cam, cam - 1))."""
    data, names = _data_names(me)
    tr, n = tracklets(data, names), unused_id(data)
    pairs, lists, all_diffs, stats = [], [], [], []
    y1 = y2 = None
    for cam in range(1, len(names)):
        diffs = []
        for obj in range(n):
            for f1, f0, a, b in samples(tr.get((cam, obj), []), tr.get((cam - 1, obj), []), 0, [1]) or []:
                y1 = a[0] if f1 else y1
                y2 = b[0] if f0 else y2
                if y1 is None or y2 is None:
                    raise ValueError("nothing to carry for cameras {} and {}, object {}".format(cam, cam - 1, obj))
                diffs.append(np.abs(y2 - y1))
        if diffs:
            arr = np.array(diffs)
            pairs.append((cam, cam - 1))
            lists.append(arr)
            all_diffs.append(np.mean(arr))
            stats.append((np.mean(arr), np.std(arr)))
        else:
            stats.append(None)
    return pairs, lists, all_diffs, stats


def projection_partners(cam, n_ids):
    """The partners estimate_projection_error gives camera ``cam``: the reference steps its ``decrement`` once per object, so
    from the neighbour it moves on by the number of ids, and it stops above camera 0.  Without ids: none."""
    return [cam - d for d in range(1, cam, n_ids)] if n_ids else []


def ref_projection_error(me, reverse_curve_offset=False):
    data, names = _data_names(me)
    tr, n = tracklets(data, names), unused_id(data)
    xe, ye = [], []
    for cam in range(1, len(names)):
        for prev in projection_partners(cam, n):
            for obj in range(n):
                for f1, f0, a, b in samples(tr.get((cam, obj), []), tr.get((prev, obj), []), 2, [0, 1]) or []:
                    if not (f1 and f0 and a[0] and b[0]):
                        continue
                    cx, cy, px, py = a[0], a[1], b[0], b[1]
                    if reverse_curve_offset:
                        d = "EB" if cy < 60 else "WB"
                        k = me.poly_params.get("{}_{}".format(names[cam], d))
                        if k is not None:
                            cy -= k[2] + k[1] * cx + k[0] * cx ** 2
                        k = me.poly_params.get("{}_{}".format(names[prev], d))
                        if k is not None:
                            py -= k[2] + k[1] * px + k[0] * px ** 2
                    xe.append(np.abs(cx - px))
                    ye.append(np.abs(cy - py))
    return xe, ye


def visited(data, last_frame):
    for f in range(len(data)):
        if f > last_frame and len(data[f]) == 0:
            return f
    return len(data)


def ref_outliers(me):
    """-> the deleted (frame, key) in tracklet order; deletes them from me.data.  RuntimeError (data untouched) when every box
    of an id below the bound would go."""
    data, names = _data_names(me)
    tr, F, stop = tracklets(data, names), len(data), visited(data, me.last_frame)
    gone = []
    for (cam, obj), rows in sorted(tr.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        by_frame = {r[0]: r for r in rows}
        dead = set()
        for r in rows:
            f = r[0]
            if f >= stop:
                break
            before = by_frame.get(F - 1) if f == 0 else (by_frame.get(f - 1) if f - 1 not in dead else None)
            after = by_frame.get(f + 1) if f + 1 < F else None
            for other in (before, after):
                if other is not None and (abs(r[1] - other[1]) > 15 or r[2] - other[2] > 5):
                    dead.add(f)
                    gone.append((f, r[4], obj))
                    break
    total, lost = {}, {}
    for (cam, obj), rows in tr.items():
        total[obj] = total.get(obj, 0) + len(rows)
    for f, key, obj in gone:
        lost[obj] = lost.get(obj, 0) + 1
    if any(lost.get(obj, 0) == cnt for obj, cnt in total.items()):
        raise RuntimeError("an id would lose every box")
    for f, key, obj in gone:
        del data[f][key]
    return [(f, key) for f, key, obj in gone]


def ref_interpolate(me, ids=None):
    """Fills every gap of the objects ``ids`` (default: all below the first unused id), object outer, camera inner."""
    data, names = _data_names(me)
    ids = list(range(unused_id(data)) if ids is None else ids)
    tr = tracklets(data, names, ids)
    added = 0
    for obj in ids:
        for cam, name in enumerate(names):
            rows = tr.get((cam, obj), [])
            for a, b in zip(rows[:-1], rows[1:]):
                box = data[a[0]][a[4]]
                for f in range(a[0] + 1, b[0]):
                    t1, t2, ti = me.all_ts[a[0]][name], me.all_ts[b[0]][name], me.all_ts[f][name]
                    p1 = float(t2 - ti) / float(t2 - t1)
                    p2 = 1.0 - p1
                    data[f]["{}_{}".format(name, obj)] = {
                        "x": p1 * a[1] + p2 * b[1], "y": p1 * a[2] + p2 * b[2], "l": box["l"], "w": box["w"], "h": box["h"],
                        "direction": box["direction"], "id": obj, "class": box["class"], "timestamp": ti, "camera": name,
                        "gen": "Interpolation"}
                    added += 1
    return added


def ref_unbias(me):
    ref_ts_bias(me)
    bias = {k: me.ts_bias[i] for i, k in enumerate(me.seq_keys)}
    for fd in me.data:
        for item in fd.values():
            if item["camera"] in bias:
                item["timestamp"] += bias[item["camera"]]
    for row in me.all_ts:
        for i, k in enumerate(me.seq_keys):
            if k in row:
                row[k] += me.ts_bias[i]


# ------------------------------------------------------------------------------------------------ dumps (arrays only)
KEYS = ("x", "y", "l", "w", "h", "direction", "id", "class", "timestamp", "camera", "gen")


def dump(data, names):
    """``data`` in dict order -> (index int64 [n,5] = (frame, camera, id, class, gen: 0 none / 1 Interpolation / 2 other),
    values fp64 [n,7] = (x, y, l, w, h, direction, timestamp))."""
    idx, val = [], []
    for f, fd in enumerate(data):
        for key, item in fd.items():
            assert key == "{}_{}".format(item["camera"], item["id"])
            gen = 0 if "gen" not in item else (1 if item["gen"] == "Interpolation" else 2)
            idx.append((f, names.index(item["camera"]), item["id"], CLASSES.index(item["class"]), gen))
            val.append([float(item[k]) for k in ("x", "y", "l", "w", "h", "direction", "timestamp")])
    return np.array(idx, np.int64).reshape(-1, 5), np.array(val, np.float64).reshape(-1, 7)


def ts_table(all_ts, names):
    return np.array([[row[n] for n in names] for row in all_ts], np.float64).reshape(len(all_ts), len(names))


def ragged(pairs, lists):
    """[(cam, prev)], [array] -> (pairs int64 [k,2], offsets int64 [k+1], flat fp64)."""
    off = np.cumsum([0] + [len(a) for a in lists]).astype(np.int64)
    flat = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in lists]) if lists else np.zeros(0)
    return np.array(pairs, np.int64).reshape(-1, 2), off, flat


def restated(name, scene):
    """Every array tools/make_golden_labels.py writes for one scene, from the restatement: {key: array}."""
    out = {}
    names = scene["names"]
    me = Labels(scene)
    pairs, lists, _ = ref_ts_bias(me)
    out["ts_pairs"], out["ts_off"], out["ts_diffs"] = ragged(pairs, lists)
    out["ts_bias"] = np.array(me.ts_bias, np.float64)
    pairs, lists, all_diffs, _ = ref_y_error(Labels(scene))
    out["y_pairs"], out["y_off"], out["y_diffs"] = ragged(pairs, lists)
    out["y_means"] = np.array(all_diffs, np.float64).reshape(-1)
    for tag, flag in (("proj", False), ("curve", True)):
        xe, ye = ref_projection_error(Labels(scene), flag)
        out[tag + "_x"], out[tag + "_y"] = np.array(xe, np.float64).reshape(-1), np.array(ye, np.float64).reshape(-1)
    me = Labels(scene)
    ref_outliers(me)
    out["outliers_idx"], out["outliers_val"] = dump(me.data, names)
    me = Labels(scene)
    ref_interpolate(me)
    ref_interpolate(me, [4])
    out["interp_idx"], out["interp_val"] = dump(me.data, names)
    me = Labels(scene)
    ref_unbias(me)
    out["unbias_idx"], out["unbias_val"] = dump(me.data, names)
    out["unbias_ts"], out["unbias_bias"] = ts_table(me.all_ts, names), np.array(me.ts_bias, np.float64)
    return {name + "_" + k: v for k, v in out.items()}

"""Scripted multi-camera label sets and a plain fp64 restatement of the label scores (label_quality.py /
csrc/label_quality.hip): calculate_total_variation, calculate_feasibility, the data half of plot_trajectories_unified and
annotator_rmse of the reference's later annotator (manual_annotator_state_v3.py).  No GPU, no package import:
tools/make_golden_label_quality.py runs the reference's own functions on ``golden_scenes()`` (-> tests/golden/
label_quality.npz), the tests rebuild the same scenes here, and the restatement is the oracle of the edge and fuzz scenes.
Python floats are fp64 with one rounding per operation, ``math.atan2`` is the C library's, every sum runs in ascending order.

Restated, not copied: the boxes are packed once into the audit's table (tracklet = object * cameras + camera, rows in
ascending frame), one ``series`` of an object's rows serves all three functions, the sort is Python's ``sorted`` on (timestamp,
position) -- the stable sort by time, which the reference's ``np.argsort`` equals wherever no two timestamps tie.

golden_scenes():
  "score"  3 cameras, 70 frames, ids 0..14 and 17 (15 is the first unused id: 17 is ignored).  Camera 1's clock runs 0.004 s
           ahead of camera 0's (its boxes of a shared frame are dropped by the 0.01 s rule), camera 2's 0.02 s (kept); camera
           2's time stamps run BACKWARDS over frames 30..36.  Ids 0..4 drive east (y < 60), 5..9 west (y > 60: the wrapper's
           second side), 10..14 west at other speeds, one of them too fast (v > 140), one with a zig-zag in y (theta outside
           +-25 degrees); id 12 is seen by one camera and stands still for two frames (v = -0.0: infeasible by the strict
           > 0); id 14 has a single box.  The ids are annotator_rmse's groups 0..4, 5..9, 10..14."""
import math

import numpy as np

import label_audit_cases as lc
import label_rewrite_cases as rc

F32, F64 = np.float32, np.float64
MIN_DT = 0.01                                                  # :3877
V_RANGE, THETA_RANGE = (0, 140), (-25, 25)                     # :3892-3894; the acceleration range never enters (:3975)
GROUP = 5                                                      # :3993


# ------------------------------------------------------------------------------------------------ tolerances
def theta_bound(theta):
    """|theta - reference| allowed: 6 ulp for an fp64 atan2 on the device (OpenCL's bound), 1 ulp for the host library, two
    roundings of the scaling by 180 / pi, all doubled: 16 ulp of max(|theta|, 1)."""
    return 16.0 * 2.0 ** -52 * max(abs(theta), 1.0)


def rmse_bound(n, largest):
    """|rmse - reference| allowed for a group of n boxes whose image coordinates are at most ``largest`` in magnitude: the
    reference's torch.mean does not sum in row order, and a sum of n terms moves by at most n ulp of its largest partial sum
    when reordered; 8 covers the mean, the differences, the squares and the root."""
    return 8.0 * n * 2.0 ** -53 * largest


# ------------------------------------------------------------------------------------------------ scenes
BIAS = (0.0, 0.004, 0.02)


def empty_scene(n_frames, seed):
    s = lc.empty_scene(3, n_frames, seed=seed)
    for f in range(n_frames):
        for c, n in enumerate(s["names"]):
            s["all_ts"][f][n] = f / 30.0 + BIAS[c] + 1e-4 * ((f * 7 + c * 3) % 11)
    for k, f in enumerate(range(30, 37)):                       # camera 2 runs backwards
        s["all_ts"][f][s["names"][2]] = 36 / 30.0 + BIAS[2] - 0.031 * k + 1e-4 * (k % 3)
    s["hg_old"] = rc.hg_spec(s["names"])
    return s


def drive(s, oid, f0, n, x0, dx, y, cams=None, zy=0.0, hold=()):
    """An object along x through the cameras that see it; frames in ``hold`` repeat the x of the frame before."""
    x, k = x0, 0
    for f in range(f0, min(f0 + n, len(s["data"]))):
        if f not in hold and f > f0:
            x += dx
            k += 1
        for c in range(len(s["names"])) if cams is None else cams:
            if 60.0 * c - 15.0 <= x <= 60.0 * c + 85.0:
                z = zy * (1.0 if (f + c) % 2 else -1.0)
                lc.put(s, f, c, oid, x + 0.03 * c + 0.011 * ((k * 5 + oid) % 7), y + 0.02 * k + 0.05 * c + z, cls=oid)


def scene_score():
    s = empty_scene(70, seed=51)
    for k in range(5):                                          # group 0: east
        drive(s, k, 2 * k, 50, -10.0 + 3.0 * k, 3.1 + 0.2 * k, 20.0 + 6.0 * k)
    for k in range(5):                                          # group 1: west, y > 60
        drive(s, 5 + k, k, 60, 200.0 - 4.0 * k, -(2.6 + 0.3 * k), 70.0 + 5.0 * k)
    drive(s, 10, 0, 40, 190.0, -5.2, 85.0)                      # 156 ft/s: too fast
    drive(s, 11, 5, 60, 170.0, -2.9, 90.0, zy=1.2)              # a zig-zag in y
    drive(s, 12, 10, 30, 100.0, -3.0, 95.0, cams=[1], hold=(20, 21))
    drive(s, 13, 25, 20, 150.0, -1.5, 100.0, cams=[2])          # inside the stretch that runs backwards
    lc.put(s, 40, 0, 14, 30.0, 75.0, cls=3)                     # a single box
    drive(s, 17, 3, 10, 10.0, 5.0, 40.0)                        # above the first unused id (15)
    return s


def golden_scenes():
    return {"score": scene_score()}


def fuzz_scene(seed):
    """lc.fuzz_scene's traffic (3 to 5 cameras, at most 60 frames and 8 ids) with camera clocks that are apart by less and by
    more than 0.01 s, and a homography."""
    rng = np.random.RandomState(4000 + seed)
    s = lc.fuzz_scene(seed)
    bias = rng.choice([0.0, 0.003, 0.008, 0.012, 0.02, -0.006], len(s["names"]))
    for f, fd in enumerate(s["data"]):
        for item in fd.values():
            c = s["names"].index(item["camera"])
            item["timestamp"] = f / 30.0 + float(bias[c]) + 1e-5 * ((f * 13 + c * 5 + item["id"]) % 17)
    s["hg_old"] = rc.hg_spec(s["names"], seed=4100 + seed, scale=0.002)
    return s


# ------------------------------------------------------------------------------------------------ the table
def table(data, names, ids=None):
    """The audit's table of the scene: (offsets int64 [n_ids * C + 1], cols fp64 [R,3] = (x, y, timestamp), lengths: ``l`` of
    every row)."""
    n = lc.unused_id(data) if ids is None else len(ids)
    tr = lc.tracklets(data, names, ids)
    offsets, rows, lengths = [0], [], []
    for obj in (range(n) if ids is None else ids):
        for cam in range(len(names)):
            for f, x, y, t, key in tr.get((cam, obj), []):
                rows.append((x, y, t))
                lengths.append(data[f][key]["l"])
            offsets.append(len(rows))
    return np.array(offsets, np.int64), np.array(rows, F64).reshape(-1, 3), lengths


def join_tables(tables):
    """[(offsets of one object per table, or of several, cols, n_cam)] with equal n_cam -> one table."""
    offsets, cols = [np.zeros(1, np.int64)], []
    for off, c in tables:
        offsets.append(np.asarray(off[1:], np.int64) + offsets[-1][-1])
        cols.append(np.asarray(c, F64).reshape(-1, 3))
    return np.concatenate(offsets), np.concatenate(cols) if cols else np.zeros((0, 3))


# ------------------------------------------------------------------------------------------------ restatement: the series
def series(rows, lane=None):
    """rows: [(x, y, t)] of one object, camera outer, frame inner -> dict: order (positions, sorted), keep, and on the m kept rows
    t, x, y, v, vy, a, theta; n, m, range, variation, feasible (segments)."""
    pos = [i for i, r in enumerate(rows) if lane is None or lane[0] < r[1] < lane[1]]
    order = sorted(pos, key=lambda i: (rows[i][2], i))
    ts = [rows[i][2] for i in order]
    keep = [1 if i == 0 or ts[i] >= ts[i - 1] + MIN_DT else 0 for i in range(len(order))]
    kept = [order[i] for i in range(len(order)) if keep[i]]
    x, y, t = ([rows[i][k] for i in kept] for k in range(3))
    m = len(kept)
    out = dict(order=order, keep=keep, t=t, x=x, y=y, n=len(order), m=m)
    if m > 1:
        dt = [t[i + 1] - t[i] + 1e-08 for i in range(m - 1)]
        v = [-((x[i + 1] - x[i]) / dt[i]) for i in range(m - 1)]
        v.append(v[-1])
        vy = [(y[i + 1] - y[i]) / dt[i] for i in range(m - 1)]
        vy.append(vy[-1])
        a = [(v[i + 1] - v[i]) / dt[i] for i in range(m - 1)]
        a.append(a[-1])
    else:
        v, vy, a = [0.0] * m, [0.0] * m, [0.0] * m
    theta = [math.atan2(vy[i], v[i]) * 180 / math.pi for i in range(m)]
    feasible = 0
    for i in range(m - 1):
        ok_v = max(v[i], v[i + 1]) < V_RANGE[1] and min(v[i], v[i + 1]) > V_RANGE[0]
        ok_t = max(theta[i], theta[i + 1]) < THETA_RANGE[1] and min(theta[i], theta[i + 1]) > THETA_RANGE[0]
        feasible += 1 if ok_v and ok_t else 0
    var = 0.0
    for i in range(1, m):
        var = var + abs(x[i] - x[i - 1])
    out.update(v=v, vy=vy, a=a, theta=theta, feasible=feasible, range=(max(x) - min(x)) if m else 0.0, variation=var)
    return out


def object_rows(offsets, cols, n_cam, obj):
    return [tuple(r) for r in cols[offsets[obj * n_cam]:offsets[(obj + 1) * n_cam]].tolist()]


def series_table(offsets, cols, n_cam, lane=None):
    """What ops.label_series returns for the table: (order int32 [R], keep uint8 [R], series fp64 [7,R], counts int32 [n,3],
    figs fp64 [n,2]), and the per-object dicts."""
    R, n = len(cols), (len(offsets) - 1) // n_cam
    order, keep = np.full(R, -1, np.int32), np.zeros(R, np.uint8)
    ser, counts, figs, per = np.zeros((7, R), F64), np.zeros((n, 3), np.int32), np.zeros((n, 2), F64), []
    for obj in range(n):
        s0 = int(offsets[obj * n_cam])
        s = series(object_rows(offsets, cols, n_cam, obj), lane)
        per.append(s)
        order[s0:s0 + s["n"]] = s0 + np.array(s["order"], np.int64)
        keep[s0:s0 + s["n"]] = s["keep"]
        for p, k in enumerate(("t", "x", "y", "v", "vy", "a", "theta")):
            ser[p, s0:s0 + s["m"]] = s[k]
        counts[obj] = (s["n"], s["m"], s["feasible"])
        figs[obj] = (s["range"], s["variation"])
    return order, keep, ser, counts, figs, per


def _per_object(me, lane=None):
    data, names = lc._data_names(me)
    offsets, cols, lengths = table(data, names)
    per = series_table(offsets, cols, len(names), lane)[5]
    return offsets, cols, lengths, per, len(names)


def ref_total_variation(me):
    """:3843-3889 -> (x_var, x_range)."""
    per = _per_object(me)[3]
    return [F64(s["variation"]) for s in per if s["n"]], [F64(s["range"]) for s in per if s["n"]]


def ref_feasibility(me):
    """:3891-3979 -> the feasible fraction of every object with more than one kept row."""
    return [F64(s["feasible"] / (s["m"] - 1)) for s in _per_object(me)[3] if s["m"] > 1]


def ref_kinematics(me, lane=None):
    """:3634-3711 with smooth = 1 -> per object with more than one kept row (id, time, x, y, v, a, theta, length of the last
    box that passed the lane filter, in camera-outer order)."""
    offsets, cols, lengths, per, C = _per_object(me, lane)
    out = []
    for obj, s in enumerate(per):
        if s["m"] > 1:
            last = int(offsets[obj * C]) + max(s["order"])
            out.append((obj, s["t"], s["x"], s["y"], s["v"], s["a"], s["theta"], lengths[last]))
    return out


# ------------------------------------------------------------------------------------------------ restatement: annotator_rmse
def rmse_boxes(me):
    """:3987-3994 -> per full group (state fp64 [n,6], camera index of the group's LAST box); ValueError for fewer than five
    ids or an empty group."""
    data, names = lc._data_names(me)
    n_ids = lc.unused_id(data)
    by_id = {}
    for fd in data:
        for obj in fd.values():
            by_id.setdefault(obj["id"], []).append(obj)
    if n_ids < GROUP:
        raise ValueError("fewer than five ids")
    groups = []
    for g in range(n_ids // GROUP):
        objs = [o for i in range(g * GROUP, (g + 1) * GROUP) for o in by_id.get(i, [])]
        if not objs:
            raise ValueError("an empty group")
        groups.append((np.array([[float(o[k]) for k in rc.STATE_KEYS] for o in objs], F64), names.index(objs[-1]["camera"])))
    return groups


def image_pos(state6, P1, P2):
    """The image of the rear bottom corners (2 and 3) of every box through one camera -> [(u2, v2, u3, v3)]: the state rounded
    to fp32, fp32 corners (homography.py:305-320), fp64 projection, the wrapper's switch on the corner-0 y."""
    out = []
    for st in state6:
        x, y, l, w, h, d = (F32(v) for v in st)
        half = d * w / F32(2.0)
        ylo, yhi = y - half, y + half
        P = P2 if P2 is not None and ylo > F32(60.0) else P1
        (u2, v2), (u3, v3) = (rc.project(P, F64(x), F64(cy), F64(0.0)) for cy in (ylo, yhi))
        out.append((float(u2), float(v2), float(u3), float(v3)))
    return out


def group_rmse(corners):
    """[(u2, v2, u3, v3)] -> (rmse, (mean u, mean v)), sums in ascending order (:3997-4000)."""
    n = len(corners)
    px = [(c[0] + c[2]) / 2.0 for c in corners]
    py = [(c[1] + c[3]) / 2.0 for c in corners]
    sx = sy = 0.0
    for i in range(n):
        sx, sy = sx + px[i], sy + py[i]
    mx, my = sx / n, sy / n
    ss = 0.0
    for i in range(n):
        dx, dy = px[i] - mx, py[i] - my
        ss = ss + (dx * dx + dy * dy)
    return math.sqrt(ss / n), (mx, my)


def ref_annotator_rmse(me):
    """:3981-4007 -> (rmse, per-group rmse, boxes per group, the largest |image coordinate| per group)."""
    names = [c.name for c in me.cameras]
    P1, P2 = rc.tables(me.hg, names)
    per, counts, largest = [], [], []
    for state6, cam in rmse_boxes(me):
        corners = image_pos(state6, P1[cam], P2[cam])
        per.append(group_rmse(corners)[0])
        counts.append(len(corners))
        largest.append(max(abs(v) for c in corners for v in c))
    total = 0.0
    for r in per:
        total = total + r
    return math.sqrt(total / len(per)), per, counts, largest


# ------------------------------------------------------------------------------------------------ dumps (arrays only)
def ragged(lists):
    off = np.cumsum([0] + [len(a) for a in lists]).astype(np.int64)
    return off, np.concatenate([np.asarray(a, F64).reshape(-1) for a in lists]) if lists else np.zeros(0)


def restated(name, scene):
    """Every array tools/make_golden_label_quality.py writes for one scene, from the restatement: {key: array}."""
    out = {}
    me = rc.Labels(scene)
    x_var, x_range = ref_total_variation(me)
    out["x_var"], out["x_range"] = np.array(x_var, F64), np.array(x_range, F64)
    out["feasible"] = np.array(ref_feasibility(me), F64)
    kin = ref_kinematics(me)
    out["ids"] = np.array([k[0] for k in kin], np.int64)
    for col, key in ((1, "time"), (4, "v"), (5, "a"), (6, "theta")):
        out["off"], out[key] = ragged([k[col] for k in kin])
    rmse, per, counts, largest = ref_annotator_rmse(me)
    out["rmse"], out["rmse_groups"] = np.array([rmse], F64), np.array(per, F64)
    out["rmse_counts"], out["rmse_largest"] = np.array(counts, np.int64), np.array(largest, F64)
    return {name + "_" + k: v for k, v in out.items()}

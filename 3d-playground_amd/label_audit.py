"""The batch passes of the reference's annotator (``seems_to_be_working.py``, class ``Annotator``) over a whole multi-camera label
set, on the GPU: ``estimate_ts_bias`` (:1845-1947), ``est_y_error`` (:1950-2036), ``estimate_projection_error`` (:2249-2357),
``remove_outliers`` (:2192-2233), ``interpolate`` (:780-836), ``unbias_timestamps`` (:1591-1627), plus ``get_unused_id``
(:894-907), ``count_classes`` (:2235-2247) and ``interpolate_all``, the loop ``for i in range(self.get_unused_id()):
self.interpolate(i, verbose=False)`` of :1584-1585 in one launch.

The functions take ``self`` exactly like the methods they replace and read the same attributes -- ``data`` (a list of
``{"<camera>_<id>": datum}`` dicts, one per frame), ``cameras`` (objects with ``.name``), ``seq_keys``, ``all_ts`` (a list of
``{camera: time stamp}`` dicts), ``ts_bias``, ``poly_params``, ``last_frame`` -- so a maintainer binds them into the reference
class unchanged::

    import label_audit
    for name in label_audit.METHODS:
        setattr(Annotator, name, getattr(label_audit, name))

or inherits ``LabelAudit``.  The reference runs each pass as a Python loop over camera pairs x objects x ALL frames with one
string-formatted dict lookup per step.  Here one pass over ``data`` packs a CSR table of tracklets (``pack_tracklets``: key
(object, camera), rows in ascending frame, fp64 x, y, timestamp and the int32 frame), one copy sends it to the device, and
csrc/label_audit.hip does the rest: ``ops.label_pair_samples`` (every camera pair x object in one launch: the overlap guard,
the five sample points, the last bracketing segment, the interpolated values), ``ops.label_outliers`` (the deletion
recurrence along every tracklet) and ``ops.label_interpolate`` (every missing frame of every tracklet).  The kernels' fp64
arithmetic rounds once per operation in the reference's order; the host assembles the lists from the sample block with numpy,
so ``np.mean`` / ``np.std`` run on identical lists and every returned number equals the reference's bit for bit
(``tests/golden/label_audit.npz``).  There is no CPU path: without a device every function raises.

Reference behaviour kept on purpose: only ids below ``get_unused_id()`` -- the FIRST id not in use -- are visited, so ids above
a gap are ignored; ``estimate_ts_bias`` drops a sample whose interpolated time is exactly 0.0 (``if time and prev_time``) and
tries partners at ``decrement = 1, 2, ...`` until one has samples; ``est_y_error`` reuses the y of the previous sample where a
crossing is not found (the reference's stale locals, carried across points, objects and camera pairs of one call);
``estimate_projection_error`` never pairs a camera with camera 0 (``decrement < cam_idx``) and advances ``decrement`` once per
OBJECT (its ``decrement += 1`` sits inside the loop over objects, :2355), so with n ids the partners of camera c are c - 1,
c - 1 - n, c - 1 - 2n, ...: with more ids than cameras, the usual case, the neighbour alone; it tests ``if cur_x and prev_x``, and
with ``reverse_curve_offset`` looks both polynomials up under the direction of the CURRENT camera's uncorrected y (``"EB"`` below
60) and leaves a y uncorrected when its lookup fails (the "Error 1458" print); ``remove_outliers`` tests y one-sided
(``np.abs(dy > 5)`` is the abs of a boolean), judges frame 0 against the LAST frame (``data[-1]``) and stops at the first empty
frame past ``last_frame``.

Differences a caller can see: ``est_y_error`` returns ``(all_diffs, per-pair (mean, std))`` and
``estimate_ts_bias`` the per-camera ``(prev_cam index, mean, std, n)`` it used (the reference returns None from both);
``est_y_error`` raises ValueError naming the pair and object where the reference raises UnboundLocalError (nothing to carry);
``remove_outliers`` prints its summary only (the per-frame and per-box prints are gone), takes the id bound once at entry and
raises RuntimeError BEFORE touching ``data`` when every box of an id below the bound would be deleted (the reference re-reads
the bound at every frame and camera and then silently stops visiting the ids above); packing refuses with ValueError an entry
whose key is not ``"{camera}_{id}"`` of its own datum, whose camera is not in ``cameras``, or whose x, y or timestamp is not
finite; ids that are not Python / numpy integers are ignored; ``estimate_projection_error`` returns two empty lists for three
or more cameras without a single id (the reference never leaves its while loop there); ``interpolate`` raises KeyError before touching ``data`` when a
time stamp it needs is missing from ``all_ts``.
"""
import numpy as np

from datareader import _cuda, _download, _upload
from retinanet_mi355x import ops

METHODS = ("estimate_ts_bias", "est_y_error", "estimate_projection_error", "remove_outliers", "interpolate", "interpolate_all",
           "unbias_timestamps", "get_unused_id", "count_classes")
COL_X, COL_Y, COL_T = 0, 1, 2                                  # the packed columns


def get_unused_id(self):
    """:894-907: the first non-negative integer that is not the ``id`` of any datum."""
    used = set()
    for frame_data in self.data:
        for item in frame_data.values():
            used.add(item["id"])
    new_id = 0
    while new_id in used:
        new_id += 1
    return new_id


def count_classes(self):
    """:2235-2247."""
    classes = {}
    for frame_data in self.data:
        for item in frame_data.values():
            classes[item["class"]] = classes.get(item["class"], 0) + 1
    print("Class counts:")
    for key in classes:
        print("{}:{}".format(key, classes[key]))


def _is_index(v):
    return (type(v) is int or isinstance(v, np.integer)) and not isinstance(v, (bool, np.bool_))


def pack_tracklets(data, names, ids=None):
    """One pass over ``data`` -> the CSR table of tracklets: offsets int64 [n_ids * C + 1] (tracklet = object * C + camera), cols
    fp64 [R,3] (x, y, timestamp), frame int32 [R] (ascending inside a tracklet), and per row its key, datum, object slot and
    camera.  ``ids``: the object ids, in slot order (default: ``range(first unused id)``, what the reference visits).  Raises
    ValueError, naming frame and key, for an entry whose key is not "{camera}_{id}" of its own datum, whose camera is not in
    ``names`` or whose x, y or timestamp is not finite -- before anything is packed."""
    cam_index = {}
    for i, n in enumerate(names):
        cam_index.setdefault(n, i)
    frames, keys, items, cams, oids, xyt = [], [], [], [], [], []
    for f, frame_data in enumerate(data):
        for key, item in frame_data.items():
            try:
                cam, oid = item["camera"], item["id"]
                x, y, t = float(item["x"]), float(item["y"]), float(item["timestamp"])
            except (KeyError, TypeError, IndexError, ValueError):
                raise ValueError("frame {}: entry {!r} is not a datum with camera, id, x, y and timestamp".format(f, key))
            if key != "{}_{}".format(cam, oid):
                raise ValueError("frame {}: key {!r} is not \"{}_{}\", the camera and id of its own datum".format(f, key, cam, oid))
            if cam not in cam_index:
                raise ValueError("frame {}: key {!r} names camera {!r}, which is not one of the cameras".format(f, key, cam))
            frames.append(f)
            keys.append(key)
            items.append(item)
            cams.append(cam_index[cam])
            oids.append(oid)
            xyt += (x, y, t)
    xyt = np.array(xyt, np.float64).reshape(-1, 3)
    bad = np.nonzero(~np.isfinite(xyt).all(axis=1))[0]
    if len(bad):
        raise ValueError("frame {}: key {!r} has an x, y or timestamp that is not finite".format(frames[bad[0]], keys[bad[0]]))
    if ids is None:
        used, n = set(oids), 0
        while n in used:
            n += 1
        ids = range(n)
    ids = list(ids)
    slot_of = {oid: j for j, oid in enumerate(ids)}
    C = len(names)
    slot = np.array([slot_of.get(o, -1) if _is_index(o) else -1 for o in oids], np.int64).reshape(-1)
    rows = np.nonzero(slot >= 0)[0]
    track = slot[rows] * C + np.array(cams, np.int64).reshape(-1)[rows]
    order = np.argsort(track, kind="stable")                    # frames stay ascending inside a tracklet
    rows, track = rows[order], track[order]
    offsets = np.zeros(len(ids) * C + 1, np.int64)
    np.cumsum(np.bincount(track, minlength=len(ids) * C), out=offsets[1:])
    return dict(offsets=offsets, cols=np.ascontiguousarray(xyt[rows]), frame=np.array(frames, np.int32).reshape(-1)[rows],
                keys=[keys[r] for r in rows], items=[items[r] for r in rows], slot=track // max(C, 1), cam=track % max(C, 1),
                ids=ids, n_cam=C, n_frames=len(data))


def _names(self):
    return [camera.name for camera in self.cameras]


def _device(self):
    return _cuda(getattr(self, "device", None))


def pair_samples(self, key_col, val0, val1=-1, device=None):
    """The sample block of every (camera pair, object) -> (flags uint8 [P, n_ids, 5], values fp64 [P, n_ids, 5, 4]) on the host
    (``ops.label_pair_samples``), or (None, None) when there is no pair or no object."""
    dev = _device(self) if device is None else device
    tab = pack_tracklets(self.data, _names(self))
    if tab["n_cam"] < 2 or len(tab["ids"]) == 0:
        return None, None
    d_off, d_cols = _upload(dev, [tab["offsets"], tab["cols"]])
    flags, values, status = ops.label_pair_samples(d_off, d_cols, tab["n_cam"], key_col, val0, val1)
    h_status, h_flags, h_values = _download([status, flags, values])
    ops.label_check(int(h_status[0]))
    return h_flags, h_values


def _pair(flags, values, cam_idx, prev_idx):
    """(guard, found cur, found prev, values [n,4]) of one pair, flat in the reference's order: objects ascending, points 0..4."""
    if flags is None:
        e = np.zeros(0, bool)
        return e, e, e, np.zeros((0, 4))
    p = ops.label_pair_index(cam_idx, prev_idx)
    fl = flags[p].reshape(-1)
    return (fl & ops.LABEL_GUARD) != 0, (fl & ops.LABEL_FOUND_CUR) != 0, (fl & ops.LABEL_FOUND_PREV) != 0, values[p].reshape(-1, 4)


def estimate_ts_bias(self):
    """:1845-1947.  Sets ``ts_bias``; -> per camera ``(prev_cam index, mean, std, n)`` of the pair it used, None for camera 0
    and for a camera without a partner (its ``ts_bias`` entry keeps its old value)."""
    names = _names(self)
    flags, values = pair_samples(self, COL_X, COL_T)
    self.ts_bias[0] = 0
    used = [None] * len(names)
    for cam_idx in range(1, len(names)):
        cam = names[cam_idx]
        decrement = 1
        while True:
            prev_cam = names[cam_idx - decrement]
            _, cur, prv, v = _pair(flags, values, cam_idx, cam_idx - decrement)
            keep = cur & prv & (v[:, 0] != 0) & (v[:, 1] != 0)                 # `if time and prev_time`: 0.0 is dropped like None
            diffs = v[keep, 0] - v[keep, 1]
            if len(diffs) > 0:
                avg_diff = np.mean(diffs)
                stdev = np.std(diffs)
                abs_bias = self.ts_bias[cam_idx - decrement] - avg_diff
                print("Camera {} ofset relative to camera {}: {}s ({}s absolute)".format(cam, prev_cam, avg_diff, abs_bias))
                self.ts_bias[cam_idx] = abs_bias
                used[cam_idx] = (cam_idx - decrement, avg_diff, stdev, len(diffs))
                break
            print("No matching points for cameras {} and {}".format(cam, prev_cam))
            decrement += 1
            if cam_idx - decrement < 0:
                break
    print("Done)")
    return used


def _carry_forward(vals, found, carry, what, cam, prev_cam, obj):
    """vals where found, else the latest found value before it (``carry`` ahead of the first) -> (filled, new carry)."""
    if len(vals) == 0:
        return vals, carry
    idx = np.maximum.accumulate(np.where(found, np.arange(len(vals)), -1))
    if idx[0] < 0 and carry is None:
        raise ValueError("est_y_error: no crossing and no earlier {} to reuse for cameras {} and {}, object {} "
                         "(the reference raises UnboundLocalError here)".format(what, cam, prev_cam, obj[0]))
    filled = np.where(idx >= 0, vals[np.maximum(idx, 0)], np.float64(0.0 if carry is None else carry))
    return filled, filled[-1]


def est_y_error(self):
    """:1950-2036 -> (all_diffs = the mean |y2 - y1| of every pair that has samples, per pair (cam, cam - 1) its (mean, std)
    or None)."""
    names = _names(self)
    flags, values = pair_samples(self, COL_X, COL_Y)
    all_diffs, stats = [], []
    y1_carry = y2_carry = None
    for cam_idx in range(1, len(names)):
        cam, prev_cam = names[cam_idx], names[cam_idx - 1]
        guard, cur, prv, v = _pair(flags, values, cam_idx, cam_idx - 1)
        at = np.nonzero(guard)[0]                                              # every point of a guarded object gives a diff
        obj = at // ops.LABEL_POINTS
        y1, y1_carry = _carry_forward(v[at, 0], cur[at], y1_carry, "y1", cam, prev_cam, obj)
        y2, y2_carry = _carry_forward(v[at, 1], prv[at], y2_carry, "y2", cam, prev_cam, obj)
        diffs = np.abs(y2 - y1)
        if len(diffs) > 0:
            avg_diff = np.mean(diffs)
            stdev = np.std(diffs)
            print("Camera {} and {} average y-error: {}ft ({})ft stdev".format(cam, prev_cam, avg_diff, stdev))
            all_diffs.append(avg_diff)
            stats.append((avg_diff, stdev))
        else:
            print("No matching points for cameras {} and {}".format(cam, prev_cam))
            stats.append(None)
    if len(all_diffs) > 0:
        print("Average y-error over all cameras: {}".format(sum(all_diffs) / len(all_diffs)))
    return all_diffs, stats


def estimate_projection_error(self, reverse_curve_offset=False):
    """:2249-2357 -> (x_errors, y_errors), lists of np.float64 in the reference's order: cam, partner, object, point."""
    names = _names(self)
    flags, values = pair_samples(self, COL_T, COL_X, COL_Y)
    x_errors, y_errors = [], []
    n_ids = 0 if flags is None else flags.shape[1]
    for cam_idx in range(1, len(names)):
        # :2268-2355: `decrement += 1` sits inside the loop over objects, so one pass of the while loop advances it by the
        # number of ids: the partners are cam_idx - 1, cam_idx - 1 - n_ids, ... above camera 0 (without ids the reference
        # never leaves the loop; here there is nothing to visit)
        for decrement in range(1, cam_idx, max(n_ids, 1)) if n_ids else ():
            cam, prev_cam = names[cam_idx], names[cam_idx - decrement]
            _, cur, prv, v = _pair(flags, values, cam_idx, cam_idx - decrement)
            keep = cur & prv & (v[:, 0] != 0) & (v[:, 1] != 0)                 # `if cur_x and prev_x`
            cur_x, prev_x, cur_y, prev_y = (v[keep, k] for k in range(4))
            if reverse_curve_offset and len(cur_x):
                cur_y, prev_y = cur_y.tolist(), prev_y.tolist()                # Python floats: x**2 is the C library's pow there
                for i, (cx, px) in enumerate(zip(cur_x.tolist(), prev_x.tolist())):
                    direction = "EB" if cur_y[i] < 60 else "WB"                # of the current camera's y, for both lookups
                    try:
                        p2, p1, p0 = self.poly_params["{}_{}".format(cam, direction)]
                        cur_y[i] -= p0 + p1 * cx + p2 * cx ** 2
                    except Exception:
                        print("Error 1458 search for it")
                    try:
                        p2, p1, p0 = self.poly_params["{}_{}".format(prev_cam, direction)]
                        prev_y[i] -= p0 + p1 * px + p2 * px ** 2
                    except Exception:
                        print("Error 1458 search for it")
                cur_y, prev_y = np.array(cur_y, np.float64), np.array(prev_y, np.float64)
            x_errors.extend(np.abs(cur_x - prev_x))
            y_errors.extend(np.abs(cur_y - prev_y))
    return x_errors, y_errors


def frames_visited(data, last_frame):
    """The frames the walk of ``remove_outliers`` reaches: it breaks at the first empty frame past ``last_frame``."""
    for f_idx in range(len(data)):
        if f_idx > last_frame and len(data[f_idx]) == 0:
            return f_idx
    return len(data)


def remove_outliers(self):
    """:2192-2233.  Deletes from ``data`` in place."""
    dev = _device(self)
    tab = pack_tracklets(self.data, _names(self))
    outliers = 0
    if len(tab["keys"]):
        d_off, d_cols, d_frame = _upload(dev, [tab["offsets"], tab["cols"], tab["frame"]])
        delete, status = ops.label_outliers(d_off, d_cols, d_frame, tab["n_frames"], frames_visited(self.data, self.last_frame))
        h_status, h_delete = _download([status, delete])
        ops.label_check(int(h_status[0]))
        h_delete = h_delete != 0
        n_ids = len(tab["ids"])
        gone = (np.bincount(tab["slot"], minlength=n_ids) > 0) & (np.bincount(tab["slot"][~h_delete], minlength=n_ids) == 0)
        if gone.any():
            raise RuntimeError("remove_outliers would delete every box of id {}: the reference then stops visiting the ids above "
                               "it part-way through; nothing was removed".format(tab["ids"][int(np.argmax(gone))]))
        for r in np.nonzero(h_delete)[0]:
            del self.data[tab["frame"][r]][tab["keys"][r]]
            outliers += 1
    print("Removed {} outlier data points".format(outliers))


def _all_ts_table(self, names, n_frames):
    table = np.full((n_frames, len(names)), np.nan)
    for f in range(min(n_frames, len(self.all_ts))):
        row = self.all_ts[f]
        for c, name in enumerate(names):
            if name in row:
                table[f, c] = float(row[name])
    return table


def _interpolate(self, ids):
    """Fills the gaps of the tracklets of ``ids`` (object outer, camera inner, frame ascending) -> the number of new boxes."""
    dev = _device(self)
    names = _names(self)
    tab = pack_tracklets(self.data, names, ids)
    same = tab["slot"][1:] * tab["n_cam"] + tab["cam"][1:] == tab["slot"][:-1] * tab["n_cam"] + tab["cam"][:-1]
    rows = int((np.diff(tab["frame"].astype(np.int64)) - 1)[same].sum()) if len(tab["keys"]) > 1 else 0
    if rows == 0:
        return 0
    table = _all_ts_table(self, names, tab["n_frames"])
    d_off, d_cols, d_frame, d_ts = _upload(dev, [tab["offsets"], tab["cols"], tab["frame"], table])
    got = ops.label_interpolate(d_off, d_cols, d_frame, d_ts, rows)
    out, src, frame, total, status = _download(list(got))
    ops.label_check(int(status[0]))
    if int(total[0]) != rows or (src < 0).any():
        raise RuntimeError("label_interpolate filled {} of {} rows".format(int(total[0]), rows))
    if np.isnan(out).any():
        u = int(np.nonzero(np.isnan(out).any(axis=1))[0][0])
        raise KeyError("all_ts has no time stamp of camera {} around frame {}".format(names[tab["cam"][src[u]]], int(frame[u])))
    for (x, y, _), r, f in zip(out.tolist(), src.tolist(), frame.tolist()):
        prev_box, cam_name = tab["items"][r], names[tab["cam"][r]]
        obj_idx = tab["ids"][tab["slot"][r]]
        self.data[f]["{}_{}".format(cam_name, obj_idx)] = {
            "x": x,
            "y": y,
            "l": prev_box["l"],
            "w": prev_box["w"],
            "h": prev_box["h"],
            "direction": prev_box["direction"],
            "id": obj_idx,
            "class": prev_box["class"],
            "timestamp": self.all_ts[f][cam_name],
            "camera": cam_name,
            "gen": "Interpolation"
        }
    return rows


def interpolate(self, obj_idx, verbose=True):
    """:780-836: fills the gaps of object ``obj_idx`` in every camera at the cameras' own time stamps."""
    _interpolate(self, [obj_idx])
    if verbose:
        print("Interpolated boxes for object {}".format(obj_idx))


def interpolate_all(self):
    """:1584-1585, every object below ``get_unused_id()`` in one launch -> the number of boxes added."""
    return _interpolate(self, None)


def unbias_timestamps(self):
    """:1591-1627: estimates the biases, then adds them to every label's timestamp and to ``all_ts``."""
    self.estimate_ts_bias()
    print(self.ts_bias)
    print(self.seq_keys)
    ts_bias_dict = dict([(self.seq_keys[i], self.ts_bias[i]) for i in range(len(self.seq_keys))])
    for f_idx in range(len(self.data)):
        for key in self.data[f_idx]:
            cam = self.data[f_idx][key]["camera"]
            try:
                self.data[f_idx][key]["timestamp"] += ts_bias_dict[cam]
            except Exception:
                print("KeyError")
    for f_idx in range(len(self.all_ts)):
        for i in range(len(self.seq_keys)):
            key = self.seq_keys[i]
            try:
                self.all_ts[f_idx][key] += self.ts_bias[i]
            except KeyError:
                print("KeyError")
    print("Un-biased timestamps")


class LabelAudit():
    """The functions above as methods: inherit it beside (or assign its members into) the reference's ``Annotator``."""
    get_unused_id = get_unused_id
    count_classes = count_classes
    estimate_ts_bias = estimate_ts_bias
    est_y_error = est_y_error
    estimate_projection_error = estimate_projection_error
    remove_outliers = remove_outliers
    interpolate = interpolate
    interpolate_all = interpolate_all
    unbias_timestamps = unbias_timestamps

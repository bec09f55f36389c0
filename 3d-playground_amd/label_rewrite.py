"""The passes of the reference's annotator (``seems_to_be_working.py``, class ``Annotator``) that ACT on what ``label_audit``
measures, on the GPU: ``replace_homgraphy`` (:1629-1730, the reference's spelling), ``replace_y`` (:1733-1776) with
``offset_box_y`` (:1779-1805), and ``replace_timestamps`` (:1546-1588).  All three keep the manually drawn boxes, rewrite them,
drop everything else and re-interpolate (``label_audit.interpolate_all``, one launch).

The functions take ``self`` like the methods they replace and read ``data``, ``cameras``, ``seq_keys``, ``all_ts``,
``poly_params``, ``last_frame`` and ``hg`` (a ``Homography_Wrapper``, or a single ``Homography``: no switch then); bind them
like ``label_audit``'s::

    import label_rewrite
    for name in label_rewrite.METHODS:
        setattr(Annotator, name, getattr(label_rewrite, name))

or inherit ``LabelRewrite`` beside ``LabelAudit``.

``replace_homgraphy`` is the slow one in the reference: per manual box three rounds of an 11 x 11 grid search over the box
centre (radii 50, 10, 2 ft), every round a ``torch.stack`` of 121 boxes through the NEW homography, the winner the centre
whose bottom footprint lands nearest the OLD box's image footprint.  Here one pass over ``data`` collects the manual boxes in
the reference's order, one packed copy sends them up with the four matrix tables, ``ops.label_rebase`` searches every box with
one wave (csrc/label_rebase.hip) and one copy brings centres, errors and indices back.  ``replace_y`` evaluates the curvature
polynomial of every box in one launch (``ops.label_offset_y``); ``replace_timestamps`` is host arithmetic plus the shared
re-interpolation.  There is no CPU path: without a device every function raises before it changes anything.

What differs from the reference: ``replace_homgraphy`` takes the new wrapper as an argument (``None``
unpickles ``EB_homography5.cpkl`` / ``WB_homography5.cpkl`` from the working directory, as the reference does), returns the
list of per-box minimum errors and prints their running average once at the end instead of every 100 frames; it refuses,
before any GPU work, a manual box whose camera is missing from either homography (KeyError) or whose x, y, l, w or h is not
finite (ValueError naming frame and key), and a status bit of the kernel raises RuntimeError with ``data`` and ``hg`` as they
were.  ``replace_y`` looks every polynomial up before it touches ``data`` (the reference dies half-way with a KeyError and
keeps the old ``data`` too) and squares x by multiplication where CPython calls the C library's ``pow`` (equal wherever that
``pow`` rounds x ** 2 correctly).  None of the three calls ``plot_all_trajectories`` (matplotlib).
"""
import copy
import pickle

import numpy as np

from datareader import _download, _upload
from label_audit import _device, _names, frames_visited, get_unused_id, interpolate_all, pack_tracklets  # noqa: F401
from retinanet_mi355x import ops

METHODS = ("replace_homgraphy", "replace_y", "offset_box_y", "replace_timestamps")
SEARCH_RAD, GRID_SIZE = 50, 11                                 # :1682-1683


def _visit(self, n_frames):
    """The truthy data of frames below ``n_frames`` in the reference's order -- frame, camera in ``self.cameras`` order, id
    ascending below ``get_unused_id()`` -- as (frame, key, datum, camera name) -- from one pass over ``data``: the reference
    forms every "{camera}_{id}" key for every frame."""
    cam_index = {}
    for i, n in enumerate(_names(self)):
        cam_index.setdefault(n, i)
    n_ids = get_unused_id(self)
    slot = {}

    def place(key):
        head, sep, tail = key.rpartition("_") if isinstance(key, str) else ("", "", "")
        if sep and head in cam_index and tail.isdigit() and str(int(tail)) == tail and int(tail) < n_ids:
            return cam_index[head], int(tail), head
        return None
    out = []
    for f in range(min(n_frames, len(self.data))):
        found = []
        for key, item in self.data[f].items():
            at = slot.get(key, False)
            if at is False:
                at = slot[key] = place(key)
            if at is not None and item:
                found.append((at[0], at[1], key, item, at[2]))
        found.sort(key=lambda e: e[:2])
        out.extend((f, key, item, cam) for _, _, key, item, cam in found)
    return out


def _sides(hg):
    """(hg1, hg2 or None) of a Homography_Wrapper or a single Homography."""
    return getattr(hg, "hg1", hg), getattr(hg, "hg2", None)


def _P_table(side, names, used):
    """fp64 [C,12]: the P of every camera in ``used`` (KeyError if the homography lacks it), zeros for the others."""
    table = np.zeros((len(names), 12), np.float64)
    for c, name in enumerate(names):
        if name in used:
            if name not in side.correspondence:
                raise KeyError("camera {} has manual boxes and no correspondence in the homography".format(name))
            table[c] = np.asarray(side.correspondence[name]["P"], np.float64).reshape(12)
    return table


def load_homography(hid=5):
    """:1632-1637: the replacement wrapper from the two pickles of the working directory."""
    from homography import Homography_Wrapper
    with open("EB_homography{}.cpkl".format(hid), "rb") as f:
        hg1 = pickle.load(f)
    with open("WB_homography{}.cpkl".format(hid), "rb") as f:
        hg2 = pickle.load(f)
    return Homography_Wrapper(hg1=hg1, hg2=hg2)


def replace_homgraphy(self, hg_new=None, grid_size=GRID_SIZE):
    """:1629-1730.  Re-centres every manual box of frames <= ``last_frame`` under ``hg_new``, drops the rest, sets ``hg`` and
    re-interpolates -> the minimum reprojection error of every box, in the reference's order."""
    if hg_new is None:
        hg_new = load_homography()
    names = _names(self)
    boxes = []
    for f, key, obj, cam in _visit(self, self.last_frame + 1):
        if obj["gen"] == "Manual":                              # :1672: a datum without "gen" raises KeyError
            boxes.append((f, key, obj, cam))
    state = np.array([[float(o[k]) for k in ("x", "y", "l", "w", "h", "direction")] for _, _, o, _ in boxes],
                     np.float64).reshape(-1, 6)
    bad = np.nonzero(~np.isfinite(state[:, :5]).all(axis=1))[0]
    if len(bad):
        raise ValueError("frame {}: key {!r} has an x, y, l, w or h that is not finite".format(boxes[bad[0]][0], boxes[bad[0]][1]))
    used = {cam for _, _, _, cam in boxes}
    tables = []
    for hg in (self.hg, hg_new):
        hg1, hg2 = _sides(hg)
        tables += [_P_table(hg1, names, used), None if hg2 is None else _P_table(hg2, names, used)]
    dev = _device(self)                                         # every refusal above comes before any GPU work
    errors = []
    new_data = [{} for _ in range(min(self.last_frame + 1, len(self.data)))]
    if boxes:
        index = {n: c for c, n in reversed(list(enumerate(names)))}
        cam = np.array([index[c] for _, _, _, c in boxes], np.int32)
        radii = np.array(ops.label_rebase_radii(SEARCH_RAD), np.float64)
        present = [t for t in tables if t is not None]
        up = _upload(dev, [state, cam, radii] + present)
        mats = iter(up[3:])
        P1o, P2o, P1n, P2n = (None if t is None else next(mats) for t in tables)
        centre, err, _, status = ops.label_rebase(up[0], up[1], P1o, P2o, P1n, P2n, up[2], grid_size)
        h_status, h_centre, h_err = _download([status, centre, err])
        ops.label_check(int(h_status[0]))
        errors = h_err.tolist()
        for (f, key, obj, _), (x, y) in zip(boxes, h_centre.tolist()):
            base = copy.deepcopy(obj)                           # :1674, :1711-1714
            base["x"] = x
            base["y"] = y
            new_data[f][key] = base
    self.data = new_data                                        # :1722-1724
    self.hg = hg_new
    interpolate_all(self)
    all_errors = [0] + errors                                   # :1650
    print("Re-based {} manual boxes. Average error: {}".format(len(errors), sum(all_errors) / len(all_errors)))
    return errors


def offset_box_y(self, box, reverse=False):
    """:1779-1805, one box on the host."""
    camera = box["camera"]
    direction = box["direction"]
    x = box["x"]
    direct = "_EB" if direction == 1 else "_WB"
    key = camera + direct
    p2, p1, p0 = self.poly_params[key]
    y_offset = x**2*p2 + x*p1 + p0
    if direction == -1:
        y_straight_offset = self.hg.hg2.correspondence[camera]["space_pts"][0][1]
        y_offset -= y_straight_offset
    if not reverse:
        box["y"] -= y_offset
    else:
        box["y"] += y_offset
    return box


def replace_y(self, reverse=False):
    """:1733-1776.  ``offset_box_y`` of every box whose "gen" is absent or "Manual", in one launch; the rest is dropped and
    re-interpolated."""
    n_frames = frames_visited(self.data, self.last_frame)
    boxes = [b for b in _visit(self, n_frames) if "gen" not in b[2].keys() or b[2]["gen"] == "Manual"]      # :1760
    xy, coef, straight, direction = [], [], [], []
    for f, key, obj, cam in boxes:
        d = obj["direction"]
        p2, p1, p0 = self.poly_params[obj["camera"] + ("_EB" if d == 1 else "_WB")]       # KeyError before data is touched
        coef.append((float(p2), float(p1), float(p0)))
        straight.append(float(self.hg.hg2.correspondence[obj["camera"]]["space_pts"][0][1]) if d == -1 else 0.0)
        direction.append(1 if d == 1 else (-1 if d == -1 else 0))
        xy.append((float(obj["x"]), float(obj["y"])))
    dev = _device(self)
    new_data = [{} for _ in range(n_frames)]
    if boxes:
        up = _upload(dev, [np.array(xy, np.float64).reshape(-1, 2), np.array(coef, np.float64).reshape(-1, 3),
                           np.array(straight, np.float64), np.array(direction, np.int32)])
        y, = _download([ops.label_offset_y(up[0], up[1], up[2], up[3], reverse)])
        if not np.isfinite(y).all():
            i = int(np.nonzero(~np.isfinite(y))[0][0])
            raise ValueError("frame {}: key {!r} has no finite y after its offset".format(boxes[i][0], boxes[i][1]))
        for (f, key, obj, _), v in zip(boxes, y.tolist()):
            base = copy.deepcopy(obj)
            base["y"] = v
            new_data[f][key] = base
    self.data = new_data                                        # :1768
    interpolate_all(self)


def replace_timestamps(self):
    """:1546-1588.  Puts every camera on its nominal frame rate, overwrites every label's timestamp, keeps the boxes whose
    "gen" is absent or "Manual" and re-interpolates."""
    _device(self)
    start_ts = [self.all_ts[0][key] for key in self.seq_keys]
    spans = [self.all_ts[-1][key] - self.all_ts[0][key] for key in self.seq_keys]
    frame_count = len(self.all_ts)
    fps_nom = [frame_count / spans[i] for i in range(len(spans))]
    print(fps_nom)
    for i in range(len(self.all_ts)):
        for j in range(len(self.seq_keys)):
            key = self.seq_keys[j]
            self.all_ts[i][key] = start_ts[j] + 1.0 / fps_nom[j] * i
    new_data = []
    for f_idx in range(len(self.data)):
        new_data.append({})
        for key in self.data[f_idx]:
            cam = self.data[f_idx][key]["camera"]
            self.data[f_idx][key]["timestamp"] = self.all_ts[f_idx][cam]
            if "gen" in self.data[f_idx][key].keys() and self.data[f_idx][key]["gen"] != "Manual":
                continue
            new_data[f_idx][key] = copy.deepcopy(self.data[f_idx][key])
    self.data = new_data
    interpolate_all(self)
    print("Replaced timestamps")


class LabelRewrite():
    """The functions above as methods: inherit it beside (or assign its members into) the reference's ``Annotator``."""
    replace_homgraphy = replace_homgraphy
    replace_y = replace_y
    offset_box_y = offset_box_y
    replace_timestamps = replace_timestamps

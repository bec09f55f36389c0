"""Drop-in for the data half of the reference's ``datareader.py``: ``Data_Reader(data_csv, homography, metric=False)`` reads a
3D tracking CSV (the file ``results_csv.write_results_csv`` writes) into ``data`` -- a list, sorted by unique rounded
timestamp, of ``{id: datum}`` dicts with the reference's thirteen keys --, ``reinterpolate(frequency, save)`` resamples every
track to a fixed rate and ``write_to_file(save_file)`` writes the file again.  Attributes as the reference: ``hg``, ``d_idx``,
``class_colors``, ``classes``, ``cameras``, ``data``.

The reference interpolates in a Python double loop over instants and ids (datareader.py:411-434) and rewrites the file with
two single-box homography calls per row (:530-550).  Here the host keeps what is serial and cheap -- the CSV parser
(:147-230, to the letter) and the walk over output instants (:406-444: ``output_time += 1.0/frequency`` accumulated one step
at a time, the frame pair each instant falls in, the "Time Error!" print), bit-equal by construction -- and everything
proportional to rows runs in csrc/datareader.hip: one packed upload, ``ops.reinterp_mate`` / ``reinterp_offsets`` /
``reinterp_rows`` (or ``ops.track_rows`` for the rewrite), one copy back.  The interpolated values are fp64 with one rounding
per operation, i.e. Python's; the reference's weights are kept as written, which put the NEXT frame's value at ``t == ts``.
The rows of the file come from ``results_csv.results_rows``, the formatter of the tracker's own result file.  There is no CPU
path.

Differences a caller can see: ``reinterpolate`` writes to ``save`` (the reference ignores the argument and
always writes its default name, :450-451; the default value is that name, so a call without arguments behaves the same);
``frequency <= 0`` raises ValueError (the reference loops forever); ``Camera_Wrapper``, ``plot_labels``, ``plot_in`` and
``test_integrity`` raise NotImplementedError (cv2 video I/O); the per-instant progress print of ``write_to_file`` is gone.
"""
import csv
import re

import numpy as np
import torch

import results_csv
from retinanet_mi355x import ops

FIELDS = ("x", "y", "l", "w", "h", "v")                        # datareader.py:426: the interpolated keys, in the packed order
DEFAULT_SAVE = "reinterpolated_3D_tracking_outputs.csv"        # :401, :451
_NO_VIDEO = "{} reads or draws video frames through cv2 (datareader.py:{}); video I/O is outside this package"


class Camera_Wrapper():
    def __init__(self, sequence, ds=2):
        raise NotImplementedError(_NO_VIDEO.format("Camera_Wrapper", "24-89"))


def test_integrity(sequence):
    raise NotImplementedError(_NO_VIDEO.format("test_integrity", "586-632"))


test_integrity.__test__ = False                                # a reference function name, not a test


# ------------------------------------------------------------------------------------------------ host <-> device blocks
def _upload(device, arrays):
    """Host arrays -> device tensors through ONE copy: the arrays are laid end to end (8-byte aligned) in one byte block."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    starts, size = [], 0
    for a in arrays:
        starts.append(size)
        size += (a.nbytes + 7) // 8 * 8
    block = np.zeros(max(size, 8), np.uint8)
    for a, s in zip(arrays, starts):
        block[s:s + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(block).to(device)
    return [dev[s:s + a.nbytes].view(torch.from_numpy(np.empty(0, a.dtype)).dtype).reshape(a.shape) for a, s in zip(arrays, starts)]


def _download(tensors):
    """Device tensors -> host arrays through ONE copy."""
    flat = []
    for t in tensors:
        b = t.contiguous().reshape(-1).view(torch.uint8)
        pad = -b.numel() % 8
        flat.append(b if pad == 0 else torch.cat((b, b.new_zeros(pad))))
    host = torch.cat(flat).cpu().numpy()
    out, s = [], 0
    for t, b in zip(tensors, flat):
        n = t.numel() * t.element_size()
        out.append(host[s:s + n].view(torch.empty(0, dtype=t.dtype).numpy().dtype).reshape(tuple(t.shape)))
        s += b.numel()
    return out


def pack_frames(data):
    """``Data_Reader.data`` as flat arrays, frames and rows in their dict order: offsets int64 [F+1], ids int64 [R] (the dict
    keys, which is what the reference mates by), fields fp64 [R,6], frame_ts fp64 [F] (the timestamp of a frame's FIRST datum,
    as ``__next__`` reads it; NaN for an empty frame), and the datum of every row."""
    offsets, ids, rows, frame_ts = [0], [], [], []
    for frame in data:
        first = True
        for key, item in frame.items():
            if first:
                frame_ts.append(item["timestamp"])
                first = False
            ids.append(key)
            rows.append(item)
        if first:
            frame_ts.append(np.nan)
        offsets.append(len(rows))
    fields = np.array([[item[k] for k in FIELDS] for item in rows], np.float64).reshape(-1, 6)
    return dict(offsets=np.asarray(offsets, np.int64), ids=np.asarray(ids, np.int64).reshape(-1), fields=fields,
                frame_ts=np.asarray(frame_ts, np.float64).reshape(-1), rows=rows, keys=ids)


def resample_packed(offsets, ids, fields, frame_ts, inst_a, inst_time, device):
    """The device half of ``reinterpolate``: host arrays in, host arrays out -> (out_fields fp64 [n,6], out_src int32 [n] (the
    input row), out_inst int32 [n] (the instant), prefix int64 [T+1]), rows in the reference's order.  Raises RuntimeError when a
    kernel refused an index (ops.reinterp_check); nothing is returned then."""
    offsets, inst_a = np.asarray(offsets, np.int64).reshape(-1), np.asarray(inst_a, np.int32).reshape(-1)
    sizes = np.diff(offsets)
    ok = inst_a[(inst_a >= 0) & (inst_a < len(sizes))]
    upper = int(np.clip(sizes[ok], 0, None).sum())             # every row of every instant's frame: no read-back in between
    d_off, d_ids, d_fields, d_ts, d_a, d_time = _upload(device, [offsets, np.asarray(ids, np.int64).reshape(-1),
                                                                 np.asarray(fields, np.float64).reshape(-1, 6),
                                                                 np.asarray(frame_ts, np.float64).reshape(-1), inst_a,
                                                                 np.asarray(inst_time, np.float64).reshape(-1)])
    mate, status = ops.reinterp_mate(d_off, d_ids)
    _, prefix, status = ops.reinterp_offsets(d_off, mate, d_a, status=status)
    out_fields, out_src, out_inst, status = ops.reinterp_rows(d_off, d_ts, d_fields, mate, d_a, d_time, prefix, upper, status=status)
    h_status, h_prefix, h_fields, h_src, h_inst = _download([status, prefix, out_fields, out_src, out_inst])
    ops.reinterp_check(int(h_status[0]))
    n = int(h_prefix[-1])
    return h_fields[:n], h_src[:n], h_inst[:n], h_prefix


def _matrices(hg, cameras, device):
    """(P, P2 or None, mat_index) for per-row camera names, through the homography's own matrix stacking."""
    if hasattr(hg, "hg1"):                                     # Homography_Wrapper: the second set switches on y > 60
        return hg._pair("P", list(cameras), device)
    P, idx = hg._matrices("P", list(cameras), device)
    return P, None, idx


def project_rows(hg, fields, direction, cameras, device):
    """The device half of ``write_to_file``: fields fp64 [N,6], direction [N], one camera name per row -> host arrays (state
    fp32 [N,7], space fp32 [N,4,2], im fp64 [N,8,2], box fp64 [N,4], keep uint8 [N])."""
    fields = np.asarray(fields, np.float64).reshape(-1, 6)
    P, P2, idx = _matrices(hg, cameras, device)
    d_fields, d_dir = _upload(device, [fields, np.asarray(direction, np.float64).reshape(-1)])
    got = ops.track_rows(d_fields, d_dir, P, P2, idx)
    state, space, im, box, keep, status = _download(list(got))
    ops.reinterp_check(int(status[0]))
    return state, space, im, box, keep


class Data_Reader():
    def __init__(self, data_csv, homography, metric=False):
        """data_csv - a tracking data file in the template of write_results_csv; homography - a Homography or
        Homography_Wrapper holding a correspondence for every camera the file names."""
        self.hg = homography
        self.d_idx = 0
        self.class_colors = [(0, 255, 0), (255, 0, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 100, 0),
                             (255, 50, 0), (0, 255, 150), (0, 255, 100), (0, 255, 50)]
        names = ["sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer"]
        self.classes = {n: i for i, n in enumerate(names)}
        self.classes["truck"] = 5
        self.classes.update({i: n for i, n in enumerate(names)})
        self.data = []
        data = {}
        with open(data_csv, "r") as f:
            in_headers = True
            for row in csv.reader(f):
                if in_headers:                                  # up to and including the "Frame #" row (:152-157)
                    if len(row) > 0 and row[0] == "Frame #":
                        in_headers = False
                        self.cameras = re.findall(r"(p\dc\d)", row[45])
                    continue
                try:                                            # :160-192: a row that fails anywhere here is skipped
                    x, y = float(row[39]), float(row[40])
                    w, l, h = float(row[42]), float(row[43]), float(row[44])
                    direction = int(float(row[35]))
                    vel = float(row[38])
                    obj_id = int(float(row[2]))
                    cls = row[3]
                    ts = np.round(float(row[1]), 4)
                    camera = row[36]
                    frame = row[0]
                    if camera == "":
                        camera = "p1c1"
                    if metric:
                        y, x, w, l, h, vel = y * 3.281, x * 3.281, w * 3.281, l * 3.281, h * 3.281, vel * 3.281
                    offsets = [float(cell) for cell in row[45].strip("[").strip("]").split(",")]
                    offsets = dict([(self.cameras[i], offsets[i]) for i in range(len(offsets))])
                except Exception:
                    continue
                datum = {"timestamp": ts, "id": obj_id, "class": cls, "x": x, "y": y, "l": l, "w": w, "h": h,
                         "direction": direction, "v": vel, "ts_bias": offsets, "camera": camera, "frame": frame}
                if ts in data:
                    data[ts][obj_id] = datum                    # a repeated (ts, id) replaces the datum, not its position
                else:
                    data[ts] = {obj_id: datum}
        self.data = [data[key] for key in sorted(data)]

    def _device(self):
        hg = getattr(self.hg, "hg1", self.hg)
        return torch.device(getattr(hg, "device", "cuda:0"))

    def __next__(self):
        """datareader.py:232-251 -> (this frame's dict (a shallow copy), its timestamp, the next frame's timestamp and dict, or
        None, None at the last frame); four Nones past the end."""
        try:
            if self.d_idx >= len(self.data):
                return None, None, None, None
            datum = self.data[self.d_idx].copy()
            ts = datum[list(datum.keys())[0]]["timestamp"]
            next_ts, next_datum = None, None
            if self.d_idx < len(self.data) - 1:
                following = self.data[self.d_idx + 1]
                next_ts = following[list(following.keys())[0]]["timestamp"]
                next_datum = following.copy()
            self.d_idx += 1
            return datum, ts, next_ts, next_datum
        except Exception:
            print(self.d_idx, self.data[self.d_idx])

    def plot_labels(self, im, boxes, state_boxes, classes, ids, speeds, directions, times):
        raise NotImplementedError(_NO_VIDEO.format("plot_labels", "253-290"))

    def plot_in(self, camera_sequences, framerate=30, savefile=None):
        raise NotImplementedError(_NO_VIDEO.format("plot_in", "293-399"))

    def _walk(self, frequency):
        """datareader.py:406-444 without the per-object body: -> (a, output_time) per output instant, a = the index in
        ``data`` of the frame the instant interpolates from (towards a + 1).  Serial, fp64, exactly as the reference writes it."""
        inst_a, inst_time = [], []
        ts_data, ts, next_ts, next_ts_data = next(self)
        output_time = ts
        while next_ts is not None:
            inst_a.append(self.d_idx - 1)
            inst_time.append(output_time)
            output_time += 1.0 / frequency
            while output_time > next_ts:
                ts_data, ts, next_ts, next_ts_data = next(self)
                if next_ts is None:
                    break
            if output_time < ts:
                print("Time Error!")
        return inst_a, inst_time

    def reinterpolate(self, frequency=30, save=DEFAULT_SAVE):
        """Overwrites ``data`` with a regular sampling of it: one dict per output instant, holding every object present in
        both frames around the instant (an instant without such an object keeps an empty dict); then writes ``save`` unless
        it is None."""
        if not frequency > 0:
            raise ValueError("reinterpolate needs frequency > 0, got {} (the reference never terminates there)".format(frequency))
        start = self.d_idx
        try:
            inst_a, inst_time = self._walk(frequency)
            pk = pack_frames(self.data)
            fields, src, inst, _ = resample_packed(pk["offsets"], pk["ids"], pk["fields"], pk["frame_ts"], inst_a, inst_time,
                                                   self._device())
        except Exception:
            self.d_idx = start                                  # nothing was replaced: the reader is where it was
            raise
        new_data = [{} for _ in inst_a]
        for j in range(len(src)):
            obj = pk["rows"][src[j]].copy()                    # class, direction, ts_bias, camera, frame, id: frame a's
            for k, name in enumerate(FIELDS):
                obj[name] = fields[j, k]
            obj["timestamp"] = inst_time[inst[j]]
            new_data[inst[j]][pk["keys"][src[j]]] = obj
        self.data = new_data
        self.d_idx = 0
        if save is not None:
            self.write_to_file(save_file=save)

    def file_rows(self):
        """The rows ``write_to_file`` writes, from ``data`` as it is now: one ops.track_rows launch, then results_rows."""
        items = [item for ts_data in self.data for item in ts_data.values()]
        if not items:
            return []
        cameras = [item["camera"] if "camera" in item else "p1c1" for item in items]
        fields = [[item[k] for k in FIELDS] for item in items]
        state, space, im, box, keep = project_rows(self.hg, fields, [item["direction"] for item in items], cameras, self._device())
        sel = [i for i in range(len(items)) if keep[i]]        # :535, decided on the fp32 state on the device
        kept = [items[i] for i in sel]
        return results_csv.results_rows([item["id"] for item in kept], [item["timestamp"] for item in kept], state[sel], space[sel],
                                        im[sel], [item["class"] for item in kept],
                                        [[item["ts_bias"][key] for key in item["ts_bias"].keys()] for item in kept],
                                        camera=[cameras[i] for i in sel], box=box[sel])

    def write_to_file(self, save_file="default_save_file.csv"):
        header = results_csv.RESULTS_HEADER + ["ts_bias for cameras {}".format(self.cameras)]
        rows = self.file_rows()                                 # before the file is opened: a refused input writes nothing
        with open(save_file, mode="w") as f:
            out = csv.writer(f, delimiter=",")
            out.writerow(header)
            out.writerows(rows)

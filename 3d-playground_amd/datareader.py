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

Beyond the reference: ``stitch(params, fill, save)`` joins the fragments a vehicle leaves behind when the tracker loses it and
fills the gaps (track_stitch.py, csrc/stitch.hip); ``smooth(kf_params, params, save)`` replaces every row's fields by the means of
a fixed-interval smoother over its track (track_smooth.py, csrc/smooth.hip); ``traffic_state(params)`` turns the rows into flow,
density and speed per lane over a space-time grid and into every row's leader, gap, headway and time to collision
(traffic_state.py, csrc/traffic.hip).

Differences a caller can see: ``reinterpolate`` writes to ``save`` (the reference ignores the argument and
always writes its default name, :450-451; the default value is that name, so a call without arguments behaves the same);
``frequency <= 0`` raises ValueError (the reference loops forever); the per-instant progress print of ``write_to_file`` is
gone.

The video half (:24-89, 253-399, 586-653) runs on frames a loader hands over, without cv2: ``Camera_Wrapper(source, ds,
reader)`` wraps an iterator of uint8 [h,w,3] frames that carries a ``.sequence`` string, reads the burnt-in time stamp through
a ``timestamp_utilities.TimestampReader`` and keeps the fp64 running frame on the device; ``test_integrity`` counts doubled
and skipped frames from an exact integer window sum (``ops.frame_absdiff``); ``plot_in(..., render={...})`` replays the file
over the cameras: the loop over time stamps (:308-399) stays on the host, a handful of floats per frame, and every frame is
shifted, projected, painted and tiled by ``mc3d_render.Replayer`` (csrc/replay.hip).  What still raises NotImplementedError,
because it is cv2 itself: a ``str`` source (video decoding), ``plot_in`` without ``render=`` (window display) or with
``savefile`` (the MPEG writer), and ``plot_labels`` (it takes and returns a host cv2 image; its label block is painted by the
replay).  Further differences: a first frame that no set reads takes 0 + 1/30.0 (the reader's previous stamps start at zero;
the reference raises TypeError on ``None + 1/30.0``); ``test_integrity`` takes ``n`` and ``save_dir`` (the reference: 1000 and
a hard-coded desktop path) and returns its counts; the drawing rules are mc3d_render's (its "Differences").
"""
import csv
import os
import re

import numpy as np
import torch

import results_csv
from retinanet_mi355x import ops

FIELDS = ("x", "y", "l", "w", "h", "v")                        # datareader.py:426: the interpolated keys, in the packed order
DEFAULT_SAVE = "reinterpolated_3D_tracking_outputs.csv"        # :401, :451
_NO_VIDEO = "{} reads or draws video frames through cv2 (datareader.py:{}); video I/O is outside this package"


def _cuda(device=None):
    dev = torch.device("cuda:0" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("the replay runs on an MI355X only: no usable device %s (no CPU fallback)" % (dev,))
    return dev


class Camera_Wrapper():
    """datareader.py:24-89 around a loader instead of cv2.VideoCapture: ``source`` is an iterator of uint8 [h,w,3] frames
    (device tensors, or host tensors / arrays uploaded here) with a ``.sequence`` string naming the camera (p?c?, digits);
    ``reader`` a ``TimestampReader(sets, 1)`` whose sets are tried in order (the reference tries two geometries).
    ``frame`` uint8 [H,W,3] on the device (ds == 2: the exact 2x reduction of ``ops.frame_ingest_half``), ``ts``, ``name``,
    ``all_ts``, ``running_frame`` fp64 [H,W,3] on the device, ``ds`` as the reference's.  One ``__next__``: at most one upload,
    the launches, one small copy back of (ts, status)."""

    def __init__(self, source, ds=2, reader=None, device=None):
        if isinstance(source, str):
            raise NotImplementedError(_NO_VIDEO.format("Camera_Wrapper", "24-89"))
        if reader is None:
            raise ValueError("Camera_Wrapper needs reader=timestamp_utilities.TimestampReader(sets, 1): the reference's "
                             "checksum tables are pickles at hard-coded paths and are not shipped")
        self.source, self.ds, self.reader = source, ds, reader
        self.device = _cuda(getattr(reader, "device", None) if device is None else device)
        self.frame = None
        self.ts = None
        self.status = None
        self.name = re.search(r"p\dc\d", source.sequence).group(0)
        self.all_ts = []
        self.running_frame = None

    def __iter__(self):
        return self

    def __next__(self):
        raw = next(self.source)                                 # StopIteration: the source has ended
        raw = raw if torch.is_tensor(raw) else torch.from_numpy(np.ascontiguousarray(raw))
        if raw.dim() != 3 or raw.shape[2] != 3 or raw.dtype != torch.uint8:
            raise ValueError("a frame is uint8 [h,w,3], got %s %s" % (raw.dtype, tuple(raw.shape)))
        raw = (raw if raw.is_cuda else raw.to(self.device)).contiguous()
        times, status = self.reader(raw.unsqueeze(0))           # every set in turn, else prev + 1/30.0 (:60-66)
        if self.ds == 2:
            raw = ops.frame_ingest_half(raw, keep_u8=True)[1][0]
        self.frame = raw
        first = self.running_frame is None
        if first:
            self.running_frame = torch.empty(raw.shape, dtype=torch.float64, device=raw.device)
        ops.running_frame(self.running_frame, raw, first)
        ts, st = torch.cat((times, status.to(torch.float64))).tolist()        # the one copy back
        self.ts, self.status = ts, int(st)
        if self.status == ops.TS_FELL_BACK:
            print("No timestamp parsed: {}".format(self.name))
        self.all_ts.append(self.ts)

    def release(self):
        for name in ("release", "close"):
            if hasattr(self.source, name):
                getattr(self.source, name)()
                return

    def __len__(self):
        return int(len(self.source))

    def skip(self, count):
        for i in range(count):
            next(self.source)                                   # cap.grab(): taken and not looked at
        next(self)


def absdiff_mean(total, H, W):
    """np.mean(|frame - prev|[100:500, 100:500, :]) from the window's exact integer sum; None for an empty window.  Every term
    of numpy's sum is an integer below 2^53, so one division of two exact operands is its value bit for bit."""
    count = ops.absdiff_window(H, W)
    return None if count == 0 else int(total) / count


def test_integrity(source, n=1000, save_dir=None, reader=None):
    """datareader.py:586-653: counts doubled time stamps, doubled frames, both, and skipped stamps over up to ``n`` frames of
    ``source`` (a loader, wrapped with ds = 1 and ``reader``, or a Camera_Wrapper).  -> dict of the five counts."""
    if isinstance(source, str):
        raise NotImplementedError(_NO_VIDEO.format("test_integrity", "586-632"))
    cam = source if isinstance(source, Camera_Wrapper) else Camera_Wrapper(source, ds=1, reader=reader)
    save = None
    if save_dir is not None:
        from PIL import Image
        os.makedirs(save_dir, exist_ok=True)

        def save(frame, i):
            Image.fromarray(frame.cpu().numpy()).save(os.path.join(save_dir, "{}_{}.png".format(cam.name, i)))
    counts = dict(doubled_ts=0, doubled_frame=0, doubled_both=0, skipped_ts=0, correct=0)
    try:
        next(cam)
        prev_ts, prev_frame = cam.ts, cam.frame.clone()
        for i in range(1, n):
            next(cam)
            ts, frame = cam.ts, cam.frame
            DTS = ts - prev_ts == 0
            mean = absdiff_mean(ops.frame_absdiff(frame, prev_frame).item(), frame.shape[0], frame.shape[1])
            DF = mean is not None and mean < 0.2
            STS = False
            if DTS and DF:
                counts["doubled_both"] += 1
            elif DTS:
                counts["doubled_ts"] += 1
            elif DF:
                counts["doubled_frame"] += 1
            elif (ts - prev_ts) > 0.05:
                counts["skipped_ts"] += 1
                STS = True
            else:
                counts["correct"] += 1
            if DTS or DF or STS:
                if save is not None:
                    save(frame, i)
                    save(prev_frame, i - 1)
                for k in (1, 2):                                # two more frames are consumed (:637-640)
                    next(cam)
                    if save is not None:
                        save(cam.frame, i + k)
            prev_frame = cam.frame.clone()
            prev_ts = cam.ts
    except StopIteration:
        pass                                                    # the source ended early
    print("Camera {} results for {} frames:".format(cam.name, n))
    print("Doubled timestamps occured {} times".format(counts["doubled_ts"]))
    print("Doubled both occured {} times".format(counts["doubled_both"]))
    print("Doubled frames occured {} times".format(counts["doubled_frame"]))
    print("Skipped timestamps occurred {} times".format(counts["skipped_ts"]))
    return counts


test_integrity.__test__ = False                                # a reference function name, not a test


def replay_walk(reader, cameras, max_frames=None):
    """The loop of plot_in (:308-399) without its drawing: a generator of (label instant index, ts_data, ts, [camera ts], [dt
    per camera]) per output frame.  ``reader``: the Data_Reader (its ``__next__``); ``cameras``: objects with ``ts``, ``name``
    and ``__next__``, already holding their first frame.  Ends when the labels run out, when a camera raises StopIteration or
    after ``max_frames`` frames.  Serial, Python floats, as the reference writes it."""
    ts_data, ts, next_ts, _ = next(reader)
    done = 0
    try:
        while max_frames is None or done < max_frames:
            max_time = max([cam.ts for cam in cameras])
            for cam in cameras:
                while cam.ts + 1 / 60.0 < max_time:
                    next(cam)
            if next_ts is None:
                break
            while max_time > next_ts:
                ts_data, ts, next_ts, _ = next(reader)
                if next_ts is None:
                    break
            stamps, dts = [], []
            for camera in cameras:
                try:
                    bias = ts_data[list(ts_data.keys())[0]]["ts_bias"][camera.name]
                except KeyError:
                    bias = 0
                stamps.append(camera.ts)
                dts.append(camera.ts + bias - ts)
            yield reader.d_idx - 1, ts_data, ts, stamps, dts
            done += 1
            next(cameras[0])
    except StopIteration:
        return


def pack_states(data):
    """Every datum of ``data`` as the fp32 row plot_in stacks (:338): (x, y, l, w, h, direction, v) -> (offsets int64 [F+1],
    state7 fp32 [R,7]), frames and rows in their dict order."""
    offsets, rows = [0], []
    for frame in data:
        rows += [[obj["x"], obj["y"], obj["l"], obj["w"], obj["h"], obj["direction"], obj["v"]] for obj in frame.values()]
        offsets.append(len(rows))
    return np.asarray(offsets, np.int64), np.asarray(rows, np.float64).reshape(-1, 7).astype(np.float32)


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
        """Refused: it takes and returns a host cv2 image.  Its label block (:262-290) is painted by the replay
        (``plot_in(..., render=...)``, mc3d_render.Replayer)."""
        raise NotImplementedError(_NO_VIDEO.format("plot_labels", "253-290"))

    def plot_in(self, sequences, framerate=10, savefile=None, render=None):
        """datareader.py:293-399 with the tracker's switch (PLOT=True -> params["render"]): ``render = {"out": directory or
        None, "size": (width, height) or None, "max_frames": int or None}`` replays the file over ``sequences`` -- a list of
        Camera_Wrappers, or of loaders wrapped here with ``TimestampReader(render["sets"], 1)``; ``render["swap_rb"]`` says
        the frames are B,G,R.  -> the number of frames rendered.  ``replayed``: the last canvas, uint8 RGB on the device;
        ``replay_log``: per output frame (label instant index, [camera ts], [dt per camera]).  Frames go to
        ``<out>/combined/00000.png ...``: one device -> host copy per written frame, none when ``out`` is None.  Without
        ``render`` (window display) and with ``savefile`` (the MPEG writer) it raises: both are cv2."""
        if render is None or savefile is not None:
            raise NotImplementedError(_NO_VIDEO.format("plot_in", "293-399"))
        import mc3d_render
        import timestamp_utilities as tsu
        dev = _cuda(self._device())
        cameras = []
        for sequence in sequences:
            cap = sequence if isinstance(sequence, Camera_Wrapper) else \
                Camera_Wrapper(sequence, reader=tsu.TimestampReader(render["sets"], 1, device=dev), device=dev)
            if cap.ts is None:
                next(cap)
            cameras.append(cap)
        self.replayed, self.replay_log = None, []
        if not cameras:
            return 0
        names = [cam.name for cam in cameras]
        P1, P2, idx = _matrices(self.hg, names, dev)
        P1 = P1.index_select(0, idx.long()).contiguous()
        P2 = None if P2 is None else P2.index_select(0, idx.long()).contiguous()
        offsets, state7 = pack_states(self.data)
        d_state7, = _upload(dev, [state7])                       # the whole file's rows, once
        H, W = cameras[0].frame.shape[:2]
        replayer = mc3d_render.Replayer(len(cameras), H, W, dev)
        writer = None if render.get("out") is None else mc3d_render.PngWriter(render["out"], [])
        for inst, ts_data, ts, stamps, dts in replay_walk(self, cameras, render.get("max_frames")):
            view = state7[offsets[inst]:offsets[inst + 1]]      # l, w, h of a view are the row's own
            lines = [[mc3d_render.replay_label_lines(view[i], obj["class"], obj["id"], ts + dt) for i, obj in enumerate(ts_data.values())]
                     for dt in dts]
            self.replayed = replayer.replay([cam.frame for cam in cameras], d_state7, int(offsets[inst]), len(view), dts, P1, P2,
                                            lines, render.get("size"), render.get("swap_rb", False))
            self.replay_log.append((inst, stamps, dts))
            if writer is not None:
                writer(self.replayed.cpu().numpy(), [])
        self.replayer = replayer
        return len(self.replay_log)

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

    def stitch(self, params=None, fill=True, save=None):
        """Beyond the reference: joins the fragments of one vehicle under one id (track_stitch.stitch_tracks; ``params`` overrides
        track_stitch.DEFAULTS) and, with ``fill``, fills the gap of every link.  Replaces ``data``, resets ``d_idx``, writes
        ``save`` unless it is None -> the report.  On an error nothing is replaced."""
        import track_stitch
        new_data, report = track_stitch.stitch_tracks(self.data, params, fill, self._device())
        self.data = new_data
        self.d_idx = 0
        if save is not None:
            self.write_to_file(save_file=save)
        return report

    def smooth(self, kf_params, params=None, save=None):
        """Beyond the reference: replaces x, y, l, w, h, v of every row by the means of a fixed-interval smoother over its track
        (track_smooth.smooth_tracks; ``kf_params`` as fit_filter.fit returns it, ``params`` overrides track_smooth.DEFAULTS).
        Replaces ``data``, resets ``d_idx``, writes ``save`` unless it is None -> the report.  On an error nothing is replaced."""
        import track_smooth
        new_data, report = track_smooth.smooth_tracks(self.data, kf_params, params, self._device())
        self.data = new_data
        self.d_idx = 0
        if save is not None:
            self.write_to_file(save_file=save)
        return report

    def traffic_state(self, params=None):
        """Beyond the reference: the traffic measures of ``data`` as it is now (traffic_state.py; ``params`` overrides
        traffic_state.DEFAULTS) -> {"fields": traffic_fields' dict (flow, density and speed per direction and lane over a space-time
        grid), "following": car_following's dict (leader, gap, headway and time to collision of every row)}.  ``data`` and ``d_idx``
        are left alone."""
        import traffic_state
        return {"fields": traffic_state.traffic_fields(self.data, params, self._device()),
                "following": traffic_state.car_following(self.data, params, self._device())}

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

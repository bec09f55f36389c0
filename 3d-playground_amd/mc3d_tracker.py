"""The reference's multi-camera tracker (``MC3D_crop_tracker.py``: ``MC_Crop_Tracker``) end to end on the GPU: frames ->
tracks -> result file, composed from the device-resident stages of this package::

    from mc3d_tracker import MC_Crop_Tracker
    trk = MC_Crop_Tracker(loaders, detector, kf_params, hg, class_dict, params=params, cd=crop_detector, PLOT=False)
    trk.track()
    trk.write_results_csv()

Same class name, constructor signature, ``params`` keys and defaults (:62-87) and attributes as the reference, so
``results_csv.write_results_csv`` binds unchanged.  ``__next__`` and ``time_sync_cameras`` restate :197-235, ``track``
restates :1051-1312 block by block: the detector's outputs go straight into ``mc3d_post.parse_detections`` and
``mc3d_track.associate``; a crop frame is ``ops.track_crop_prior`` (view 1/30 s ahead, nearest camera, per-track dt; csrc/
track_step.hip), ``Torch_KF.predict``, ``mc3d_post.crop_refine``, ``Torch_KF.update`` and ONE device -> host copy with the
confidences, classes and cameras for the host dictionaries; every frame ends with ``mc3d_track.prune`` and one
``rn_kf_view`` launch that writes the tracks at the frame's clock time into a device-resident track log.

Differences from the reference:
  * Frame sources.  ``sequences`` is a list of loader objects, not of video paths (a path string raises
    NotImplementedError: video decoding is cv2).  A loader has ``__next__`` -> the reference's chunk ``(frame_num, frame
    [3,H,W] float32 on the device, original_im or None, timestamp float or None)``, ``(-1, None, None, None)`` at the end;
    ``__len__``; and a string ``sequence`` searched with the reference's regex ``p\\dc\\d`` for the camera name.
    ``Frames4K`` adapts decoded 4K uint8 frames.
  * The time stamp table.  The reference overrides the stamps from a hard-coded pickle (:188-189, used at :228-230); here
    ``params["ts"]`` is that dict ``{sequence: [stamps]}``; without it ``time_sync_cameras`` uses the chunk's own stamp.
    ``None`` -> previous + 1/30 in both places, as :213-215 and :229-230.  A loader that ends inside
    ``time_sync_cameras`` ends the run (``frame_num = -1``); the reference falls into its ``except TypeError`` there and
    goes on with a stale frame.
  * The filter is ``Torch_KF(self.device, INIT=kf_params)`` on the GPU (``params["GPU"]`` picks the device, default the
    current one); the reference keeps it on the CPU (:103).
  * Refusals at construction, before any GPU work: ``PLOT=True`` and ``OUT is not None`` raise NotImplementedError (pass
    ``PLOT=False``, as the reference's own ``__main__`` does: these paths are cv2 drawing and image writers); a missing
    ``params["cam_centers"]`` raises ValueError; a camera without an entry in the homography raises KeyError.
  * A crop frame reached with ``cd=None`` raises RuntimeError naming ``cd``.
  * Output frames.  ``PLOT`` / ``OUT`` stay refused (a cv2 window and cv2 writers); the picture of ``plot()`` (:733-917) is
    asked for through ``params["render"]``, a dict with ``out`` (a directory for PNG frames in the reference's layout, or
    None), ``label_len`` (5), ``single_box`` (True), ``fancy_crop`` (True) and ``every`` (1: render every n-th frame).  The
    frame is rendered on the device (``mc3d_render.Renderer``) after the store block, under ``time_metrics["plot"]``, with
    the detections of the frame's own branch: the parsed ones on a detection frame, the refined boxes and crop windows on a
    crop frame (priors, with ``single_box=False``, on crop frames only).  ``rendered`` holds the last canvas on the device
    (uint8 RGB, all cameras tiled), ``original_ims[i]`` camera i's window of it.  One device -> host copy per rendered frame
    (the label numbers), a second one only when frames are written.  Without the key nothing of this runs.
  * ``all_confs`` / ``all_cameras`` receive Python numbers, as ``mc3d_track`` already does (the reference appends the whole
    ``confs`` tensor at :1250; both lists are write-only).
  * ``all_tracks`` is materialised lazily from the device track log: one device -> host copy of the whole log the first
    time it is read after a frame; a list of ``[id, time, state tensor (CPU)]`` as the reference's.  ``params["log_rows"]``
    sizes the log's first chunk (chunks double; old chunks are kept, nothing is copied).
  * No ``torch.cuda.synchronize()`` / ``empty_cache()`` per frame (:1295-1296).
Kept on purpose: what ``mc3d_track`` lists (swapped ``increment_fslds`` arguments, unmatched rows rolled by ``dt_default``,
all-tie ``remove_overlaps``); ``guess_heights`` called with integer labels always gives 5; a crop frame does nothing when
no track is alive; ``d = -1`` means every frame (``x % -1 == 0``).  Known difference: ``Torch_KF.predict`` with a
per-object dt does not reproduce the reference's Q broadcast at exactly 6 rows (tests/track_cases.py: sequence).
"""
import re
import time

import numpy as np
import torch

import mc3d_post
import mc3d_track
import results_csv
from retinanet_mi355x import ops as _ops
from util_track.kf import Torch_KF


class TrackLog:
    """The tracks of every frame, [rows,7] float32 on the device.  ``slot(n)`` hands out the next n rows of the current
    chunk (a new chunk of twice the size when they do not fit; old chunks stay where they are), ``commit`` records the
    frame's ids and clock time on the host.  ``tracks()`` -> the reference's ``all_tracks`` list, from one device -> host
    copy of the whole log, cached until the next commit."""

    def __init__(self, device, first_rows=4096):
        self.device = torch.device(device)
        self.first_rows = max(1, int(first_rows))
        self.chunks, self.used = [], []           # device buffers and the rows taken of each
        self.frames = []                          # (ids, clock_time) per committed frame, in log order
        self.copies = 0                           # device -> host copies made by tracks()
        self._pending = None
        self._cache = None

    def __len__(self):
        return sum(self.used)

    def slot(self, n):
        if not self.chunks or self.used[-1] + n > len(self.chunks[-1]):
            rows = max(n, 2 * len(self.chunks[-1]) if self.chunks else self.first_rows)
            self.chunks.append(torch.empty((rows, 7), dtype=torch.float32, device=self.device))
            self.used.append(0)
        self._pending = n
        return self.chunks[-1][self.used[-1]:self.used[-1] + n]

    def commit(self, ids, clock_time):
        assert self._pending == len(ids)
        self.used[-1] += self._pending
        self.frames.append((list(ids), clock_time))
        self._pending, self._cache = None, None

    def tracks(self):
        if self._cache is None:
            parts = [c[:u] for c, u in zip(self.chunks, self.used) if u]
            out = []
            if parts:
                host = (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu()
                self.copies += 1
                r = 0
                for ids, clock_time in self.frames:
                    for oid in ids:
                        out.append([oid, clock_time, host[r]])
                        r += 1
            self._cache = out
        return self._cache


class Frames4K:
    """Loader over decoded 4K frames: ``frames_u8_iter`` yields uint8 [2H,2W,3] frames (device tensors, or host tensors that
    are uploaded here); every ``__next__`` is one ``ops.load_frames_4k`` call -- the burnt-in time stamp through ``reader`` (a
    ``timestamp_utilities.TimestampReader`` for one camera) and the 2x reduction + normalisation -- and one small copy of
    (stamp, status).  A status other than TS_READ gives ``timestamp = None``."""

    def __init__(self, sequence, frames_u8_iter, reader):
        self.sequence = sequence
        self.reader = reader
        self._n = len(frames_u8_iter) if hasattr(frames_u8_iter, "__len__") else 0
        self._it = iter(frames_u8_iter)
        self.frame_num = -1

    def __len__(self):
        return self._n

    def __iter__(self):
        return self

    def __next__(self):
        try:
            f = next(self._it)
        except StopIteration:
            return (-1, None, None, None)
        self.frame_num += 1
        f = torch.as_tensor(f)
        if not f.is_cuda:
            f = f.to(self.reader.device)
        frames, stamps, status = _ops.load_frames_4k(f[None] if f.dim() == 3 else f, self.reader)
        stamp, st = torch.stack((stamps[:1], status[:1].double())).cpu().reshape(-1).tolist()
        return (self.frame_num, frames[0], None, stamp if int(st) == _ops.TS_READ else None)


class MC_Crop_Tracker(mc3d_post.DetectionParser, mc3d_track.TrackManager):
    """See the module docstring.  sequences: loader objects; detector / cd: callables with ``.to`` and ``.eval`` (the
    full-frame detector is called as ``detector(frames, MULTI_FRAME=True)``, the crop detector as ``cd(crops,
    LOCALIZE=True)``); kf_params: INIT of ``Torch_KF``; homography: a ``Homography_Wrapper`` with every camera;
    class_dict: int -> name and name -> int."""

    write_results_csv = results_csv.write_results_csv

    def __init__(self, sequences, detector, kf_params, homography, class_dict, params={}, cd=None, PLOT=True, OUT=None,
                 early_cutoff=1000):
        if PLOT:
            raise NotImplementedError("plotting is cv2 drawing and is not part of this tracker: pass PLOT=False")
        if OUT is not None:
            raise NotImplementedError("writing output frames (OUT) needs cv2 image writers: pass OUT=None and PLOT=False")
        # parse params (MC3D_crop_tracker.py:62-87)
        defaults = dict(sigma_d=0.1, sigma_c=0.1, sigma_min=0.5, f_init=5, phi_nms_space=0.2, phi_nms_im=0.3, phi_match=0.1,
                        phi_over=0.1, W=0.5, cd_max=50, f_max=5, cs=112, b=1.25, d=1, s=1, q=1, x_range=[0, 2000])
        for k, v in defaults.items():
            setattr(self, k, params[k] if k in params else v)
        self.max_size = params["max_size"] if "max_size" in params else torch.tensor([100, 15, 15])
        self.est_ts = True
        self.ts_alpha = 0.05
        camera_centers = params["cam_centers"] if "cam_centers" in params else None
        if camera_centers is None:
            raise ValueError('params["cam_centers"] is required: {camera name: (x, y) of its centre of view in state space}')
        # the loaders (:115-127)
        self.cameras, self.sequences, self.loaders = [], [], []
        for loader in sequences:
            if isinstance(loader, str):
                raise NotImplementedError("sequences takes loader objects (see mc3d_tracker.Frames4K), not video paths: decoding "
                                          "%r is cv2" % loader)
            name = re.search(r"p\dc\d", loader.sequence).group(0)
            self.cameras.append(name)
            self.sequences.append(name + "_0_4k")
            self.loaders.append(loader)
        for hg in (getattr(homography, "hg1", homography), getattr(homography, "hg2", None)):
            corr = getattr(hg, "correspondence", None)
            if corr is not None:
                for name in self.cameras:
                    if name not in corr:
                        raise KeyError("camera %s has no correspondence in the homography" % name)
        self.centers = torch.tensor([camera_centers[key] for key in self.cameras])            # :132
        self.n_frames = len(self.loaders[0]) if self.loaders else 0
        self.ts = params["ts"] if "ts" in params else None
        self.render_params = None
        if "render" in params and params["render"] is not None:
            known = dict(out=None, label_len=5, single_box=True, fancy_crop=True, every=1)
            extra = set(params["render"]) - set(known)
            if extra:
                raise ValueError('params["render"] takes %s; got %s' % (sorted(known), sorted(extra)))
            self.render_params = dict(known, **params["render"])
            if int(self.render_params["every"]) < 1:
                raise ValueError('params["render"]["every"] is a positive frame count')
        # the device (:95-98); everything above runs without one
        device_id = params["GPU"] if "GPU" in params else torch.cuda.current_device()
        self.device = torch.device("cuda:{}".format(device_id))
        torch.cuda.set_device(device_id)
        self.state_size = kf_params["Q"].shape[0] + 1                                          # + the direction
        self.filter = Torch_KF(self.device, INIT=kf_params)
        self.hg = homography
        self.class_dict = class_dict
        self.detector = detector.to(self.device)
        self.detector.eval()
        self.crop_detector = None
        if cd is not None:
            self.crop_detector = cd.to(self.device)
            self.crop_detector.eval()
        self._centers_dev = self.centers.to(self.device).float().reshape(-1, 2).contiguous()   # what int64 - float32 promotes to
        self.output_file = "_outputs/3D_tracking_results.csv"
        self.writers = []
        self.renderer, self.rendered, self._render_inputs = None, None, None
        if self.render_params is not None and self.render_params["out"] is not None:
            import mc3d_render
            self.writers.append(mc3d_render.PngWriter(self.render_params["out"], self.cameras))
        # data storage (:157-165)
        self.next_obj_id = 0
        self.fsld = {}
        self.track_log = TrackLog(self.device, params["log_rows"] if "log_rows" in params else 4096)
        self.all_classes, self.all_confs, self.all_cameras = {}, {}, {}
        self.all_times, self.all_ts_bias = [], []
        self.time_metrics = {"load": 0, "predict": 0, "crop and align": 0, "localize": 0, "post localize": 0, "detect": 0,
                             "parse": 0, "match": 0, "update": 0, "add and remove": 0, "store": 0, "plot": 0}
        self.PLOT = PLOT
        self.cutoff_frame = early_cutoff
        self.timestamps = [0 for _ in self.loaders]
        self.ts_bias = [0 for _ in self.loaders]
        self.frame_num = 0
        self.frames = None
        self.original_ims = []
        self.updated_this_frame = []
        print("Initialized MC Crop Tracker for {} sequences".format(len(self.cameras)))

    @property
    def all_tracks(self):
        """[[id, clock time, state [7] float32 CPU tensor], ...] in the order the reference appends them (:1276-1280)."""
        return self.track_log.tracks()

    # ---- MC3D_crop_tracker.py:197-235
    def __next__(self):
        next_frames = [next(l) for l in self.loaders]
        frame_nums = [chunk[0] for chunk in next_frames]
        for item in frame_nums:                                    # catch last frame of sequence
            if item == -1:
                self.frame_num = -1
                return
        self.frames = torch.stack([chunk[1] for chunk in next_frames])
        self.original_ims = [chunk[2] for chunk in next_frames]
        self.frame_num = frame_nums[0]
        prev_ts = self.timestamps.copy()
        self.timestamps = [chunk[3] for chunk in next_frames]
        for idx in range(len(self.timestamps)):
            if self.timestamps[idx] is None:
                self.timestamps[idx] = prev_ts[idx] + 1 / 30.0

    def time_sync_cameras(self):
        if self.frame_num == -1:
            return
        latest = max(self.timestamps)
        for i in range(len(self.timestamps)):
            while latest - self.timestamps[i] >= 0.02:
                fr_num, fr, orig_im, timestamp = next(self.loaders[i])
                if fr_num == -1:                                   # the loader ran out while catching up: the run ends
                    self.frame_num = -1
                    return
                self.frames[i] = fr
                self.original_ims[i] = orig_im
                if self.ts is not None:
                    timestamp = self.ts[self.sequences[i]][fr_num]
                    if timestamp is None:
                        timestamp = self.ts[self.sequences[i]][fr_num - 1] + 1 / 30.0
                elif timestamp is None:
                    timestamp = self.timestamps[i] + 1 / 30.0
                self.timestamps[i] = timestamp

    # ---- MC3D_crop_tracker.py:1051-1312
    def _crop_frame(self):
        tm = self.time_metrics
        flt = self.filter
        self._render_inputs = None
        if self.crop_detector is None:
            raise RuntimeError("frame %d is a crop frame (d = %s, s = %s) and needs the crop detector: pass cd=... to "
                               "MC_Crop_Tracker" % (self.frame_num, self.d, self.s))
        if flt.X is None or len(flt.X) == 0:
            return
        start = time.time()
        # view 1/30 s ahead, nearest camera centre and the dt to that camera's corrected time stamp: one launch (:1150-1171)
        host = torch.tensor([[float(t) for t in self.timestamps], [float(b) for b in self.ts_bias]], dtype=torch.float64)
        state = host.to(self.device)                                                # row 0 time stamps, row 1 biases
        _, cam_idxs, dts = _ops.track_crop_prior(flt.X.float(), flt.D.float(), flt.T.double(), flt.F, self._centers_dev,
                                                 state[0], state[1])
        tm["crop and align"] += time.time() - start
        start = time.time()
        flt.predict(dt=dts)
        pre_ids, pre_loc = flt.view(with_direction=True)
        tm["predict"] += time.time() - start
        start = time.time()
        detections, classes, confs, crop_boxes = self.crop_refine(self.frames, pre_loc[:, :6], cam_idxs)    # :1172-1230
        tm["localize"] += time.time() - start
        start = time.time()
        flt.update(detections[:, :5], pre_ids)
        # classes, confs and fsld (:1240-1252) from one device -> host copy
        flat = torch.stack((confs.double(), classes.double(), cam_idxs.double())).cpu().numpy()
        confs_h, classes_h, cams_h = flat[0].astype(np.float32), flat[1].astype(np.int64), flat[2].astype(np.int64)
        for i, oid in enumerate(pre_ids):
            if confs_h[i] < self.sigma_c:
                self.fsld[oid] += 1
            else:
                self.fsld[oid] = 0
            self.all_confs[oid].append(confs_h[i].item())
            self.all_classes[oid][int(classes_h[i])] += 1
            self.all_cameras[oid].append(int(cams_h[i]))
        tm["update"] += time.time() - start
        self.crop_cameras = cams_h                                 # the last crop frame's picks, row order of pre_ids
        if self.render_params is not None:
            self._render_inputs = (detections, cam_idxs, pre_loc, crop_boxes)

    def _render_frame(self):
        """plot() (:733-917, called at :1288 with label_len = 5) on the device; see mc3d_render."""
        import mc3d_render
        rp = self.render_params
        if self.renderer is None:
            self.renderer = mc3d_render.Renderer(len(self.cameras), self.frames.shape[2], self.frames.shape[3], self.device)
        detections, cams, pre_loc, crop_boxes = self._render_inputs if self._render_inputs is not None else (None,) * 4
        self.rendered = self.renderer.render_tracker(self, detections, cams, pre_loc=pre_loc, crop_boxes=crop_boxes, crop_cams=cams,
                                                     label_len=rp["label_len"], single_box=rp["single_box"],
                                                     fancy_crop=rp["fancy_crop"])
        self.original_ims = self.renderer.views()
        if self.writers:
            host = self.rendered.cpu().numpy()                       # the second copy: only when frames are written
            self.writers[0](host, self.renderer.views(host))

    def track(self):
        tm = self.time_metrics
        self.start_time = time.time()
        next(self)                                                 # advances frame
        self.time_sync_cameras()
        self.clock_time = max(self.timestamps)
        while self.frame_num != -1:
            if self.frame_num % self.d == 0:                       # full frame detection
                start = time.time()
                with torch.no_grad():
                    scores, labels, boxes, camera_idxs = self.detector(self.frames, MULTI_FRAME=True)
                tm["detect"] += time.time() - start
                start = time.time()                                # no .cpu(): the outputs are parsed where they are
                detections, labels, scores, camera_idxs = self.parse_detections(scores, labels, boxes, camera_idxs,
                                                                                refine_height=True)
                tm["parse"] += time.time() - start
                start = time.time()
                self.associate(detections, labels, scores, camera_idxs)            # :1100-1137
                tm["update"] += time.time() - start
                if self.render_params is not None:
                    self._render_inputs = (detections, camera_idxs, None, None)
            elif self.frame_num % self.s == 0:
                self._crop_frame()
            else:
                self._render_inputs = None
            # remove overlapping objects and anomalies (:1259-1261)
            start = time.time()
            self.prune()
            tm["add and remove"] += time.time() - start
            # all object locations at the clock time (the mean time stamp) into the track log (:1266-1282)
            start = time.time()
            clock_time = sum(self.timestamps) / len(self.timestamps)
            self.all_times.append(clock_time)
            n = 0 if self.filter.X is None else len(self.filter.X)
            if n:
                dts = self.filter.get_dt(clock_time)
                post_ids, _ = self.filter.view(with_direction=True, dt=dts, out=self.track_log.slot(n))
                self.track_log.commit(post_ids, clock_time)
                for _ in range(n):
                    self.all_ts_bias.append(self.ts_bias.copy())
            tm["store"] += time.time() - start
            # the output frame (:1285-1289)
            start = time.time()
            if self.render_params is not None and self.frame_num % int(self.render_params["every"]) == 0:
                self._render_frame()
            tm["plot"] += time.time() - start
            # load next frame
            start = time.time()
            next(self)
            self.time_sync_cameras()
            tm["load"] += time.time() - start
            elapsed = time.time() - self.start_time
            fps = self.frame_num / max(elapsed, 1e-9)
            fps_noload = self.frame_num / max(elapsed - tm["load"] - tm["plot"], 1e-9)
            print("\rTracking frame {} of {} at {:.1f} FPS ({:.1f} FPS without loading and plotting)".format(
                self.frame_num, self.n_frames, fps, fps_noload), end="\r", flush=True)
            if self.frame_num > self.cutoff_frame:
                for item in tm.items():
                    print(item)
                break
        self.end_time = time.time()

"""Drop-in for the association step of the reference's multi-camera tracker (``MC3D_crop_tracker.py``):
``match_hungarian`` (:637-731), ``manage_tracks`` (:385-461), ``increment_fslds`` (:463-479), ``remove_overlaps``
(:482-518) and ``remove_anomalies`` (:520-557), plus ``associate``, the detection-frame block of ``track``
(:1100-1137) in one call, ``prune``, the pruning at the end of every frame (:1259-1261), and ``estimate_ts_bias``
(:237-315), which parse_detections calls between the transforms and the space NMS when ``est_ts`` is set (the
reference's default).

The functions take ``self`` exactly like the methods they replace and read the same attributes (``filter`` = a
``Torch_KF``, ``timestamps``, ``ts_bias``, ``ts_alpha``, ``phi_nms_space``, ``phi_match``, ``phi_over``, ``f_max``, ``max_size``, ``x_range``,
``class_dict``, ``fsld``, ``all_classes``, ``all_confs``, ``all_cameras``, ``next_obj_id``, ``updated_this_frame``),
so a maintainer binds them into the reference class unchanged::

    import mc3d_track
    MC_Crop_Tracker.match_hungarian = mc3d_track.match_hungarian
    MC_Crop_Tracker.manage_tracks = mc3d_track.manage_tracks
    MC_Crop_Tracker.increment_fslds = mc3d_track.increment_fslds
    MC_Crop_Tracker.remove_overlaps = mc3d_track.remove_overlaps
    MC_Crop_Tracker.remove_anomalies = mc3d_track.remove_anomalies
    MC_Crop_Tracker.estimate_ts_bias = mc3d_track.estimate_ts_bias

or inherits ``TrackManager``.  With the filter on the GPU (``util_track/kf.py``) and the detections from
``mc3d_post.parse_detections`` left on the device, the cost matrix, the assignment and the gate run in
libretinanet_mi355x.so (``rn_track_cost``, ``rn_linear_sum_assignment``); the host sees one copy per frame of the
matchings with the labels, scores and cameras of the detections (the bookkeeping dictionaries are host Python), and
the ids of the tracks that pruning removes; ``estimate_ts_bias`` (``rn_estimate_ts_bias``) costs one more small copy,
the biases with the pair count.

Reference behaviour kept on purpose:
  * ``associate`` calls ``increment_fslds(pre_ids, undetected)`` with the arguments swapped against the signature
    ``(undetected, pre_ids)``, as the reference's call site does (:1137): every prior, matched or not, gets +1 (a matched
    track ends the frame at fsld 1) and only the truly undetected ids are tested for removal.
  * Predicting the matched rows to their detection times (``get_dt(match_times, idxs=...)``) also rolls every
    unmatched row forward by ``dt_default``.
  * ``remove_overlaps`` scores every track with ``len(all_classes[id])``, which is always 8: every score ties, and
    under this repository's NMS convention ties go to the lower index, so the oldest row survives (torchvision's tie
    order is not pinned).
Difference: ``all_confs`` / ``all_cameras`` receive Python numbers where the reference appends 0-d tensors (both lists
are write-only in the reference).
"""
import time

import numpy as np
import torch

from retinanet_mi355x import ops as _ops


def _host(x):
    """Host numpy view of a tensor / array / list (one copy for a device tensor)."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _on_device(*xs):
    return any(isinstance(x, torch.Tensor) and x.is_cuda for x in xs)


def _device(self, *xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device(getattr(getattr(self, "filter", None), "device", "cuda:0"))


def match_hungarian(self, first, second):
    """-> [l,2] pairs [prior row, detection row] in row order: an ``np.ndarray`` for CPU inputs (``[]`` when the
    assignment is invalid, as the reference's ``except ValueError``), an int64 device tensor for device inputs."""
    if len(first) == 0 or len(second) == 0:
        return []
    dev = _device(self, first, second)
    cost = _ops.track_cost(first.to(dev), second.to(dev))
    row_match, info = _ops.match(cost, 1 - self.phi_match, info=True)      # the gate is fp64, as in Python (:721)
    if not _on_device(first, second):
        k, status = (int(x) for x in info.cpu())
        if status != _ops.LSAP_OK:
            return []
        rm = row_match.cpu().numpy()
        return np.array([[i, int(rm[i])] for i in range(len(rm)) if rm[i] != -1])
    k = int(info[0])                                                       # the one device -> host word
    rows = _ops._matched_rows(row_match, k)
    return torch.stack((rows, row_match[rows].long()), dim=1)


def manage_tracks(self, detections, matchings, pre_ids, labels, scores, cameras, detection_times, mean_object_sizes=True):
    """MC3D_crop_tracker.py:385-461.  ``detections`` may stay on the device (the filter reads it there); matchings,
    labels, scores and cameras are read on the host (one copy each if they are device tensors; ``associate`` hands
    them over already copied)."""
    m = _host(matchings).reshape(-1, 2).astype(np.int64) if len(matchings) else np.zeros((0, 2), np.int64)
    lab, sc, cam = _host(labels), _host(scores), _host(cameras)
    dev_det = detections if isinstance(detections, torch.Tensor) else torch.as_tensor(np.asarray(detections))
    # 1. update tracked and matched objects
    update_ids = []
    for a, b in m:
        update_ids.append(pre_ids[a])
        self.fsld[pre_ids[a]] = 0
        self.updated_this_frame.append(pre_ids[a])
    if len(m) > 0:
        idx = torch.as_tensor(m[:, 1], dtype=torch.long, device=dev_det.device)
        self.filter.update(dev_det[idx, :5].double(), update_ids)
        for i, (a, b) in enumerate(m):
            self.all_classes[update_ids[i]][int(lab[b])] += 1
            self.all_confs[update_ids[i]].append(sc[b].item())
            self.all_cameras[update_ids[i]].append(cam[b].item())
    # 2. every detection not in matchings starts a new object
    matched = set(int(b) for b in m[:, 1])
    new_rows, new_ids, new_classes, new_times = [], [], [], []
    for i in range(len(dev_det)):
        if i in matched:
            continue
        new_rows.append(i)
        new_ids.append(self.next_obj_id)
        new_times.append(detection_times[i])
        self.fsld[self.next_obj_id] = 0
        self.all_classes[self.next_obj_id] = np.zeros(8)
        self.all_confs[self.next_obj_id] = []
        self.all_cameras[self.next_obj_id] = []
        self.updated_this_frame.append(self.next_obj_id)
        cls = int(lab[i])
        self.all_classes[self.next_obj_id][cls] += 1
        self.all_confs[self.next_obj_id].append(sc[i].item())
        self.all_cameras[self.next_obj_id].append(cam[i].item())
        new_classes.append(self.class_dict[cls])
        self.next_obj_id += 1
    if new_rows:
        idx = torch.as_tensor(new_rows, dtype=torch.long, device=dev_det.device)
        new = dev_det[idx]
        kw = dict(init_speed=True, classes=new_classes) if mean_object_sizes else dict(init_speed=True)
        self.filter.add(new[:, :5], new_ids, new[:, 5].double(), np.array(new_times, dtype=np.float64), **kw)


def increment_fslds(self, undetected, pre_ids):
    """MC3D_crop_tracker.py:463-479: +1 for every id of ``undetected``, then remove the ids of ``pre_ids`` that reached
    f_max.  (``associate`` passes the arguments swapped, as the reference's call site does.)"""
    start = time.time()
    for i in undetected:
        self.fsld[i] += 1
    removals = []
    for i in pre_ids:
        if self.fsld[i] >= self.f_max:
            removals.append(i)
            self.fsld.pop(i, None)
    if len(removals) > 0:
        self.filter.remove(removals)
    tm = getattr(self, "time_metrics", None)
    if tm is not None and "add and remove" in tm:
        tm["add and remove"] += time.time() - start
    return removals


def _view_now(self):
    dts = self.filter.get_dt(max(self.timestamps))
    return self.filter.view(with_direction=True, dt=dts)


def remove_overlaps(self):
    """MC3D_crop_tracker.py:482-518 on the device: footprints of the tracks viewed at the latest timestamp, NMS at
    phi_over scored by ``len(all_classes[id])`` (always 8: ties, the lower row -- the oldest track -- survives).
    -> the removed ids (sorted)."""
    if not self.phi_over > 0:
        return []
    ids, boxes = _view_now(self)
    if len(ids) == 0:
        return []
    sp = _ops.hg_state_to_space(boxes)
    fp = torch.stack((sp[:, 0:4, 0].min(1).values, sp[:, 0:4, 1].min(1).values,
                      sp[:, 0:4, 0].max(1).values, sp[:, 0:4, 1].max(1).values), dim=1)
    scores = torch.tensor([len(self.all_classes[i]) for i in ids], dtype=torch.float32).to(fp.device)
    keep = _ops.nms(fp, scores, self.phi_over)
    gone = torch.ones(len(ids), dtype=torch.bool, device=fp.device)
    gone[keep] = False
    rows = gone.nonzero().squeeze(1).cpu().tolist()                      # only the removals reach the host
    removals = sorted(set(ids[r] for r in rows))
    if len(removals) > 0:
        self.filter.remove(removals)
    return removals


def remove_anomalies(self, x_bounds=[300, 600]):
    """MC3D_crop_tracker.py:520-557 on the device: the reference's predicate on (y, l, w, h, v, x) of the tracks viewed
    at the latest timestamp, strict comparisons.  -> the removed ids (sorted)."""
    max_sizes = self.max_size
    ids, b = _view_now(self)
    if len(ids) == 0:
        return []
    bad = (b[:, 1] > 120) | (b[:, 1] < -10)
    bad |= (b[:, 2] > max_sizes[0]) | (b[:, 2] < 0) | (b[:, 3] > max_sizes[1]) | (b[:, 3] < 0)
    bad |= (b[:, 4] > max_sizes[2]) | (b[:, 4] < 0)
    bad |= (b[:, 6] > 150) | (b[:, 6] < -150)
    bad |= (b[:, 0] < x_bounds[0]) | (b[:, 0] > x_bounds[1])
    rows = bad.nonzero().squeeze(1).cpu().tolist()                       # only the removals reach the host
    removals = sorted(set(ids[r] for r in rows))
    if len(removals) > 0:
        self.filter.remove(removals)
    return removals


def associate(self, detections, labels, scores, camera_idxs):
    """The detection-frame block of MC_Crop_Tracker.track (MC3D_crop_tracker.py:1100-1137) after parse_detections:
    view the filter at the mean timestamp, match, predict the matched rows to their detection times, manage_tracks,
    increment_fslds.  -> (pre_ids, matchings); matchings as match_hungarian returns them."""
    self.updated_this_frame = []
    avg_time = sum(self.timestamps) / len(self.timestamps)
    dts = self.filter.get_dt(avg_time)
    pre_ids, pre_loc = self.filter.view(with_direction=True, dt=dts)
    if isinstance(detections, torch.Tensor) and detections.is_cuda and len(pre_ids) > 0 and len(detections) > 0:
        # match_hungarian without its own synchronisation: one device -> host copy carries the (count, status) word,
        # the row matches and the labels / scores / cameras of the detections
        dev = detections.device
        cost = _ops.track_cost(pre_loc, detections)
        row_match, info = _ops.match(cost, 1 - self.phi_match, info=True)
        n, d = len(pre_ids), len(detections)
        flat = torch.cat([info.double(), row_match.double(), labels.to(dev).double().reshape(-1),
                          scores.to(dev).double().reshape(-1), camera_idxs.to(dev).double().reshape(-1)]).cpu().numpy()
        rm = flat[2:2 + n].astype(np.int64)
        lab = flat[2 + n:2 + n + d].astype(np.int64)
        sc = flat[2 + n + d:2 + n + 2 * d].astype(np.float32)
        cam = flat[2 + n + 2 * d:2 + n + 3 * d].astype(np.int64)
        rows = np.nonzero(rm >= 0)[0]
        m = np.stack((rows, rm[rows]), axis=1).astype(np.int64)
        matchings = torch.from_numpy(m).to(dev) if len(m) else torch.zeros((0, 2), dtype=torch.int64, device=dev)
    else:
        matchings = self.match_hungarian(pre_loc, detections)
        m = _host(matchings).reshape(-1, 2).astype(np.int64) if len(matchings) else np.zeros((0, 2), np.int64)
        lab, sc, cam = _host(labels), _host(scores), _host(camera_idxs)
    if len(m) > 0:
        filter_idxs = [int(a) for a in m[:, 0]]
        match_times = [self.timestamps[cam[b]] + self.ts_bias[cam[b]] for b in m[:, 1]]
        self.filter.predict(dt=self.filter.get_dt(match_times, idxs=filter_idxs))
    detection_times = [self.timestamps[c] + self.ts_bias[c] for c in cam]
    self.manage_tracks(detections, m, pre_ids, lab, sc, cam, detection_times)
    updated = set(self.updated_this_frame)
    undetected = [i for i in pre_ids if i not in updated]
    self.increment_fslds(pre_ids, undetected)                           # swapped, as at MC3D_crop_tracker.py:1137
    return pre_ids, matchings


def estimate_ts_bias(self, boxes, camera_idxs):
    """MC3D_crop_tracker.py:237-315 on the device: ``boxes`` [d,6] states and ``camera_idxs`` [d] as parse_detections
    holds them before the space NMS.  Reads ``filter``, ``timestamps``, ``ts_bias``, ``phi_nms_space``, ``ts_alpha``;
    the footprints and md_iou are the kernel's own (``hg`` / ``md_iou`` of the host class are not called).  Uploads the
    time stamps and biases (a few doubles), runs ``rn_estimate_ts_bias`` and replaces ``self.ts_bias`` by a list of
    Python floats from one device -> host copy (biases and the (pairs, status) word together).  When the pair buffer
    was too small the call is repeated once with a buffer sized from the count.  Returns None, as the reference."""
    if len(camera_idxs) == 0:
        return
    _, objs = self.filter.view(with_direction=True)
    if len(objs) == 0:
        return
    dev = _device(self, boxes, camera_idxs, objs)
    if not isinstance(boxes, torch.Tensor):
        boxes = torch.as_tensor(np.asarray(boxes, dtype=np.float32))
    if not isinstance(camera_idxs, torch.Tensor):
        camera_idxs = torch.as_tensor(np.asarray(camera_idxs, dtype=np.int64))
    n_cam = len(self.ts_bias)
    host = torch.tensor([[float(t) for t in self.timestamps], [float(b) for b in self.ts_bias]], dtype=torch.float64)
    if host.shape[1] != n_cam:
        raise RuntimeError("estimate_ts_bias: %d timestamps for %d biases" % (len(self.timestamps), n_cam))
    state = host.to(dev)                                                  # row 0 time stamps, row 1 biases
    boxes, camera_idxs, objs = boxes.to(dev), camera_idxs.to(dev), objs.to(dev)
    mu_v = float(self.filter.mu_v)
    max_pairs = None
    for attempt in range(2):
        info = _ops.estimate_ts_bias(boxes, camera_idxs, objs, state[0], state[1], self.phi_nms_space, self.ts_alpha, mu_v,
                                     max_pairs=max_pairs)
        flat = torch.cat((state[1], info.double())).cpu().tolist()        # the one device -> host copy
        count, status = int(flat[n_cam]), int(flat[n_cam + 1])
        if status != _ops.TS_OVERFLOW:
            break
        max_pairs = count                                                 # ts_bias was left untouched: run again
    if status == _ops.TS_BAD_CAMERA:
        raise IndexError("estimate_ts_bias: a camera index is outside the %d cameras of ts_bias" % n_cam)
    if status != _ops.TS_OK:
        raise RuntimeError("estimate_ts_bias: %d pairs did not fit the pair buffer" % count)
    if count > 0:                                                         # no pair: the reference writes nothing
        self.ts_bias = [float(b) for b in flat[:n_cam]]


def prune(self):
    """remove_overlaps, then remove_anomalies(x_bounds=self.x_range) (MC3D_crop_tracker.py:1259-1261).
    -> (overlap removals, anomaly removals)."""
    return self.remove_overlaps(), self.remove_anomalies(x_bounds=self.x_range)


class TrackManager:
    """Mixin carrying the methods; the host class provides the attributes listed in the module docstring."""
    match_hungarian = match_hungarian
    manage_tracks = manage_tracks
    increment_fslds = increment_fslds
    remove_overlaps = remove_overlaps
    remove_anomalies = remove_anomalies
    associate = associate
    estimate_ts_bias = estimate_ts_bias
    prune = prune

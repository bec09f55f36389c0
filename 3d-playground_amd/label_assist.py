"""The detector-assisted labelling path of the reference's annotator (``manual_annotator_state_v3.py``, class ``Annotator``;
``seems_to_be_working.py`` holds the same code at other line numbers), on the GPU: ``box_to_state`` (:521-543), ``find_box``
(:1005-1028), ``copy_paste`` (:798-848), ``paste_in_2D_bbox`` (:588-642), ``crop_detect`` (:699-741) and ``automate``
(:644-697), plus the batch form the reference lacks, ``automate_many``.  This is the path that MAKES the labels which
``label_audit``, ``label_rewrite``, ``label_trajectory`` and ``label_quality`` take as input.

The functions take ``self`` like the methods they replace and read ``data``, ``cameras``, ``seq_keys``, ``all_ts``, ``hg`` (a
``Homography_Wrapper``), ``frame_idx``, ``active_cam``, ``clicked_camera``, ``copied_box``, ``AUTO``, ``detector`` and, in
``automate``, ``buffer`` / ``buffer_frame_idx``; bind them like ``label_rewrite``'s::

    import label_assist
    for name in label_assist.METHODS:
        setattr(Annotator, name, getattr(label_assist, name))

or inherit ``LabelAssist``.

``paste_in_2D_bbox`` is the slow one in the reference: three rounds of an 11 x 11 grid search over the box centre (radii 50, 10,
2 ft), every round a ``torch.stack`` of 121 boxes through ``state_to_im``, the winner the centre whose 2D extent lies nearest
the detected box.  Here ``ops.label_fit_box2d`` searches every box with one wave (csrc/label_assist.hip), ``ops.label_crop_windows``
makes the crop windows and ``ops.label_best_anchor`` picks the localiser's best anchor; ``to_tensor`` is ``ops.frame_ingest``
with mean 0 and std 1 and ``roi_align`` is ``ops.roi_align``.  There is no CPU path: without a device every function raises
before it changes anything.

What differs from the reference: ``automate`` does not draw; it returns ``{"crop_box", "box_2D", "skipped"}``,
the two rectangles the reference draws (``None`` where the reference returns before it has them).  ``crop_detect`` takes the
frame as a uint8 ``[H,W,3]`` device tensor or numpy array in the reference's channel order and returns the box on the host, as
the reference does.  ``box_to_state`` returns a float32 ``[2,2]`` host tensor.  A status bit of a kernel raises RuntimeError
before ``data`` is touched.  ``automate_many`` treats every key's camera as the active view (no 1920 shift): the returned
rectangles are in the key's own camera's pixels.
"""
import copy

import numpy as np
import torch

from datareader import _download, _upload
from label_audit import _device, _names
from retinanet_mi355x import ops

METHODS = ("box_to_state", "find_box", "copy_paste", "paste_in_2D_bbox", "crop_detect", "automate", "automate_many")
SEARCH_RAD, GRID_SIZE = 50, 11                                 # :603-604
VIEW_WIDTH, FRAME_W, FRAME_H = 1920, 1920, 1080                # :530, :672
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # :722-723
STATE_KEYS = ("x", "y", "l", "w", "h", "direction")
F32 = np.float32


def _tables(hg, names, key, used=None):
    """fp64 [C, 9 | 12] of ``key`` ("H" or "P") for both sides of the wrapper (the second ``None`` for a single Homography):
    the matrix of every camera in ``used`` (all by default; KeyError if the homography lacks one), zeros for the others."""
    out = []
    for side in (getattr(hg, "hg1", hg), getattr(hg, "hg2", None)):
        if side is None:
            out.append(None)
            continue
        table = np.zeros((len(names), 9 if key == "H" else 12), np.float64)
        for c, n in enumerate(names):
            if used is None or n in used:
                table[c] = np.asarray(side.correspondence[n][key], np.float64).reshape(-1)
        out.append(table)
    return out


def _view_camera(self, x0):
    """:530-535, :1009-1013: a point right of 1920 lies in the view's second camera."""
    return (self.seq_keys[self.active_cam + 1], True) if x0 > VIEW_WIDTH else (self.seq_keys[self.active_cam], False)


def _mats(tensor, width):
    return None if tensor is None else tensor.reshape(-1, 3, width)


def _points_to_xy(points, cam, H1, H2):
    """``hg.im_to_state(point repeated over the 8 corners, heights = 0)[:, :2]`` on the device: points fp64 [k,2], cam int32 [k]
    or None (matrix 0) -> fp32 [k,2]."""
    k = points.shape[0]
    im = points.reshape(k, 1, 2).expand(k, 8, 2)
    state = ops.hg_from_im(im, torch.zeros(k, dtype=torch.float32, device=points.device), _mats(H1, 3), _mats(H2, 3), cam)
    return state[:, :2]


def _centres(boxes, cam, H1, H2):
    """:598: ``box_to_state(box).mean(dim = 0)`` of every box: boxes fp64 [n,4] -> fp32 [n,2]."""
    n = boxes.shape[0]
    xy = _points_to_xy(boxes.reshape(n * 2, 2), None if cam is None else cam.repeat_interleave(2), H1, H2).reshape(n, 2, 2)
    return ((xy[:, 0] + xy[:, 1]) / 2).contiguous()


def box_to_state(self, point, direction=False):
    """:521-543.  point: 4 values (start x / y, end x / y) in view pixels -> float32 [2,2] host tensor, start and end on the road."""
    point = point.copy()
    cam, shifted = _view_camera(self, point[0])
    if shifted:
        point[0] -= VIEW_WIDTH
        point[2] -= VIEW_WIDTH
    H1, H2 = _tables(self.hg, [cam], "H")
    up = _upload(_device(self), [np.array([[point[0], point[1]], [point[2], point[3]]], np.float64)] + [H1] + ([] if H2 is None else [H2]))
    xy, = _download([_points_to_xy(up[0], None, up[1], up[2] if H2 is not None else None)])
    return torch.from_numpy(xy.copy())


def find_box(self, point):
    """:1005-1028: the id of the frame's box nearest to the clicked point on the road; the first smallest in the dict's order."""
    point = point.copy()
    cam, shifted = _view_camera(self, point[0])
    if shifted:
        point[0] -= VIEW_WIDTH
    H1, H2 = _tables(self.hg, [cam], "H")
    up = _upload(_device(self), [np.array([[point[0], point[1]]], np.float64)] + [H1] + ([] if H2 is None else [H2]))
    xy, = _download([_points_to_xy(up[0], None, up[1], up[2] if H2 is not None else None)])
    sx, sy = xy[0]
    min_dist, min_id = np.inf, None
    with np.errstate(all="ignore"):
        for box in self.data[self.frame_idx].values():
            dx, dy = F32(box["x"]) - sx, F32(box["y"]) - sy     # float32: a Python float beside a float32 tensor
            dist = dx * dx + dy * dy
            if dist < min_dist:
                min_dist = dist
                min_id = box["id"]
    return min_id


def copy_paste(self, point):
    """:798-848: the first click copies the nearest box, the next pastes it where the click lands (and automates it once when
    ``AUTO`` is set)."""
    if self.copied_box is None:
        obj_idx = find_box(self, point)
        if obj_idx is None:
            return
        state_point = box_to_state(self, point)[0].numpy()
        key = "{}_{}".format(self.clicked_camera, obj_idx)
        obj = self.data[self.frame_idx].get(key)
        if obj is None:
            return
        self.copied_box = (obj_idx, obj.copy(), [state_point[0], state_point[1]])
    else:
        state_point = box_to_state(self, point)[0].numpy()
        obj_idx = self.copied_box[0]
        new_obj = copy.deepcopy(self.copied_box[1])
        dx = state_point[0] - self.copied_box[2][0]
        dy = state_point[1] - self.copied_box[2][1]
        new_obj["x"] = (F32(new_obj["x"]) + dx).item()          # :829-832: float32, as a Python float plus a float32 tensor
        new_obj["y"] = (F32(new_obj["y"]) + dy).item()
        new_obj["timestamp"] = self.all_ts[self.frame_idx][self.clicked_camera]
        new_obj["camera"] = self.clicked_camera
        new_obj["gen"] = "Manual"
        self.data[self.frame_idx]["{}_{}".format(self.clicked_camera, obj_idx)] = new_obj
        if getattr(self, "AUTO", False):
            self.automate(obj_idx) if hasattr(self, "automate") else automate(self, obj_idx)
            self.AUTO = False


def _template(obj):
    return [float(obj[k]) for k in STATE_KEYS[2:]]


def paste_in_2D_bbox(self, box, grid_size=GRID_SIZE):
    """:588-642.  Slides the copied box until its image footprint fits the 2D ``box`` (4 values in view pixels; shifted in
    place by 1920 when it lies in the second view, as the reference does) and writes it under "{clicked_camera}_{id}"."""
    if self.copied_box is None:
        return
    base = self.copied_box[1].copy()
    point = box.copy()
    cam, shifted = _view_camera(self, point[0])
    if shifted:
        point[[0, 2]] -= VIEW_WIDTH
    target = box.copy()
    if target[0] > VIEW_WIDTH:                                  # :600-601
        target[[0, 2]] -= VIEW_WIDTH
    H1, H2 = _tables(self.hg, [cam], "H")
    P1, P2 = _tables(self.hg, [self.clicked_camera], "P")
    stamp = self.all_ts[self.frame_idx][self.clicked_camera]
    radii = np.array(ops.label_rebase_radii(SEARCH_RAD), np.float64)
    parts = [np.asarray(point, np.float64).reshape(1, 4), np.asarray(target).astype(F32).reshape(1, 4),
             np.array([_template(base)], F32), np.zeros(1, np.int32), radii, H1, P1] + ([] if H2 is None else [H2, P2])
    up = _upload(_device(self), parts)                          # every refusal above comes before any GPU work
    box[...] = target                                           # the reference shifts the caller's array in place
    dH2, dP2 = (up[7], up[8]) if H2 is not None else (None, None)
    centre = _centres(up[0], None, up[5], dH2)
    out, _, _, status = ops.label_fit_box2d(up[2], up[3], centre, up[1], _mats(up[6], 4), _mats(dP2, 4), up[4], grid_size)
    h_status, h_out = _download([status, out])
    ops.label_check(int(h_status[0]))
    base["x"] = h_out[0, 0].item()                              # :636-637: self.safe(center[0])
    base["y"] = h_out[0, 1].item()
    base["camera"] = self.clicked_camera
    base["gen"] = "Manual"
    base["timestamp"] = stamp
    self.data[self.frame_idx]["{}_{}".format(self.clicked_camera, base["id"])] = base


def _frames_on(dev, frames):
    t = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError("a frame is uint8 [H,W,3], got %s %s" % (t.dtype, tuple(t.shape)))
    return t if t.is_cuda else t.to(dev)


def _localise(self, frames_u8, rois, win, cs):
    """:720-740 for every RoI: frames uint8 [B,H,W,3] on the device, rois fp32 [n,5], win fp32 [n,3] -> what
    ``ops.label_best_anchor`` returns."""
    dev = frames_u8.device
    im = ops.frame_ingest(frames_u8, swap_rb=False, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))      # F.to_tensor
    crops = ops.roi_align(im, rois, (cs, cs))
    mean = torch.tensor(MEAN, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    crops.sub_(mean).div_(std)                                  # F.normalize
    det = self.detector
    det.eval()
    det.training = False                                        # :727-728
    with torch.no_grad():
        reg_boxes, classes = det(crops, LOCALIZE=True)
    return ops.label_best_anchor(reg=reg_boxes.float().contiguous(), cls=classes.float().contiguous(), win=win, cs=cs)


def crop_detect(self, frame, crop, ber=1.2, cs=112):
    """:699-741.  The best 2D box of the localiser inside the square window about ``crop`` (x1, y1, x2, y2 in frame pixels),
    in frame coordinates -> float32 [4] host tensor."""
    c = np.asarray(crop.detach().cpu() if torch.is_tensor(crop) else crop).astype(F32)
    w, h = c[2] - c[0], c[3] - c[1]
    scale = (h if h > w else w) * F32(ber)                      # Python's max(w, h) of two float32 tensors
    half = scale / F32(2.0)
    mx, my = (c[2] + c[0]) / F32(2.0), (c[3] + c[1]) / F32(2.0)
    minx, miny = mx - half, my - half
    dev = _device(self)
    frames = _frames_on(dev, frame)
    rois, win = _upload(dev, [np.array([[0.0, minx, miny, mx + half, my + half]], F32), np.array([[minx, miny, scale]], F32)])
    box, _, _, _ = _localise(self, frames, rois, win, cs)
    got, = _download([box])
    return torch.from_numpy(got[0].copy())


def _camera_index(self, cam):
    """:658-660: the reference's loop leaves the last index when no camera matches."""
    names = _names(self)
    return names.index(cam) if cam in names else len(names) - 1


def automate(self, obj_idx, ber=1.2, cs=112):
    """:644-697 without the drawing: crops around the clicked camera's box ``obj_idx``, localises it (``ber`` and ``cs`` are
    crop_detect's, at the reference's defaults), fits the copied template to the detected 2D box -> {"crop_box", "box_2D",
    "skipped"} in view pixels (float32 arrays), or None without the box."""
    cam = self.clicked_camera
    prev_box = self.data[self.frame_idx].get("{}_{}".format(cam, obj_idx))
    if prev_box is None:
        return None
    c_idx = _camera_index(self, cam)
    P1, P2 = _tables(self.hg, [cam], "P")
    state = np.array([[prev_box[k] for k in STATE_KEYS]], F32)  # :662: torch.tensor of Python floats is float32
    up = _upload(_device(self), [state, np.zeros(1, np.int32), P1] + ([] if P2 is None else [P2]))
    crop, _, _, skipped, status = ops.label_crop_windows(up[0], up[1], _mats(up[2], 4), _mats(up[3], 4) if P2 is not None else None,
                                                         ber, FRAME_W, FRAME_H)
    h_status, h_crop, h_skipped = _download([status, crop, skipped])
    ops.label_check(int(h_status[0]))
    crop_box = h_crop[0].copy()
    if h_skipped[0]:                                            # :672: near the edge, the reference returns silently
        return {"crop_box": crop_box, "box_2D": None, "skipped": True}
    frame = self.buffer[self.buffer_frame_idx][c_idx][0]
    box_2D = (self.crop_detect if hasattr(self, "crop_detect") else crop_detect.__get__(self))(frame, crop_box, ber, cs)
    box_2D = np.array(box_2D.detach().cpu() if torch.is_tensor(box_2D) else box_2D, F32)
    if self.active_cam != c_idx:                                # :683-685
        crop_box[[0, 2]] += VIEW_WIDTH
        box_2D[[0, 2]] += VIEW_WIDTH
    paste_in_2D_bbox(self, box_2D.copy())
    return {"crop_box": crop_box, "box_2D": box_2D, "skipped": False}


def automate_many(self, keys, frames, ber=1.2, cs=112, grid_size=GRID_SIZE):
    """``copy_paste`` + ``automate`` of every key of ``data[frame_idx]`` in one pass: keys "{camera}_{id}", frames {camera:
    uint8 [H,W,3]} or a uint8 [C,H,W,3] tensor in ``seq_keys`` order.  Every key's own box is its template and its camera the
    active view.  One upload, one launch each of the crop windows, roi_align, the detector, the best anchor and the fit, one
    copy back -> {key: {"crop_box", "box_2D", "skipped"}}; the data of the keys that were not skipped are rewritten."""
    keys = list(keys)
    frame_data = self.data[self.frame_idx]
    if isinstance(frames, dict):
        order = [n for n in self.seq_keys if n in frames]
    else:
        order = list(self.seq_keys)
        if len(frames) != len(order):
            raise ValueError("frames holds %d cameras, seq_keys %d" % (len(frames), len(order)))
    boxes = []
    for key in keys:
        obj = frame_data[key]                                   # KeyError: the key is not in this frame
        cam = key.rpartition("_")[0]
        if cam not in order:
            raise KeyError("no frame of camera {} for key {!r}".format(cam, key))
        boxes.append((key, obj, cam, self.all_ts[self.frame_idx][cam]))
    if not boxes:
        return {}
    state = np.array([[o[k] for k in STATE_KEYS] for _, o, _, _ in boxes], F32).reshape(-1, 6)
    cam_idx = np.array([order.index(c) for _, _, c, _ in boxes], np.int32)
    used = {c for _, _, c, _ in boxes}
    H1, H2 = _tables(self.hg, order, "H", used)
    P1, P2 = _tables(self.hg, order, "P", used)
    radii = np.array(ops.label_rebase_radii(SEARCH_RAD), np.float64)
    dev = _device(self)                                         # every refusal above comes before any GPU work
    parts = [state, cam_idx, radii, H1, P1] + ([] if H2 is None else [H2, P2])
    host_frames = isinstance(frames, dict) and not any(torch.is_tensor(frames[n]) for n in order)
    if host_frames:
        parts.append(np.stack([np.ascontiguousarray(frames[n]) for n in order]))
    up = _upload(dev, parts)
    dH2, dP2 = (up[5], up[6]) if H2 is not None else (None, None)
    if host_frames:
        frames_u8 = _frames_on(dev, up[-1])
    elif isinstance(frames, dict):
        frames_u8 = torch.stack([_frames_on(dev, frames[n]) for n in order])
    else:
        frames_u8 = _frames_on(dev, frames)
    d_state, d_cam = up[0], up[1]
    status = ops.label_status(dev)
    crop, rois, win, skipped, _ = ops.label_crop_windows(d_state, d_cam, _mats(up[4], 4), _mats(dP2, 4), ber, FRAME_W, FRAME_H,
                                                         status=status)
    box, _, _, _ = _localise(self, frames_u8, rois, win, cs)
    centre = _centres(box.double(), d_cam, up[3], dH2)
    out, _, _, _ = ops.label_fit_box2d(d_state[:, 2:].contiguous(), d_cam, centre, box, _mats(up[4], 4), _mats(dP2, 4), up[2],
                                       grid_size, skip=skipped, status=status)
    h_status, h_crop, h_box, h_skipped, h_out = _download([status, crop, box, skipped, out])
    ops.label_check(int(h_status[0]))
    result = {}
    for i, (key, obj, cam, stamp) in enumerate(boxes):
        if h_skipped[i]:
            result[key] = {"crop_box": h_crop[i].copy(), "box_2D": None, "skipped": True}
            continue
        base = obj.copy()
        base["x"] = h_out[i, 0].item()
        base["y"] = h_out[i, 1].item()
        base["camera"] = cam
        base["gen"] = "Manual"
        base["timestamp"] = stamp
        frame_data["{}_{}".format(cam, base["id"])] = base
        result[key] = {"crop_box": h_crop[i].copy(), "box_2D": h_box[i].copy(), "skipped": False}
    return result


class LabelAssist():
    """The functions above as methods: inherit it beside (or assign its members into) the reference's ``Annotator``."""
    box_to_state = box_to_state
    find_box = find_box
    copy_paste = copy_paste
    paste_in_2D_bbox = paste_in_2D_bbox
    crop_detect = crop_detect
    automate = automate
    automate_many = automate_many

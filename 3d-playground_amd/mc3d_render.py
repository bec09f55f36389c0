"""The tracker's output frames on the GPU: ``MC_Crop_Tracker.plot`` (MC3D_crop_tracker.py:733-917) and ``Homography.
plot_boxes`` / ``Homography_Wrapper.plot_state_boxes`` (homography.py:670-714, 864-905) without cv2.

Per camera the frame with every track's 3D box and the detections drawn in, the label block (class, id, speed, size), the crop
windows lit against a dimmed frame and the time-bias banner; all cameras tiled into one image.  Everything is painted as bits
of a mask plane by ``ops.render_edges`` / ``render_rects`` / ``render_text`` and turned into pixels by ONE pass over the frames
the detector already has (``ops.render_compose``, csrc/render.hip).  Layer order, colours, blend weights, label contents and
geometry are the reference's; the rasteriser and the font are this project's own (OpenCV's are not available), in exact
integer arithmetic, restated in tests/render_cases.py.

Differences from the reference:
  * Lines: a pixel is covered when it lies within thickness / 2 of the segment (include/retinanet_mi355x.h); text is a 6x8
    cell font (``FONT``) at integer scales, 1 for the labels (the reference: Hershey plain 0.8) and 2 for the banner (1.6).
  * The label blend (0.7 / 0.3) applies only under label pixels and a pixel inside a crop window keeps its value (the
    reference blends every pixel with itself there: 0.3 v + 0.7 v), so an empty mask gives the frame back exactly.
  * Crop windows are clipped at the frame (numpy's slices wrap negative corners).
  * ``plot_state_boxes`` leaves out a box whose y is exactly 60 (neither ``> 60`` nor ``< 60``); here it is drawn through the
    wrapper's own switch (``y > 60`` -> second homography).
  * The mosaic puts camera i at ``(i // cols, i % cols)``; see ``mosaic_layout``.
  * uint8 RGB output (the reference: float64 BGR, scaled by 255 in its writer).
  * ``Replayer`` (Data_Reader.plot_in, datareader.py:253-399) shares the line and font rules above.  Its label goes over the
    whole rectangle as 0.7 v + 0.3 * 255 and text wins everywhere; the reference draws every label's text into both of its
    copies but lets a LATER label's rectangle grey an earlier label's text in one of them (:281-288).  Its canvas keeps the
    reference's column-major tiles (``replay_layout``), resampled to the output size by this project's own integer bilinear
    rule (include/retinanet_mi355x.h, rn_replay_compose), not cv2.resize.
"""
import math
import os

import numpy as np
import torch

from retinanet_mi355x import ops as _ops

BITS = _ops.RENDER_BITS

# 5x7 glyphs in the upper left of the 6x8 cell, ASCII 32..126, seven rows each, top to bottom
_GLYPHS = """
..... ..... ..... ..... ..... ..... .....
..X.. ..X.. ..X.. ..X.. ..X.. ..... ..X..
.X.X. .X.X. .X.X. ..... ..... ..... .....
.X.X. .X.X. XXXXX .X.X. XXXXX .X.X. .X.X.
..X.. .XXXX X.X.. .XXX. ..X.X XXXX. ..X..
XX... XX..X ...X. ..X.. .X... X..XX ...XX
.XX.. X..X. X.X.. .X... X.X.X X..X. .XX.X
.XX.. ..X.. .X... ..... ..... ..... .....
...X. ..X.. .X... .X... .X... ..X.. ...X.
.X... ..X.. ...X. ...X. ...X. ..X.. .X...
..... ..X.. X.X.X .XXX. X.X.X ..X.. .....
..... ..X.. ..X.. XXXXX ..X.. ..X.. .....
..... ..... ..... ..... .XX.. ..X.. .X...
..... ..... ..... XXXXX ..... ..... .....
..... ..... ..... ..... ..... .XX.. .XX..
..... ....X ...X. ..X.. .X... X.... .....
.XXX. X...X X..XX X.X.X XX..X X...X .XXX.
..X.. .XX.. ..X.. ..X.. ..X.. ..X.. .XXX.
.XXX. X...X ....X ...X. ..X.. .X... XXXXX
XXXXX ...X. ..X.. ...X. ....X X...X .XXX.
...X. ..XX. .X.X. X..X. XXXXX ...X. ...X.
XXXXX X.... XXXX. ....X ....X X...X .XXX.
..XX. .X... X.... XXXX. X...X X...X .XXX.
XXXXX ....X ...X. ..X.. .X... .X... .X...
.XXX. X...X X...X .XXX. X...X X...X .XXX.
.XXX. X...X X...X .XXXX ....X ...X. .XX..
..... .XX.. .XX.. ..... .XX.. .XX.. .....
..... .XX.. .XX.. ..... .XX.. ..X.. .X...
...X. ..X.. .X... X.... .X... ..X.. ...X.
..... ..... XXXXX ..... XXXXX ..... .....
.X... ..X.. ...X. ....X ...X. ..X.. .X...
.XXX. X...X ....X ...X. ..X.. ..... ..X..
.XXX. X...X ....X .XX.X X.X.X X.X.X .XXX.
.XXX. X...X X...X X...X XXXXX X...X X...X
XXXX. X...X X...X XXXX. X...X X...X XXXX.
.XXX. X...X X.... X.... X.... X...X .XXX.
XXX.. X..X. X...X X...X X...X X..X. XXX..
XXXXX X.... X.... XXXX. X.... X.... XXXXX
XXXXX X.... X.... XXXX. X.... X.... X....
.XXX. X...X X.... X.XXX X...X X...X .XXXX
X...X X...X X...X XXXXX X...X X...X X...X
.XXX. ..X.. ..X.. ..X.. ..X.. ..X.. .XXX.
..XXX ...X. ...X. ...X. ...X. X..X. .XX..
X...X X..X. X.X.. XX... X.X.. X..X. X...X
X.... X.... X.... X.... X.... X.... XXXXX
X...X XX.XX X.X.X X.X.X X...X X...X X...X
X...X X...X XX..X X.X.X X..XX X...X X...X
.XXX. X...X X...X X...X X...X X...X .XXX.
XXXX. X...X X...X XXXX. X.... X.... X....
.XXX. X...X X...X X...X X.X.X X..X. .XX.X
XXXX. X...X X...X XXXX. X.X.. X..X. X...X
.XXXX X.... X.... .XXX. ....X ....X XXXX.
XXXXX ..X.. ..X.. ..X.. ..X.. ..X.. ..X..
X...X X...X X...X X...X X...X X...X .XXX.
X...X X...X X...X X...X X...X .X.X. ..X..
X...X X...X X...X X.X.X X.X.X X.X.X .X.X.
X...X X...X .X.X. ..X.. .X.X. X...X X...X
X...X X...X X...X .X.X. ..X.. ..X.. ..X..
XXXXX ....X ...X. ..X.. .X... X.... XXXXX
.XXX. .X... .X... .X... .X... .X... .XXX.
..... X.... .X... ..X.. ...X. ....X .....
.XXX. ...X. ...X. ...X. ...X. ...X. .XXX.
..X.. .X.X. X...X ..... ..... ..... .....
..... ..... ..... ..... ..... ..... XXXXX
.X... ..X.. ...X. ..... ..... ..... .....
..... ..... .XXX. ....X .XXXX X...X .XXXX
X.... X.... X.XX. XX..X X...X X...X XXXX.
..... ..... .XXX. X.... X.... X...X .XXX.
....X ....X .XX.X X..XX X...X X...X .XXXX
..... ..... .XXX. X...X XXXXX X.... .XXX.
..XX. .X..X .X... XXX.. .X... .X... .X...
..... .XXXX X...X X...X .XXXX ....X .XXX.
X.... X.... X.XX. XX..X X...X X...X X...X
..X.. ..... .XX.. ..X.. ..X.. ..X.. .XXX.
...X. ..... ..XX. ...X. ...X. X..X. .XX..
X.... X.... X..X. X.X.. XX... X.X.. X..X.
.XX.. ..X.. ..X.. ..X.. ..X.. ..X.. .XXX.
..... ..... XX.X. X.X.X X.X.X X...X X...X
..... ..... X.XX. XX..X X...X X...X X...X
..... ..... .XXX. X...X X...X X...X .XXX.
..... XXXX. X...X X...X XXXX. X.... X....
..... .XXXX X...X X...X .XXXX ....X ....X
..... ..... X.XX. XX..X X.... X.... X....
..... ..... .XXX. X.... .XXX. ....X XXXX.
.X... .X... XXX.. .X... .X... .X..X ..XX.
..... ..... X...X X...X X...X X..XX .XX.X
..... ..... X...X X...X X...X .X.X. ..X..
..... ..... X...X X...X X.X.X X.X.X .X.X.
..... ..... X...X .X.X. ..X.. .X.X. X...X
..... X...X X...X X...X .XXXX ....X .XXX.
..... ..... XXXXX ...X. ..X.. .X... XXXXX
...X. ..X.. ..X.. .X... ..X.. ..X.. ...X.
..X.. ..X.. ..X.. ..X.. ..X.. ..X.. ..X..
.X... ..X.. ..X.. ...X. ..X.. ..X.. .X...
..... ..... .X... X.X.X ...X. ..... .....
"""


def _font():
    rows = [line.split() for line in _GLYPHS.strip().splitlines()]
    assert len(rows) == 95 and all(len(r) == 7 and all(len(c) == 5 for c in r) for r in rows)
    table = np.zeros((95, 8), np.uint8)
    for g, glyph in enumerate(rows):
        for r, cells in enumerate(glyph):
            table[g, r] = sum(1 << (5 - c) for c, ch in enumerate(cells) if ch == "X")
    return table


FONT = _font()                      # uint8 [95,8]: 8 rows of 6 bits per glyph, bit 5 the left column
CELL_W, CELL_H = 6, 8
LINE_H = 12                         # the reference's text height + 4 (:874-880), with the 8-row cell
BANNER_AT, BANNER_SCALE = (20, 30), 2
TRACK_THICKNESS, DET_THICKNESS, PRIOR_THICKNESS = 3, 1, 1


def mosaic_layout(n):
    """(rows, cols) of the combined image of n cameras: rows = round(sqrt(n)), cols = ceil(n / rows), camera i in tile
    ``(i // cols, i % cols)``.  The reference sizes its canvas the same way (:899-902) but indexes it with ``// n_row`` and
    ``% n_row`` (:904-905), which overruns its own canvas for 2 or 18 cameras; dividing by the column count is the evident
    intent and what is done here."""
    rows = int(np.round(np.sqrt(n)))
    return rows, int(math.ceil(n / rows))


def label_lines(state7, class_name, obj_id, label_len=5):
    """The reference's label strings (:799-804, :855-862) of one track: state7 = (x, y, l, w, h, direction, speed) as
    ``filter.view(with_direction=True)`` gives it.  fp32 arithmetic and numpy's rounding (half to even), as written there."""
    s = np.asarray(state7, dtype=np.float32)
    speed = np.round(np.abs(s[6]) * np.float32(3600) / np.float32(5280) * np.float32(10)) / np.float32(10)    # mph
    dims = np.round(s[2:5] * np.float32(10)) / np.float32(10)
    direction = "WB" if s[5] == -1 else "EB"
    full = ["{} {}:".format(class_name, obj_id), "{:.1f}mph {}".format(float(speed), direction), "L: {:.1f}ft".format(float(dims[0])),
            "W: {:.1f}ft".format(float(dims[1])), "H: {:.1f}ft".format(float(dims[2]))]
    return full[:label_len]


def banner_text(bias, mu_v):
    return "Estimated time bias: {:.4f}s ({:.1f}ft)".format(bias, float(bias * mu_v))           # :888


def label_records(labels, bits=BITS):
    """labels: [(box index, camera, [lines])] -> (rect records int32 [n,8], text runs int32 [m,9], bytes) of the label blocks
    (:864-882 with the 6x8 cell in place of getTextSize): the rectangle from c1 = (int(min x), int(max y)) of the box to c1 +
    (6 L + 10, n_lines * 12) inclusive, L the longest line; line k (from 1) on the baseline c1.y + 12 k.  Labels with the same
    lines (a track in every camera) share their bytes; the records are laid out with numpy, one pass over the labels.
    ``bits``: the table naming the ``label`` and ``label_text`` bit numbers (the replay's plane has its own)."""
    text, keys, shapes, spans = bytearray(), {}, [], []               # per distinct label: (longest, n_lines), [(start, length)]
    box, cam, key = (np.empty(len(labels), np.int32) for _ in range(3))
    for j, (b, c, lines) in enumerate(labels):
        t = tuple(lines)
        k = keys.get(t)
        if k is None:
            k = keys[t] = len(shapes)
            raws = [line.encode("latin-1", "replace") for line in t]
            shapes.append((max((len(r) for r in raws), default=0), len(raws)))
            spans.append([])
            for r in raws:
                spans[k].append((len(text), len(r)))
                text += r
        box[j], cam[j], key[j] = b, c, k
    if not shapes:
        return np.zeros((0, 8), np.int32), np.zeros((0, 9), np.int32), text
    shapes = np.asarray(shapes, np.int32).reshape(-1, 2)
    longest, n_lines = shapes[key, 0], shapes[key, 1]
    keep = n_lines > 0
    zero = np.zeros(int(keep.sum()), np.int32)
    rects = np.stack((zero, zero, CELL_W * longest[keep] + 11, LINE_H * n_lines[keep] + 1, cam[keep], zero, box[keep],
                      zero + bits["label"]), axis=1)
    runs = []
    for k in range(int(n_lines.max())):                               # line k of every label that has one
        has = n_lines > k
        span = np.asarray([sp[k] if len(sp) > k else (0, 0) for sp in spans], np.int32).reshape(-1, 2)[key[has]]
        zero = np.zeros(int(has.sum()), np.int32)
        runs.append(np.stack((zero, zero + LINE_H * (k + 1), cam[has], box[has], zero + 1, zero, zero + bits["label_text"],
                              span[:, 0], span[:, 1]), axis=1))
    return rects.astype(np.int32), np.concatenate(runs).astype(np.int32) if runs else np.zeros((0, 9), np.int32), text


class Renderer:
    """``render`` paints and composes one frame of all cameras; ``render_tracker`` restates ``plot()`` on a tracker.
    ``rendered``: the last canvas, uint8 [rows*H, cols*W, 3] RGB on the device; ``views()``: the per-camera windows of it.
    ``copies`` counts the device -> host copies made for the label numbers (one per ``render_tracker`` call), ``last`` holds
    the arguments of the last ``render`` call (device tensors, not copied)."""

    def __init__(self, n_cam, H, W, device, mean=_ops.IMAGENET_MEAN, std=_ops.IMAGENET_STD):
        self.n_cam, self.H, self.W, self.device = int(n_cam), int(H), int(W), torch.device(device)
        self.rows, self.cols = mosaic_layout(self.n_cam)
        self.mean, self.std = tuple(mean), tuple(std)
        self.mask = _ops.render_mask(self.n_cam, self.H, self.W, self.device)
        self.font = torch.from_numpy(FONT).to(self.device)
        self._cam_ids = torch.arange(self.n_cam, dtype=torch.int32, device=self.device)
        self.rendered, self.last = None, None
        self.copies = 0

    def views(self, canvas=None):
        canvas = self.rendered if canvas is None else canvas
        H, W, C = self.H, self.W, self.cols
        return [canvas[(i // C) * H:(i // C + 1) * H, (i % C) * W:(i % C + 1) * W] for i in range(self.n_cam)]

    def _boxes(self, what, pair):
        if pair is None:
            return None
        corners, cam = pair
        corners = corners.to(self.device, torch.float64).reshape(-1, 8, 2).contiguous()
        cam = cam.to(self.device, torch.int32).reshape(-1).contiguous()
        if len(corners) != len(cam):
            raise ValueError("%s: %d boxes and %d camera indices" % (what, len(corners), len(cam)))
        return (corners, cam) if len(cam) else None

    def render(self, frames, tracks=None, detections=None, priors=None, crops=None, labels=None, banners=None, fancy_crop=True):
        """frames fp32 [n_cam,3,H,W] on the device.  tracks / detections / priors: (image corners [n,8,2], camera [n]) or
        None; crops: (boxes [k,4] x1 y1 x2 y2, camera [k]) or None; labels: [(index into tracks, camera, [lines])]; banners: one
        string per camera.  -> the canvas.  A pure function of its arguments: one mask clear, the paint launches, one
        compose, and one upload of the label and banner records."""
        crops_present = self.paint(tracks, detections, priors, crops, labels, banners, fancy_crop)
        self.last["frames"] = frames
        self.rendered = _ops.render_compose(frames, self.mask, crops_present, self.cols, self.mean, self.std)
        return self.rendered

    def paint(self, tracks=None, detections=None, priors=None, crops=None, labels=None, banners=None, fancy_crop=True):
        """The first half of ``render``: clears the mask plane and paints every layer into it.  -> crops_present."""
        tracks, detections, priors = (self._boxes(k, v) for k, v in (("tracks", tracks), ("detections", detections), ("priors", priors)))
        labels = [] if labels is None or tracks is None else [(int(b), int(c), list(lines)) for b, c, lines in labels]
        self.last = dict(tracks=tracks, detections=detections, priors=priors, crops=crops, labels=labels,
                         banners=None if banners is None else list(banners), fancy_crop=bool(fancy_crop))
        mask = self.mask
        mask.zero_()
        for pair, thick, bit in ((priors, PRIOR_THICKNESS, "prior"), (tracks, TRACK_THICKNESS, "track"), (detections, DET_THICKNESS, "det")):
            if pair is not None:
                _ops.render_edges(pair[0], pair[1], thick, BITS[bit], mask)
        if crops is not None and len(crops[0]):
            box = crops[0].to(self.device).int().reshape(-1, 4)                   # crops.int() of :770 / :839
            cam = crops[1].to(self.device, torch.int32).reshape(-1, 1)
            if fancy_crop:                                                        # the window im[y1:y2, x1:x2] (:845)
                mode, bit = 0, BITS["in_crop"]
            else:                                                                 # cv2.rectangle(c1, c2, white, 1): c2 inclusive
                box, mode, bit = torch.cat((box[:, :2], box[:, 2:] + 1), dim=1), 1, BITS["crop_edge"]
            col = lambda v: torch.full_like(cam, v)                               # noqa: E731  (filled on the device: no upload)
            _ops.render_rects(torch.cat((box, cam, col(mode), col(-1), col(bit)), dim=1).contiguous(), mask)
        rects, runs, text = label_records(labels)
        extra = []
        for b, line in enumerate(banners or []):
            raw = line.encode("latin-1", "replace")
            for dilate, bit in ((1, "banner_edge"), (0, "banner_text")):          # the white pass, then the black one (:890-891)
                extra.append([BANNER_AT[0], BANNER_AT[1], b, -1, BANNER_SCALE, dilate, BITS[bit], len(text), len(raw)])
            text += raw
        if extra:
            runs = np.concatenate((runs, np.asarray(extra, np.int32)))
        if len(runs):
            d_rects, d_runs, d_text = self._upload(rects, runs, text)
            anchors = None if tracks is None else tracks[0]
            if len(d_rects):
                _ops.render_rects(d_rects, mask, anchors)
            _ops.render_text(d_runs, d_text, self.font, mask, anchors)
        return crops is not None and bool(fancy_crop)

    def _upload(self, rects, runs, text):
        """Rect records, text runs and bytes in ONE host -> device copy; views of the device buffer."""
        r = np.ascontiguousarray(rects, np.int32).reshape(-1, 8)
        t = np.ascontiguousarray(runs, np.int32).reshape(-1, 9)
        buf = np.concatenate((r.view(np.uint8).reshape(-1), t.view(np.uint8).reshape(-1), np.frombuffer(bytes(text), np.uint8)))
        dev = torch.from_numpy(buf).to(self.device)
        a, b = r.size * 4, r.size * 4 + t.size * 4
        return dev[:a].view(torch.int32).view(-1, 8), dev[a:b].view(torch.int32).view(-1, 9), dev[b:]

    def render_tracker(self, trk, detections, det_cams, pre_loc=None, crop_boxes=None, crop_cams=None, label_len=5, single_box=True,
                       fancy_crop=True):
        """``plot(detections, camera_idxs, ..., pre_locations=pre_loc, label_len, single_box, crops)`` (:733-896) of tracker
        ``trk``: per camera the filter viewed at that camera's time stamp plus bias (:792-793), projected through the
        wrapper's switch; every track is drawn in every camera, as the reference does; detections (state form) in their own
        camera.  ``views_state`` / ``view_ids`` keep the per-camera views [n_cam*n,7] and the ids.  Reads the filter, never
        writes it."""
        import mc3d_post
        dev, flt, nc = self.device, trk.filter, self.n_cam
        _, _, P1, P2 = mc3d_post._camera_matrices(trk, dev)
        n = 0 if flt.X is None else len(flt.X)
        tracks, labels, ids = None, [], []
        self.views_state = torch.empty((nc * n, 7), dtype=torch.float32, device=dev)
        if n:
            for c in range(nc):
                dts = flt.get_dt(float(trk.timestamps[c]) + float(trk.ts_bias[c]))
                ids, _ = flt.view(with_direction=True, dt=dts, out=self.views_state[c * n:(c + 1) * n])
            cam = self._cam_ids.repeat_interleave(n)
            tracks = (_ops.hg_to_im(self.views_state, P1, P2, cam, from_state=True), cam)
            host = self.views_state.cpu().numpy()                                  # the label numbers: the frame's one copy
            self.copies += 1
            names = [trk.class_dict[int(np.argmax(trk.all_classes[oid]))] for oid in ids]
            lines = {}                                                             # a view moves x only: most rows repeat per camera
            for c in range(nc):
                for i, oid in enumerate(ids):
                    row = host[c * n + i]
                    key = (i, row[2:7].tobytes())
                    if key not in lines:
                        lines[key] = label_lines(row, names[i], oid, label_len)
                    labels.append((c * n + i, c, lines[key]))
        self.view_ids = list(ids)
        dets = None
        if detections is not None and len(detections):
            dc = det_cams.to(dev, torch.int32).reshape(-1).contiguous()
            dets = (_ops.hg_to_im(detections.to(dev), P1, P2, dc, from_state=True), dc)
        priors = None
        if pre_loc is not None and len(pre_loc) and not single_box:
            cam = self._cam_ids.repeat_interleave(len(pre_loc))
            priors = (_ops.hg_to_im(pre_loc.to(dev).repeat(nc, 1), P1, P2, cam, from_state=True), cam)
        crops = None if crop_boxes is None else (crop_boxes, crop_cams)
        mu_v = float(flt.mu_v)
        banners = [banner_text(float(trk.ts_bias[c]), mu_v) for c in range(nc)] if getattr(trk, "est_ts", True) else None
        return self.render(trk.frames, tracks, dets, priors, crops, labels, banners, fancy_crop)


REPLAY_BITS = _ops.REPLAY_BITS
REPLAY_THICKNESS = 2                # plot_in's thickness argument (datareader.py:351)
replay_layout = _ops.replay_layout


def replay_label_lines(view7, class_name, obj_id, time):
    """plot_labels' five lines (datareader.py:262-268) of one object: view7 = the fp32 view (x, y, l, w, h, direction, v), its
    numbers formatted as the fp32 tensor elements the reference formats; ``time`` = ts + dt through ``str``."""
    s = np.asarray(view7, dtype=np.float32)
    return ["{} {}:".format(class_name, obj_id), "L: {:.1f}ft".format(float(s[2])), "W: {:.1f}ft".format(float(s[3])),
            "H: {:.1f}ft".format(float(s[4])), "{}".format(time)]


class Replayer:
    """One output frame of ``Data_Reader.plot_in``: ``replay`` shifts and projects the objects of a label instant into every
    camera (``ops.replay_boxes``), paints boxes and label blocks into its mask plane and composes the uint8 mosaic at the
    output size (``ops.replay_compose``).  One host -> device copy per frame: the cameras' dt with the label records.
    ``rendered``: the last canvas; ``last``: views, corners, side and camera of the last frame (device tensors)."""

    def __init__(self, n_cam, H, W, device):
        self.n_cam, self.H, self.W, self.device = int(n_cam), int(H), int(W), torch.device(device)
        self.rows, self.cols = replay_layout(self.n_cam)
        self.mask = _ops.render_mask(self.n_cam, self.H, self.W, self.device)
        self.font = torch.from_numpy(FONT).to(self.device)
        self.frames = torch.empty((self.n_cam, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        self.rendered, self.last = None, None

    def records(self, lines_per_object):
        """Label records of one frame, on the host: lines_per_object[c][i] = the lines of object i in camera c ->
        (rects int32 [m,8], runs int32 [k,9], text bytes), anchored at box c * n + i."""
        labels = []
        for c, per_cam in enumerate(lines_per_object):
            n = len(per_cam)
            labels += [(c * n + i, c, lines) for i, lines in enumerate(per_cam)]
        return label_records(labels, REPLAY_BITS)

    def _upload(self, dts, rects, runs, text):
        """dt, rect records, text runs and bytes in ONE host -> device copy; views of the device buffer."""
        d = np.ascontiguousarray(dts, np.float64).reshape(-1)
        r = np.ascontiguousarray(rects, np.int32).reshape(-1, 8)
        t = np.ascontiguousarray(runs, np.int32).reshape(-1, 9)
        buf = np.concatenate((d.view(np.uint8), r.view(np.uint8).reshape(-1), t.view(np.uint8).reshape(-1), np.frombuffer(bytes(text), np.uint8)))
        dev = torch.from_numpy(buf).to(self.device)
        a = d.size * 8
        b = a + r.size * 4
        c = b + t.size * 4
        return dev[:a].view(torch.float64), dev[a:b].view(torch.int32).view(-1, 8), dev[b:c].view(torch.int32).view(-1, 9), dev[c:]

    def paint(self, corners, side, cam, d_rects, d_runs, d_text):
        """Clears the mask plane and paints boxes (primary where side == 0, else secondary) and label blocks into it."""
        mask = self.mask
        mask.zero_()
        if len(cam):
            off = torch.full_like(cam, -1)                                      # a camera outside [0, n_cam) paints nothing
            _ops.render_edges(corners, torch.where(side == 0, cam, off), REPLAY_THICKNESS, REPLAY_BITS["primary"], mask)
            _ops.render_edges(corners, torch.where(side == 0, off, cam), REPLAY_THICKNESS, REPLAY_BITS["secondary"], mask)
            if len(d_rects):
                _ops.render_rects(d_rects, mask, corners)
            if len(d_runs):
                _ops.render_text(d_runs, d_text, self.font, mask, corners)
        return mask

    def replay(self, frames, state7, offset, count, dts, P1, P2, lines_per_object, size=None, swap_rb=False):
        """frames: n_cam uint8 [H,W,3] device tensors (or one [n_cam,H,W,3]); state7 fp32 [R,7] on the device, rows [offset,
        offset + count) the instant's objects; dts: n_cam host floats; lines_per_object as ``records``.  -> the canvas."""
        if torch.is_tensor(frames):
            stacked = frames
        else:
            for c, f in enumerate(frames):
                self.frames[c].copy_(f)
            stacked = self.frames
        rects, runs, text = self.records(lines_per_object)
        d_dt, d_rects, d_runs, d_text = self._upload(dts, rects, runs, text)
        views, corners, side, cam = _ops.replay_boxes(state7, d_dt, P1, P2, offset, count)
        self.paint(corners, side, cam, d_rects, d_runs, d_text)
        self.last = dict(views=views, corners=corners, side=side, cam=cam)
        self.rendered = _ops.replay_compose(stacked, self.mask, size, swap_rb)
        return self.rendered


class PngWriter:
    """The reference's frame directories (:137-154): ``<out>/<camera>/00000.png`` per camera and ``<out>/combined/00000.png``,
    numbered in the order they are written (util_track/mp_writer.py:44).  Written through PIL."""

    def __init__(self, out_dir, cameras):
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("writing output frames needs PIL (Pillow), which is not installed: pass "
                               "params['render']['out'] = None to render without writing") from e
        self._image = Image
        self.out_dir, self.cameras = str(out_dir), list(cameras)
        for name in self.cameras + ["combined"]:
            os.makedirs(os.path.join(self.out_dir, name), exist_ok=True)
        self.frame = 0

    def __call__(self, canvas, views):
        """canvas uint8 [rows*H, cols*W, 3] and its per-camera windows, on the host."""
        name = "{}.png".format(str(self.frame).zfill(5))
        for cam, im in zip(self.cameras, views):
            self._image.fromarray(np.ascontiguousarray(im)).save(os.path.join(self.out_dir, cam, name))
        self._image.fromarray(np.ascontiguousarray(canvas)).save(os.path.join(self.out_dir, "combined", name))
        self.frame += 1

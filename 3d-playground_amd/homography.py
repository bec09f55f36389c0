"""Drop-in for the transform half of the reference's ``homography.py``: ``Homography`` and
``Homography_Wrapper`` with the same attributes (``correspondence[name] = {"H","H_inv","P",...}`` numpy float64,
``default_correspondence``, ``class_heights``) and the same methods for the per-frame hot path
(homography.py:274-333, 388-551, 793-862): state_to_space, space_to_state, space_to_im, im_to_space,
state_to_im, im_to_state, guess_heights, height_from_template; ``name`` may be None, a str or a list of names.

Objects are plain picklable classes (the reference pickles them, homography.py:22-23, 75-76) holding only
numpy matrices; inputs and outputs are CPU tensors exactly as every caller of the reference passes and expects
(state fp32, image points fp64), while the arithmetic runs in the HIP kernels of libretinanet_mi355x.so on
``device`` (default cuda:0).  A device tensor input stays on its device.

The set-up half is here too (homography.py:12-154, 239-271, 336-385, 554-666): ``get_homographies``, ``line_to_point``,
``find_vanishing_point`` (+ ``find_vanishing_points``: many line sets, one launch), ``add_i24_camera``,
``add_correspondence``, ``remove_correspondence``, ``test_transformation`` and ``scale_Z``, on the kernels of
csrc/calibrate.hip.  The vanishing-point search, the reprojection error and the ``scale_Z`` search restate the reference's
arithmetic operation by operation (numpy's ``arange`` / ``linspace`` rules included; ``scale_Z`` leaves ``P`` scaled by the
LAST candidate it evaluated, not the best, exactly as the reference does).  ``add_correspondence`` fits ``H`` / ``H_inv``
with ``ops.fit_homography`` (normalised DLT + Gauss-Newton) where the reference calls ``cv2.findHomography``: parity with
OpenCV is UNPINNED -- OpenCV is not available to build or test against -- so a caller who owns cv2 and needs its bits passes
``H=`` / ``H_inv=``, which are stored as they are.  Differences a caller can see: ``remove_correspondence`` works (the
reference's misspells ``self.correspondences`` and can only raise AttributeError); a non-finite vanishing-point start, an
empty ``boxes`` or a ``granularity`` at or above the first step raise ValueError (the reference dies with ValueError /
TypeError / NameError); plotting (``im is not None``) raises NotImplementedError.
``load_i24_csv`` (homography.py:750-791) is here: pure ``csv``, host side.
"""
import csv
import os
import _pickle as pickle

import numpy as np
import torch

from retinanet_mi355x import ops as _ops

I24_CAMERAS = ["p1c1", "p1c2", "p1c3", "p1c4", "p1c5", "p1c6", "p2c1", "p2c3", "p2c5", "p2c6", "p3c1", "p3c2", "p3c3", "p3c4",
               "p3c5", "p3c6"]                                                 # homography.py:30


def get_homographies(save_file="i24_all_homography.cpkl", directory="/home/worklab/Documents/derek/i24-dataset-gen/DATA/tform2",
                     direction="EB", fit_Z=True, data_dir="/home/worklab/Data/dataset_alpha/manual_correction",
                     vp_dir="/home/worklab/Documents/derek/i24-dataset-gen/DATA/vp", cameras=None):
    """homography.py:12-78: the Homography pickled in ``save_file`` if that exists; otherwise one built from the
    transform-point files of ``directory`` and the axis files of ``vp_dir``, its Z axis fitted to the first non-empty
    frame of each camera's label file in ``data_dir``, and pickled.  ``data_dir``, ``vp_dir`` and ``cameras`` default to
    what the reference hard-codes (homography.py:30-35)."""
    try:
        with open(save_file, "rb") as f:
            hg = pickle.load(f)
    except FileNotFoundError:
        print("Regenerating i24 homgraphy...")
        hg = Homography()
        for camera_name in (I24_CAMERAS if cameras is None else cameras):
            print("Adding camera {} to homography".format(camera_name))
            data_file = os.path.join(data_dir, "rectified_{}_0_track_outputs_3D.csv".format(camera_name))
            vp_file = os.path.join(vp_dir, "{}_axes.csv".format(camera_name))
            point_file = os.path.join(directory, "{}_{}_im_lmcs_transform_points.csv".format(camera_name, direction))
            if not os.path.exists(point_file):
                point_file = os.path.join(directory, "{}_im_lmcs_transform_points.csv".format(camera_name))
                if not os.path.exists(point_file):
                    other_direction = "EB" if direction == "WB" else "WB"
                    point_file = os.path.join(directory, "{}_{}_im_lmcs_transform_points.csv".format(camera_name, other_direction))
            hg.add_i24_camera(point_file, vp_file, camera_name)
            if fit_Z:
                try:                                                            # homography.py:48-73: any failure is passed over
                    labels, data = load_i24_csv(data_file)
                    i = 0
                    frame_data = data[i]
                    while len(frame_data) == 0:
                        i += 1
                        frame_data = data[i]
                    boxes = []
                    classes = []
                    for item in frame_data:
                        if len(item[11]) > 0:
                            boxes.append(np.array(item[11:27]).astype(float))
                            classes.append(item[3])
                    boxes = torch.from_numpy(np.stack(boxes))
                    boxes = torch.stack((boxes[:, ::2], boxes[:, 1::2]), dim=-1)
                    heights = hg.guess_heights(classes)
                    hg.scale_Z(boxes, heights, name=camera_name)
                except Exception:
                    pass
        with open(save_file, "wb") as f:
            pickle.dump(hg, f)
    return hg


def line_to_point(line, point):
    """homography.py:81-94: distance of ``point`` (x, y) from the line through (x0, y0) and (x1, y1); host side."""
    numerator = np.abs((line[2] - line[0]) * (line[1] - point[1]) - (line[3] - line[1]) * (line[0] - point[0]))
    return numerator / (np.sqrt((line[2] - line[0]) ** 2 + (line[3] - line[1]) ** 2) + 1e-08)


def find_vanishing_points(list_of_line_sets, device="cuda:0"):
    """find_vanishing_point (homography.py:96-154) for every set of lines [(x0, y0, x1, y1, ...), ...] in one launch ->
    [[px, py], ...].  A set of fewer than two lines raises IndexError as the reference's ``lines[1]`` does; a starting
    point that is not finite raises ValueError (the reference fails inside np.arange)."""
    sets = []
    for lines in list_of_line_sets:
        if len(lines) < 2:
            raise IndexError("list index out of range")
        sets.append(np.stack([np.asarray(line, dtype=np.float64)[:4] for line in lines]))
    if len(sets) == 0:
        return []
    offsets = np.cumsum([0] + [len(s) for s in sets]).astype(np.int64)
    dev = torch.device(device)
    out, _, status = _ops.vanishing_points(torch.from_numpy(np.concatenate(sets)).to(dev), torch.from_numpy(offsets).to(dev))
    out, status = out.cpu().numpy(), status.cpu().numpy()
    for i, st in enumerate(status):
        if st & _ops.VP_BAD_START:
            raise ValueError("arange: cannot compute length (line set %d: the starting point (%s, %s) is not finite)"
                             % (i, out[i, 0], out[i, 1]))
        if st:
            raise RuntimeError("vanishing-point search of line set %d failed with status %d" % (i, st))
    return [[out[i, 0], out[i, 1]] for i in range(len(sets))]


def find_vanishing_point(lines, device="cuda:0"):
    return find_vanishing_points([lines], device=device)[0]


def load_i24_csv(file):
    """homography.py:750-791: -> (the ``Frame #`` header row, {frame index: [row, ...]}).  Lines up to and including the row
    whose first cell is ``Frame #`` are headers; empty rows are skipped; rows of one frame index gather under one key in
    file order, wherever they appear."""
    with open(file, "r") as f:
        rows = list(csv.reader(f))
    data, headers, in_headers = {}, None, True
    for row in rows:
        if in_headers:
            headers = row
            in_headers = not (len(row) > 0 and row[0] == "Frame #")
        elif len(row) > 0:
            data.setdefault(int(row[0]), []).append(row)
    return headers, data


class Homography():
    def __init__(self, f1=None, f2=None, device="cuda:0"):
        if f1 is not None or f2 is not None:
            raise NotImplementedError("custom state<->space functions run as Python in the reference "
                                      "(homography.py:180-186); only the built-in I-24 formulation has kernels")
        self.device = device
        self.correspondence = {}
        self.default_correspondence = None
        self.class_heights = {                      # homography.py:191-202
            "sedan": 4, "midsize": 5, "van": 6, "pickup": 5, "semi": 12, "truck (other)": 12, "truck": 12,
            "motorcycle": 4, "trailer": 3, "other": 5,
        }
        self.class_dims = {                         # homography.py:205-216
            "sedan": [16, 6, 4], "midsize": [18, 6.5, 5], "van": [20, 6, 6.5], "pickup": [20, 6, 5],
            "semi": [55, 9, 12], "truck (other)": [25, 9, 12], "truck": [25, 9, 12], "motorcycle": [7, 3, 4],
            "trailer": [16, 7, 3], "other": [18, 6.5, 5],
        }
        names = ["sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer"]
        self.class_dict = {n: i for i, n in enumerate(names)}          # homography.py:218-235 (both directions)
        self.class_dict["truck"] = 5
        self.class_dict.update({i: n for i, n in enumerate(names)})

    # ---- plumbing
    def _dev(self, t):
        return t.device if t.is_cuda else torch.device(self.device)

    def _matrices(self, key, name, dev):
        """(stacked fp64 matrices on device, per-object int32 index or None)."""
        if name is None:
            name = self.default_correspondence
        if isinstance(name, list):
            uniq = sorted(set(name))
            pos = {n: i for i, n in enumerate(uniq)}
            mats = np.stack([np.asarray(self.correspondence[n][key], dtype=np.float64) for n in uniq])
            idx = torch.tensor([pos[n] for n in name], dtype=torch.int32, device=dev)
            return torch.from_numpy(mats).to(dev), idx
        mats = np.asarray(self.correspondence[name][key], dtype=np.float64)[None]
        return torch.from_numpy(np.ascontiguousarray(mats)).to(dev), None

    @staticmethod
    def _back(out, like):
        return out if like.is_cuda else out.cpu()

    # ---- set-up (homography.py:239-271, 336-385)
    def add_i24_camera(self, point_path, vp_path, camera_name):
        corr_pts = []
        space_pts = []
        with open(point_path, "r") as f:
            lines = f.readlines()
            for line in lines[1:-4]:
                line = line.rstrip("\n").split(",")
                corr_pts.append([float(line[0]), float(line[1])])
                space_pts.append([float(line[2]), float(line[3])])
        axes = {"0": [], "1": [], "2": []}
        with open(vp_path, "r") as f:
            for item in csv.reader(f):
                if item[4] in axes:
                    axes[item[4]].append(np.array(item).astype(float))
        vps = find_vanishing_points([axes["0"], axes["1"], axes["2"]], device=self.device)     # the three in one launch
        self.add_correspondence(corr_pts, space_pts, vps, name=camera_name)

    def _fit_pair(self, corr_pts, space_pts):
        dev = torch.device(self.device)
        a, b = torch.from_numpy(np.ascontiguousarray(corr_pts, dtype=np.float64)), torch.from_numpy(np.ascontiguousarray(space_pts, dtype=np.float64))
        n = a.shape[0]
        if a.dim() != 2 or a.shape[1] != 2 or b.shape != a.shape:
            raise ValueError("corr_pts and space_pts are n (x, y) pairs each; got %s and %s" % (tuple(a.shape), tuple(b.shape)))
        offsets = torch.tensor([0, n, 2 * n], dtype=torch.int64, device=dev)
        H, status = _ops.fit_homography(torch.cat((a, b)).to(dev), torch.cat((b, a)).to(dev), offsets)
        status = status.cpu().tolist()
        if any(status):
            raise ValueError("no plane homography fits these %d point pairs (fewer than 4, collinear, or a non-finite "
                             "result; status %s)" % (n, status))
        H = H.cpu().numpy()
        return H[0], H[1]

    def add_correspondence(self, corr_pts, space_pts, vps, name=None, H=None, H_inv=None):
        """homography.py:336-376.  H / H_inv given: stored as they are (the way to keep cv2.findHomography's own bits);
        otherwise both are fitted by ops.fit_homography, two separate fits as in the reference (parity with OpenCV unpinned)."""
        if name is None:
            name = self.default_correspondence
        corr_pts = np.stack(corr_pts)
        space_pts = np.stack(space_pts)
        cor = {}
        cor["vps"] = vps
        cor["corr_pts"] = corr_pts
        cor["space_pts"] = space_pts
        if H is None or H_inv is None:
            fit_H, fit_H_inv = self._fit_pair(corr_pts, space_pts)
        cor["H"] = fit_H if H is None else H
        cor["H_inv"] = fit_H_inv if H_inv is None else H_inv
        P = np.zeros([3, 4])
        P[:, 0] = cor["H_inv"][:, 0]
        P[:, 1] = cor["H_inv"][:, 1]
        P[:, 3] = cor["H_inv"][:, 2]
        P[:, 2] = np.array([vps[2][0], vps[2][1], 1]) * 0.01
        cor["P"] = P
        self.correspondence[name] = cor
        if self.default_correspondence is None:
            self.default_correspondence = name

    def remove_correspondence(self, name):
        """homography.py:380-385 with its evident intent: the reference deletes from ``self.correspondences``, which does
        not exist, so it can only raise AttributeError."""
        try:
            del self.correspondence[name]
            print("Deleted correspondence for {}".format(name))
        except KeyError:
            print("Tried to delete correspondence {}, but this does not exist".format(name))

    # ---- reprojection error and the Z scale (homography.py:554-666)
    def _calib_matrices(self, name, dev):
        cor = self.correspondence[name]
        return (torch.from_numpy(np.ascontiguousarray(cor["H"], dtype=np.float64)).to(dev),
                torch.from_numpy(np.ascontiguousarray(cor["P"], dtype=np.float64)).to(dev))

    def test_transformation(self, points, classes=None, name=None, im=None, heights=None, verbose=True):
        if name is None:
            name = self.default_correspondence
        if heights is None:
            if classes is None:
                print("Must either specify heights or classes for boxes")
                return
            else:
                guess_heights = self.guess_heights(classes)
        else:
            guess_heights = heights
        if im is not None:
            raise NotImplementedError("plotting the reprojected boxes (homography.py:596-602) needs OpenCV")
        dev = self._dev(points)
        H, P = self._calib_matrices(name, dev)
        err = self._back(_ops.hg_reproj_error(points.to(dev), guess_heights.to(dev), H, P,
                                              torch.ones(1, dtype=torch.float64, device=dev)), points)
        top_error, bottom_error = err[0, 0], err[0, 1]
        if verbose:
            print("Average distance between reprojected points and original points:")
            print("-----------------------------")
            print("Top: {} pixels".format(top_error))
            print("Bottom: {} pixels".format(bottom_error))
        return top_error + bottom_error

    def scale_Z(self, boxes, heights, name=None, granularity=1e-06, max_scale=10):
        """homography.py:607-666.  Like the reference this leaves P scaled by the LAST candidate evaluated (the upper
        bound of the final iteration), not by the best one."""
        if name is None:
            name = self.default_correspondence
        P_orig = self.correspondence[name]["P"].copy()
        if boxes.shape[0] == 0:
            raise ValueError("scale_Z needs at least one box (the reference fails with a TypeError on None - step_size)")
        dev = self._dev(boxes)
        H, P = self._calib_matrices(name, dev)
        _, out, info = _ops.hg_scale_z(boxes.to(dev), heights.to(dev), H, P, granularity, max_scale)
        out, (iters, status) = out.cpu(), info.cpu().tolist()
        if status & _ops.SZ_BAD_FIRST_STEP:
            raise ValueError("scale_Z: the first grid step (max_scale - granularity) / 9 is not above granularity, so no "
                             "candidate is evaluated (the reference fails with a NameError on best_error)")
        if status & _ops.SZ_NO_WINNER:
            raise ValueError("scale_Z: every reprojection error was NaN (the reference fails with a TypeError on None - step_size)")
        if status:
            raise RuntimeError("scale_Z did not reach granularity %s within %d iterations" % (granularity, _ops.SZ_MAX_ITERS))
        P = P_orig.copy()
        P[:, 2] *= float(out[0])
        self.correspondence[name]["P"] = P
        print("Best Error: {}".format(out[2]))

    # ---- state <-> space (homography.py:274-333)
    def i24_state_to_space(self, points):
        return self._back(_ops.hg_state_to_space(points.to(self._dev(points))), points)

    def i24_space_to_state(self, points):
        return self._back(_ops.hg_space_to_state(points.to(self._dev(points))), points)

    def state_to_space(self, points):
        return self.i24_state_to_space(points)

    def space_to_state(self, points):
        return self.i24_space_to_state(points)

    # ---- space <-> image (homography.py:388-476)
    def im_to_space(self, points, name=None, heights=None):
        if heights is None:
            print("No heights were input")              # homography.py:430-432
            return
        dev = self._dev(points)
        H, idx = self._matrices("H", name, dev)
        self._need8(points, idx)
        return self._back(_ops.hg_from_im(points.to(dev), heights.to(dev), H, None, idx, to_state=False), points)

    def space_to_im(self, points, name=None):
        dev = self._dev(points)
        P, idx = self._matrices("P", name, dev)
        self._need8(points, idx)
        return self._back(_ops.hg_to_im(points.to(dev), P, None, idx, from_state=False), points)

    def state_to_im(self, points, name=None):
        dev = self._dev(points)
        P, idx = self._matrices("P", name, dev)
        return self._back(_ops.hg_to_im(points.to(dev), P, None, idx, from_state=True), points)

    def im_to_state(self, points, name=None, heights=None):
        if heights is None:
            print("No heights were input")
            return self.space_to_state(None)            # the reference fails the same way (None.shape)
        dev = self._dev(points)
        H, idx = self._matrices("H", name, dev)
        self._need8(points, idx)
        return self._back(_ops.hg_from_im(points.to(dev), heights.to(dev), H, None, idx, to_state=True), points)

    @staticmethod
    def _need8(points, idx):
        if points.dim() != 3 or points.shape[1] != 8:
            raise RuntimeError("the box transforms take 8 points per object (homography.py:405, 459 hard-code 8); "
                               "got %s" % (tuple(points.shape),))

    # ---- heights (homography.py:502-551)
    def guess_heights(self, classes):
        heights = torch.zeros(len(classes))
        for i in range(len(classes)):
            try:
                heights[i] = self.class_heights[classes[i]]
            except (KeyError, TypeError):
                heights[i] = self.class_heights["other"]
        return heights

    def height_from_template(self, template_boxes, template_space_heights, boxes):
        def im_height(b):
            top = torch.mean(b[:, 4:8, :], dim=1)
            bottom = torch.mean(b[:, 0:4, :], dim=1)
            return torch.sum(torch.sqrt(torch.pow(top - bottom, 2)), dim=1)
        return im_height(boxes) / (im_height(template_boxes) / template_space_heights)


class Homography_Wrapper():
    """Two homographies, one per travel direction; objects whose corner-0 space y > 60 use the second
    (homography.py:793-862)."""

    def __init__(self, hg1=None, hg2=None):
        if hg1 is None or hg2 is None:
            raise RuntimeError("the default constructor unpickles EB_homography2.cpkl / WB_homography2.cpkl, which the "
                               "reference does not ship (homography.py:824-826): pass two populated Homography objects")
        self.hg1 = hg1
        self.hg2 = hg2

    def guess_heights(self, classes):
        return self.hg1.guess_heights(classes)

    def state_to_space(self, points):
        return self.hg1.state_to_space(points)

    def space_to_state(self, points):
        return self.hg1.space_to_state(points)

    def height_from_template(self, template_boxes, template_space_heights, boxes):
        return self.hg1.height_from_template(template_boxes, template_space_heights, boxes)

    def _pair(self, key, name, dev):
        m1, idx = self.hg1._matrices(key, name, dev)
        m2, idx2 = self.hg2._matrices(key, name, dev)
        if m1.shape != m2.shape:
            raise RuntimeError("hg1 and hg2 must hold the same set of correspondence names (homography.py:821)")
        return m1, m2, idx

    def im_to_space(self, points, name=None, heights=None):
        dev = self.hg1._dev(points)
        H1, H2, idx = self._pair("H", self.hg1.default_correspondence if name is None else name, dev)
        return Homography._back(_ops.hg_from_im(points.to(dev), heights.to(dev), H1, H2, idx, to_state=False), points)

    def space_to_im(self, points, name=None):
        dev = self.hg1._dev(points)
        P1, P2, idx = self._pair("P", self.hg1.default_correspondence if name is None else name, dev)
        return Homography._back(_ops.hg_to_im(points.to(dev), P1, P2, idx, from_state=False), points)

    def im_to_state(self, points, name=None, heights=None):
        dev = self.hg1._dev(points)
        H1, H2, idx = self._pair("H", self.hg1.default_correspondence if name is None else name, dev)
        return Homography._back(_ops.hg_from_im(points.to(dev), heights.to(dev), H1, H2, idx, to_state=True), points)

    def state_to_im(self, points, name=None):
        dev = self.hg1._dev(points)
        P1, P2, idx = self._pair("P", self.hg1.default_correspondence if name is None else name, dev)
        return Homography._back(_ops.hg_to_im(points.to(dev), P1, P2, idx, from_state=True), points)

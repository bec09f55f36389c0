"""Drop-in for the reference's ``fit_filter_3D.py``: the parameters ``Torch_KF(device, INIT=kf_params)`` needs -- ``mu_Q``,
``Q`` (:242-304), ``mu_R``, ``R`` (:306-389), ``class_size`` / ``class_covariance`` (:394-441), ``mu_v`` and ``P``
(:444-485) -- refitted on the device after the detector has been retrained.

The reference is a cell script that opens its dataset, homography and checkpoint at import; its four cells are restated
here as functions of tensors, so the loader is the caller's.  Inputs and outputs may stay on the GPU: the image ->
state transforms run in ``rn_im_to_state`` / ``rn_state_to_im``, the filter step in ``rn_kf_predict`` (``util_track/kf.py``),
the nearest-box search in ``rn_fit_nearest`` and every mean / covariance in ``rn_residual_moments``.

``hg`` is a ``Homography_Wrapper`` (``hg.hg1`` / ``hg.hg2`` with ``correspondence[name]["H" / "P"]``), as in
``mc3d_post``.  ``cameras`` names the camera of every object: one name for all, a list of one name per object (the
reference's ``name=``), or ``(camera_names, camera_idxs)`` with an integer tensor that may already be on the device.
``classes`` are class names (through ``hg.guess_heights``, as in the script), class indices (through ``CLASS_NAMES``,
the script's ``class_dict``) or a float tensor of heights.

    import fit_filter
    kf_params = fit_filter.fit(hg, kf_params, tracklets_im, tracklet_classes, tracklet_cameras,
                               detector, frames, gt_im, gt_classes, frame_cameras)
    pickle.dump(kf_params, open("kf_params_save2.cpkl", "wb"))
"""
import numpy as np
import torch

from retinanet_mi355x import ops as _ops
from util_track.kf import Torch_KF

CLASS_NAMES = ["sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer"]   # :122-139
FPS = 30                                                                                                  # :270, :468


def _device(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda:0")


def _camera_matrices(hg, names, dev):
    """Per-camera H / P of both wrapper homographies stacked in ``names`` order (as mc3d_post._camera_matrices)."""
    def stack(h, k):
        m = np.stack([np.asarray(h.correspondence[c][k], dtype=np.float64) for c in names])
        return torch.from_numpy(np.ascontiguousarray(m)).to(dev)
    return stack(hg.hg1, "H"), stack(hg.hg2, "H"), stack(hg.hg1, "P"), stack(hg.hg2, "P")


def _cameras(hg, cameras, n, dev):
    """-> (H1, H2, P1, P2, int32 [n] index into them)."""
    if isinstance(cameras, str):
        names, idx = [cameras], torch.zeros(n, dtype=torch.int32, device=dev)
    elif isinstance(cameras, tuple) and len(cameras) == 2 and not isinstance(cameras[1], str):
        names = list(cameras[0])
        idx = torch.as_tensor(cameras[1]).to(dev).to(torch.int32).reshape(-1)
    else:
        names = list(dict.fromkeys(cameras))
        pos = {c: i for i, c in enumerate(names)}
        idx = torch.tensor([pos[c] for c in cameras], dtype=torch.int32, device=dev)
    if idx.shape[0] != n:
        raise RuntimeError("fit_filter: %d cameras for %d objects" % (idx.shape[0], n))
    return _camera_matrices(hg, names, dev) + (idx.contiguous(),)


def _repeat_cameras(cameras, k):
    """One camera per object -> one per (object, frame), frames innermost."""
    if isinstance(cameras, str):
        return cameras
    if isinstance(cameras, tuple) and len(cameras) == 2 and not isinstance(cameras[1], str):
        return cameras[0], torch.as_tensor(cameras[1]).reshape(-1).repeat_interleave(k)
    return [c for c in cameras for _ in range(k)]


def _heights(hg, classes, n, dev):
    if isinstance(classes, torch.Tensor) and classes.is_floating_point():
        h = classes.to(dev).float().reshape(-1)
    else:
        cl = classes.reshape(-1).tolist() if isinstance(classes, (torch.Tensor, np.ndarray)) else list(classes)
        cl = [c if isinstance(c, str) else CLASS_NAMES[int(c)] for c in cl]
        h = hg.guess_heights(cl).to(dev).float()
    if h.shape[0] != n:
        raise RuntimeError("fit_filter: %d classes for %d objects" % (h.shape[0], n))
    return h


def _im_height(b):
    """The image height of homography.py:540-547: |mean(top) - mean(bottom)| summed over x and y, in b's dtype.  The
    reference writes sqrt(pow(d, 2)); with a correctly rounded square root that is |d| bit for bit."""
    top = (((b[:, 4] + b[:, 5]) + b[:, 6]) + b[:, 7]) / 4
    bottom = (((b[:, 0] + b[:, 1]) + b[:, 2]) + b[:, 3]) / 4
    d = (top - bottom).abs()
    return d[:, 0] + d[:, 1]


def gt_states(hg, gt_im, classes, cameras):
    """The two-pass conversion of fit_filter_3D.py:262-266 (and :325-329, :349-354): image corners [n,8,2] -> states
    [n,6] fp32 with the guessed heights, back to the image, height_from_template (homography.py:519-551) of the
    reprojection against the boxes themselves, and to states again with the refined heights.  Device tensor."""
    dev = _device(gt_im)
    im = torch.as_tensor(gt_im).to(dev)
    n = im.shape[0]
    if n == 0:
        return torch.zeros((0, 6), dtype=torch.float32, device=dev)
    H1, H2, P1, P2, idx = _cameras(hg, cameras, n, dev)
    h0 = _heights(hg, classes, n, dev)
    temp = _ops.hg_from_im(im, h0, H1, H2, idx, to_state=True)                 # :263
    repro = _ops.hg_to_im(temp, P1, P2, idx, from_state=True)                  # :264, fp64
    refined = _im_height(im) / (_im_height(repro) / h0)                        # :265
    return _ops.hg_from_im(im, refined, H1, H2, idx, to_state=True)            # :266


def _moments(E):
    mean, cov, _ = _ops.residual_moments(E)
    return mean, cov


def tracklet_states(hg, tracklets_im, classes, cameras):
    """[n,f,8,2] image corners of n objects over f frames -> [n,f,6] states (gt_states on every frame); classes one per
    object (or per object and frame), cameras one per object."""
    dev = _device(tracklets_im)
    tr = torch.as_tensor(tracklets_im).to(dev)
    if tr.dim() != 4 or tuple(tr.shape[2:]) != (8, 2):
        raise RuntimeError("fit_filter: tracklets are [n,f,8,2] image corners, got %s" % (tuple(tr.shape),))
    n, f = tr.shape[0], tr.shape[1]
    if isinstance(classes, (torch.Tensor, np.ndarray)):
        cl = torch.as_tensor(classes)
        cl = (cl.reshape(n, 1).expand(n, f) if cl.numel() == n else cl.reshape(n, f)).reshape(-1)
    else:
        cl = list(classes)
        per_object = len(cl) == n and not isinstance(cl[0], (list, tuple))
        cl = [c for c in cl for _ in range(f)] if per_object else [c for row in cl for c in row]
    return gt_states(hg, tr.reshape(n * f, 8, 2), cl, _repeat_cameras(cameras, f)).reshape(n, f, 6)


def q_errors(hg, kf_params, tracklets_im, classes, cameras, states=None):
    """The rows of fit_Q before the moments: -> (error [n,6], prediction [n,6], target [n,6]) fp32 device tensors.
    ``states`` [n,3,6] = tracklet_states(...) already computed."""
    s = tracklet_states(hg, tracklets_im, classes, cameras) if states is None else states
    if s.shape[1] < 3:
        raise RuntimeError("fit_Q needs three frames per tracklet, got %d" % s.shape[1])
    dev, n = s.device, s.shape[0]
    vel = (s[:, 1, 0] - s[:, 0, 0]) * FPS                                      # :270
    init = torch.cat((s[:, 0, :5], vel[:, None]), dim=1)                       # :271
    kf = Torch_KF(dev, INIT=kf_params)                                         # :243
    kf.add(init, list(range(n)), s[:, 0, 5].clone(), torch.zeros(n, dtype=torch.float64, device=dev))   # :273
    kf.predict()                                                               # :281
    vel2 = (s[:, 2, 0] - s[:, 1, 0]) * FPS                                     # :275
    target = torch.cat((s[:, 1, :5], vel2[:, None]), dim=1)                    # :276
    return kf.X - target, kf.X, target                                         # :289


def fit_Q(hg, kf_params, tracklets_im, classes, cameras, states=None):
    """fit_filter_3D.py:242-304: the model error of one prediction step.  tracklets_im [n,3,8,2]: three consecutive
    frames of n objects; classes one per object (or per object and frame).  States of frames 0..2, speeds by finite
    differences x 30; every object enters a ``Torch_KF(INIT=kf_params)`` at frame 0 with the first speed, one
    ``predict()``, and the error against frame 1 with the second speed.  -> (mu_Q [6], Q [6,6]) fp32 on the device.

    The reference adds four rows per iteration to one growing filter and predicts all of it every time, but reads back
    only the newest four rows (``kf.objs()`` by id, ids 0..3 reused).  ``predict`` treats every row on its own, so the
    rows it reads have seen exactly one step: one batched add and one predict is the same computation."""
    err, _, _ = q_errors(hg, kf_params, tracklets_im, classes, cameras, states=states)
    return _moments(err)


def _detect(detector, frames):
    """The detector in eval mode on one frame at a time (:340-342) -> (scores, labels, boxes20, offsets)."""
    detector.eval()
    sc, lb, bx, off = [], [], [], [0]
    with torch.no_grad():
        for f in frames:
            s, l, b = detector(f)
            sc.append(s.reshape(-1)), lb.append(l.reshape(-1)), bx.append(b.reshape(-1, 20))
            off.append(off[-1] + int(s.numel()))
    return torch.cat(sc), torch.cat(lb), torch.cat(bx), torch.tensor(off, dtype=torch.int32)


def r_errors(hg, detector, frames, gt_im, classes, cameras, detections=None):
    """The rows of fit_R before the moments: -> (resid [B,5] compacted, rows int32 [B], info int32 [3], gt_state [B,6],
    det_state [D,6]) device tensors; info = (matched, empty, unmatchable) frames."""
    dev = _device(gt_im, frames)
    gt = torch.as_tensor(gt_im).to(dev)
    B = gt.shape[0]
    gt = gt.reshape(B, 8, 2)                                                   # [B,1,8,2]: one ground-truth box per frame
    if detections is None:
        detections = _detect(detector, frames)
    scores, labels, boxes20, offsets = detections
    offsets = torch.as_tensor(offsets).to(torch.int64).reshape(-1)
    if offsets.shape[0] != B + 1:
        raise RuntimeError("fit_R: %d offsets for %d frames" % (offsets.shape[0], B))
    gt_state = gt_states(hg, gt, classes, cameras)                             # :325-329
    det_im = torch.as_tensor(boxes20).to(dev).reshape(-1, 10, 2)[:, :8, :]     # :347-348, the 2D box dropped
    D = det_im.shape[0]
    per_frame = (offsets[1:] - offsets[:-1]).cpu()
    if isinstance(cameras, str):
        det_cams = cameras
    elif isinstance(cameras, tuple) and len(cameras) == 2 and not isinstance(cameras[1], str):
        det_cams = (cameras[0], torch.as_tensor(cameras[1]).reshape(-1).cpu().repeat_interleave(per_frame))
    else:
        det_cams = [c for c, k in zip(cameras, per_frame.tolist()) for _ in range(k)]
    det_state = gt_states(hg, det_im, torch.as_tensor(labels).reshape(-1).long(), det_cams)   # :349-354
    rows, resid, info = _ops.fit_nearest(gt_state, det_state, offsets.to(dev))                # :356-375
    return resid, rows, info, gt_state, det_state


def fit_R(hg, detector, frames, gt_im, classes, cameras, detections=None):
    """fit_filter_3D.py:306-389: the measurement error of the detector.  frames: B images for ``detector`` (eval mode,
    one frame per call, -> scores, labels, boxes [d,20]); gt_im [B,1,8,2] with one class and one camera per frame.
    ``detections`` = (scores [D], labels [D], boxes20 [D,20], offsets [B+1]) precomputed replaces the detector.  Each
    frame's detections lose their 2D box, become states by the two-pass conversion, and the one nearest to the
    ground truth (``rn_fit_nearest``) gives the residual.  -> (mu_R [5], R [5,5], n_empty, n_unmatchable); frames
    without detections are skipped as the script does, frames in which no box compares (the script would stop on
    ``None - gt_state``) are skipped and counted.  One device -> host copy (the three counts)."""
    resid, _, info, _, _ = r_errors(hg, detector, frames, gt_im, classes, cameras, detections)
    matched, empty, bad = (int(x) for x in info.cpu())
    mean, cov = _moments(resid[:matched])
    return mean, cov, empty, bad


def fit_class_sizes(states, class_ids, class_names=CLASS_NAMES):
    """fit_filter_3D.py:423-441: per class the mean (l, w, h) and its covariance.  states [n,6], class_ids [n] integer
    -> (class_size, class_covariance) dicts keyed by class name, for the classes that occur."""
    dev = _device(states)
    st = torch.as_tensor(states).to(dev).float()
    ids = torch.as_tensor(class_ids).to(dev).reshape(-1)
    mean, cov, count = _ops.residual_moments(st[:, 2:5].contiguous(), ids, len(class_names))
    count = count.cpu().tolist()
    sizes = {class_names[g]: mean[g].clone() for g in range(len(class_names)) if count[g] > 0}
    covs = {class_names[g]: cov[g].clone() for g in range(len(class_names)) if count[g] > 0}
    return sizes, covs


def fit_speed(states_first, states_last, n_frames):
    """fit_filter_3D.py:468-478: |x_last - x_first| / ((n_frames - 1) / 30.0) per tracklet -> (mu_v [1], var [1,1])."""
    dev = _device(states_first, states_last)
    a, b = torch.as_tensor(states_first).to(dev).float(), torch.as_tensor(states_last).to(dev).float()
    # a device tensor as the divisor: torch divides by it; a Python number may be turned into a multiplication by its
    # reciprocal on the device, which is not the reference's rounding
    span = torch.tensor((n_frames - 1) / 30.0, dtype=torch.float32, device=dev)
    vel = torch.abs(b[:, 0] - a[:, 0]) / span                                  # :468
    return _moments(vel[:, None].contiguous())


def fit(hg, kf_params, tracklets_im, tracklet_classes, tracklet_cameras, detector, frames, gt_im, gt_classes,
        frame_cameras, detections=None, device_out=False):
    """The four cells in the script's order on one set of tracklets [n,3,8,2] (Q, class sizes, speed) and one set of
    detector frames (R).  -> a new dict: ``kf_params`` with ``mu_Q``, ``Q``, ``mu_R``, ``R``, ``class_size``,
    ``class_covariance``, ``mu_v`` [1] and ``P`` = zeros(6,6) with P[:5,:5] = R and P[5,5] = var(v) (:482-485), fp32
    CPU tensors as the reference pickles them (device_out=True leaves them on the device); ``Torch_KF(INIT=...)``
    takes it unchanged.  The counts of skipped frames are returned beside it: (kf_params, n_empty, n_unmatchable)."""
    dev = _device(tracklets_im, gt_im)
    out = dict(kf_params)
    s = tracklet_states(hg, tracklets_im, tracklet_classes, tracklet_cameras)
    n, f = s.shape[0], s.shape[1]
    out["mu_Q"], out["Q"] = fit_Q(hg, kf_params, tracklets_im, tracklet_classes, tracklet_cameras, states=s)
    out["mu_R"], out["R"], empty, bad = fit_R(hg, detector, frames, gt_im, gt_classes, frame_cameras, detections)
    cl = tracklet_classes
    if not (isinstance(cl, torch.Tensor) and not cl.is_floating_point()):
        cl = torch.tensor([CLASS_NAMES.index(c) if isinstance(c, str) else int(c) for c in
                           (row[0] if isinstance(row, (list, tuple)) else row for row in cl)])
    cl = cl.reshape(n, -1)[:, 0]                                               # the tracklet's first class keys it (:408)
    out["class_size"], out["class_covariance"] = fit_class_sizes(s.reshape(n * f, 6), cl.repeat_interleave(f))   # :426
    out["mu_v"], var_v = fit_speed(s[:, 0], s[:, -1], f)
    P = torch.zeros([6, 6], dtype=torch.float32, device=dev)                   # :482
    P[:5, :5] = out["R"]                                                       # :484
    P[5, 5] = var_v[0, 0]                                                      # :485
    out["P"] = P
    if not device_out:
        def host(v):
            if isinstance(v, dict):
                return {k: host(x) for k, x in v.items()}
            return v.cpu() if isinstance(v, torch.Tensor) else v
        out = {k: host(v) for k, v in out.items()}
    return out, empty, bad

"""The scores the reference's later annotator (``manual_annotator_state_v3.py``) judges an adjusted label set by, on the GPU:
``calculate_total_variation`` (:3843-3889), ``calculate_feasibility`` (:3891-3979), ``annotator_rmse`` (:3981-4007), the data half
of ``plot_trajectories_unified`` (:3634-3711) as ``kinematics``, and the "Summary of metrics" block (:4349-4354) for one
annotator as ``quality_report``.

The functions take the annotator as ``ann`` like the module-level functions they replace and read the same attributes --
``data``, ``cameras``, for ``annotator_rmse`` also ``hg`` -- so a maintainer calls them in place of the reference's, binds them
into the class::

    import label_quality
    for name in label_quality.METHODS:
        setattr(Annotator, name, getattr(label_quality, name))

or inherits ``LabelQuality``.  The reference runs every score as a Python loop over objects x cameras x ALL frames with one
string-formatted dict lookup per step.  Here ``label_audit.pack_tracklets`` packs the label set once, one copy sends the table
to the device and ``ops.label_series`` (csrc/label_quality.hip) does the rest in one launch, one workgroup per object: the
optional lane filter, the sort of the object's boxes from all cameras by (timestamp, position) -- a bitonic network in LDS, the
same network on a global workspace for an object of more than 4096 boxes -- the 0.01 s keep rule, the compaction, v, vy, a,
theta, the range, the variation and the count of feasible segments.  ``ops.label_group_rmse`` reduces the projected boxes of
``annotator_rmse``, which ``ops.hg_to_im`` projects.  The kernels' fp64 arithmetic rounds once per operation in the reference's
order and sums in ascending order, so every number but theta (atan2) and the RMSE (torch.mean's summation order) equals the
reference's bit for bit (``tests/golden/label_quality.npz``).  There is no CPU path: without a device every function raises.

Reference behaviour kept on purpose: only ids below ``get_unused_id()`` are visited; a row is dropped when it follows the
previous SORTED row -- kept or not -- by less than 0.01 s (:3875-3878); ``v`` is negated (:3947), so an object that drives
towards larger x has negative speeds and no feasible segment, and one that stands still has ``v = -0.0`` and fails the strict
``> 0``; the feasibility mask is ``np.logical_and(tmask, vmask, amask)`` (:3975), whose third argument is numpy's ``out=``: the
acceleration mask is overwritten and acceleration does NOT enter the result; ``annotator_rmse`` projects a whole group through
the camera of the LAST box it appended (:3992), ignores trailing ids beyond a multiple of five and returns the root of the mean
of the groups' RMSEs (:4006), a root of a mean of roots.

Differences a caller can see: the variation of an object with a single kept row is ``np.float64(0.0)`` (the
reference: the int ``0``); ``annotator_rmse`` returns ``(rmse, per-group rmse)`` (the reference returns None) and raises
ValueError before any device work for fewer than five ids or an empty group (the reference: ZeroDivisionError / RuntimeError
from ``torch.stack([])``); boxes of one object with exactly equal timestamps are ordered camera first, then frame (the
reference's ``np.argsort`` leaves them unordered); ``kinematics(lane=None)`` applies no lane filter (the reference's default is
``[82, 98]``), returns the series instead of drawing them and raises NotImplementedError for ``smooth != 1`` or ``plot=True``;
packing refuses what ``pack_tracklets`` refuses.
"""
import math

import numpy as np

from datareader import _download, _upload
from label_audit import _device, _is_index, _names, estimate_projection_error, get_unused_id, pack_tracklets  # noqa: F401
from label_rewrite import _P_table, _sides
from retinanet_mi355x import ops

METHODS = ("calculate_total_variation", "calculate_feasibility", "kinematics", "annotator_rmse", "quality_report")
GROUP = 5                                                      # :3993
STATE_KEYS = ("x", "y", "l", "w", "h", "direction")


def label_series(ann, lane=None, lds_rows=None, tab=None):
    """``ops.label_series`` on the label set (or on ``tab``, a ``pack_tracklets`` table of it) -> dict on the host: tab, first
    (the first row of every object), order, keep, series fp64 [7, R] = (t, x, y, v, vy, a, theta), counts int32 [n_ids, 3] =
    (n, m, feasible segments), figs fp64 [n_ids, 2] = (range, variation)."""
    if tab is None:
        tab = pack_tracklets(ann.data, _names(ann))
    dev = _device(ann)
    C, n_ids = tab["n_cam"], len(tab["ids"])
    if C == 0 or n_ids == 0:
        return dict(tab=tab, first=np.zeros(0, np.int64), order=np.zeros(0, np.int32), keep=np.zeros(0, np.uint8),
                    series=np.zeros((ops.LABEL_SERIES_PLANES, 0)), counts=np.zeros((0, 3), np.int32), figs=np.zeros((0, 2)))
    d_off, d_cols = _upload(dev, [tab["offsets"], tab["cols"]])
    order, keep, series, counts, figs, status = ops.label_series(d_off, d_cols, C, lane, lds_rows)
    h_status, h_order, h_keep, h_series, h_counts, h_figs = _download([status, order, keep, series, counts, figs])
    ops.label_check(int(h_status[0]))
    return dict(tab=tab, first=tab["offsets"][:-1:C], order=h_order, keep=h_keep, series=h_series, counts=h_counts, figs=h_figs)


def calculate_total_variation(ann, verbose=True, _series=None):
    """:3843-3889 -> (x_var, x_range): per object below ``get_unused_id()`` the summed |step| of x along its time-sorted kept
    boxes and max(x) - min(x), lists of np.float64 in id order."""
    got = label_series(ann) if _series is None else _series
    x_range, x_var = list(got["figs"][:, 0]), list(got["figs"][:, 1])
    if verbose:
        print("Total vs True variation: {}/{}   ({}x)".format(sum(x_var), sum(x_range), sum(x_var) / sum(x_range)))
    return x_var, x_range


def calculate_feasibility(ann, _series=None):
    """:3891-3979 -> per object with more than one kept box the fraction of its segments whose v lies in (0, 140) and whose
    theta in (-25, 25) at both ends (acceleration does not enter, as in the reference)."""
    got = label_series(ann) if _series is None else _series
    f_percentage = []
    for n, m, feasible in got["counts"].tolist():
        if m > 1:
            f_percentage.append(np.float64(feasible) / (m - 1))
    return f_percentage


def kinematics(ann, lane=None, smooth=1, plot=False):
    """The data half of plot_trajectories_unified (:3634-3711) -> per object with more than one kept box a dict: id, time, x, y,
    v, a, theta (np.float64 arrays) and length (``l`` of the last box of the object that passed the lane filter, cameras in
    order, frames ascending).  ``lane``: (lo, hi), only boxes with lo < y < hi; None: all."""
    if smooth != 1 or plot:
        raise NotImplementedError("kinematics returns the series of plot_trajectories_unified for smooth = 1 (np.hamming(1) is "
                                  "[1.]); smoothing and drawing are not part of this port")
    got = label_series(ann, lane)
    tab, ser, out = got["tab"], got["series"], []
    for j, (n, m, _) in enumerate(got["counts"].tolist()):
        if m > 1:
            s0 = int(got["first"][j])
            t, x, y, v, _, a, theta = (ser[p, s0:s0 + m].copy() for p in range(ops.LABEL_SERIES_PLANES))
            last = int(got["order"][s0:s0 + n].max())
            out.append(dict(id=tab["ids"][j], time=t, x=x, y=y, v=v, a=a, theta=theta, length=tab["items"][last]["l"]))
    return out


def _rmse_groups(ann):
    """:3987-3994 -> per group of five ids its boxes, in id, frame, dict order; ValueError where the reference fails."""
    n_ids = get_unused_id(ann)
    if n_ids < GROUP:
        raise ValueError("annotator_rmse needs at least five ids (0..4 label one object): the label set has {}".format(n_ids))
    by_id = [[] for _ in range(n_ids // GROUP * GROUP)]
    for frame_data in ann.data:
        for obj in frame_data.values():
            i = obj["id"]
            if _is_index(i) and 0 <= i < len(by_id):
                by_id[i].append(obj)
    groups = [[o for objs in by_id[g * GROUP:(g + 1) * GROUP] for o in objs] for g in range(n_ids // GROUP)]
    for g, boxes in enumerate(groups):                          # cannot happen below the first unused id; kept as a guard
        if not boxes:
            raise ValueError("annotator_rmse: ids {}..{} have no box".format(g * GROUP, g * GROUP + GROUP - 1))
    return groups


def annotator_rmse(ann, verbose=True):
    """:3981-4007 -> (rmse, per-group rmse): ids 5k .. 5k+4 are annotations of one object; per group the root mean squared
    distance of the boxes' rear bottom centres in the image of the camera of the group's LAST box from their mean; overall the
    root of the mean of the groups' values."""
    groups = _rmse_groups(ann)
    names = _names(ann)
    index = {n: c for c, n in reversed(list(enumerate(names)))}
    state = np.array([[float(o[k]) for k in STATE_KEYS] for boxes in groups for o in boxes], np.float64).astype(np.float32)
    group = np.repeat(np.arange(len(groups), dtype=np.int32), [len(b) for b in groups])
    cams = [index[boxes[-1]["camera"]] for boxes in groups]     # :3992
    cam = np.repeat(np.array(cams, np.int32), [len(b) for b in groups])
    hg1, hg2 = _sides(ann.hg)
    used = {names[c] for c in cams}
    tables = [_P_table(hg1, names, used)] + ([] if hg2 is None else [_P_table(hg2, names, used)])
    dev = _device(ann)                                          # every refusal above comes before any GPU work
    up = _upload(dev, [state, group, cam] + tables)
    P1 = up[3].reshape(-1, 3, 4)
    P2 = up[4].reshape(-1, 3, 4) if hg2 is not None else None
    im = ops.hg_to_im(up[0], P1, P2, up[2], from_state=True)
    rmse, _, _, status = ops.label_group_rmse(im, up[1], len(groups))
    h_status, h_rmse = _download([status, rmse])
    ops.label_check(int(h_status[0]))
    mses = list(h_rmse)
    total = np.float64(math.sqrt(sum(mses) / len(mses)))        # :4006
    if verbose:
        print("RMSE: {}".format(total))
    return total, mses


def quality_report(ann, reverse_curve_offset=False, verbose=True):
    """The "Summary of metrics" block (:4349-4354) for one annotator -> dict: ccde_x, ccde_y (the means of
    ``label_audit.estimate_projection_error``), v_total = sum(variation) / sum(range), feasible = the mean feasible fraction,
    and the lists they were formed from (x_error, y_error, x_var, x_range, f_percent).  The variation and the feasibility share
    one packed table and one launch; ``estimate_projection_error`` packs for itself (it takes no table)."""
    x_error, y_error = estimate_projection_error(ann, reverse_curve_offset=reverse_curve_offset)
    got = label_series(ann)
    x_var, x_range = calculate_total_variation(ann, verbose=verbose, _series=got)
    f_percent = calculate_feasibility(ann, _series=got)

    def ratio(num, den):
        return num / den if den else float("nan")
    rep = dict(ccde_x=ratio(sum(x_error), len(x_error)), ccde_y=ratio(sum(y_error), len(y_error)),
               v_total=ratio(sum(x_var), sum(x_range)), feasible=ratio(sum(f_percent), len(f_percent)),
               x_error=x_error, y_error=y_error, x_var=x_var, x_range=x_range, f_percent=f_percent)
    if verbose:
        print("Summary of metrics:")
        print("CCDE x: {}".format(rep["ccde_x"]))
        print("CCDE y: {}".format(rep["ccde_y"]))
        print("V total: {}".format(rep["v_total"]))
        print("Percent feasible: {}".format(rep["feasible"]))
    return rep


class LabelQuality():
    """The functions above as methods: inherit it beside (or assign its members into) the reference's ``Annotator``."""
    calculate_total_variation = calculate_total_variation
    calculate_feasibility = calculate_feasibility
    kinematics = kinematics
    annotator_rmse = annotator_rmse
    quality_report = quality_report

"""Fixed-interval smoothing of tracking output: every row the tracker writes is its forward filter's posterior at that frame, so
it uses only the past -- the first rows of a track carry the large initial covariance, a bad association stays in the file as a
jump, the speed lags the positions, and where ``stitch`` filled a gap a noise-free cubic meets noisy rows.  ``smooth_tracks(data,
kf_params, params=None, device=None)`` takes ``Data_Reader.data`` and the parameters ``fit_filter.fit`` fits, and returns
``(new_data, report)``: the same rows with x, y, l, w, h, v replaced by the means of a Rauch-Tung-Striebel smoother that uses every
row of a track, past and future, and treats a row whose innovation fails a chi-square gate as missing.  This goes beyond the
reference.

Model (csrc/smooth.hip; tests/smooth_cases.py restates both passes; DESIGN.md "Fixed-interval smoothing" has the rationale): state
(x, y, l, w, h, v); the measurement of a row is its own (x, y, l, w, h), so H = [I5 | 0] is fixed and ``kf_params["H"]`` is not
read; x advances by d dt v with d the sign of the tracklet's summed directions (``track_stitch.bounds``' rule); Qk = q_scale Q dt /
dt_default, the tracker's scaling; R = r_scale R; the first row starts from its own fields with covariance ``kf_params["P"]``;
``mu_Q`` and ``mu_R`` are ignored, as the tracker ignores them by default.
  host   track_stitch.pack_tracklets: a tracklet = all rows of one id, rows in frame order -- ONE packed upload
  1      ops.smooth_filter   forward: predict, innovation, gate, Joseph-form update
  2      ops.smooth_rts      backward: the smoothed means and variances
  host   ONE copy back; every datum is copied with its six fields replaced.
There is no CPU path.  A NaN or infinite field, a repeated time stamp inside a track or a covariance that is not positive
definite raises RuntimeError and nothing is replaced.
"""
import numpy as np
import torch

from retinanet_mi355x import ops
import track_stitch

DEFAULTS = {"gate": 20.515, "q_scale": 1.0, "r_scale": 1.0, "dt_default": 1 / 30}     # gate: chi-square(5) at 0.999; 0 switches it off
FIELDS = track_stitch.FIELDS


def resolve_params(params=None):
    """DEFAULTS overridden by ``params`` as floats; ValueError on an unknown key, a negative or infinite gate or a non-positive
    scale or dt_default."""
    out = dict(DEFAULTS)
    for key, value in (params or {}).items():
        if key not in DEFAULTS:
            raise ValueError("unknown smoothing parameter %r (known: %s)" % (key, ", ".join(DEFAULTS)))
        out[key] = value
    out = {k: float(v) for k, v in out.items()}
    if not 0 <= out["gate"] < float("inf"):
        raise ValueError("gate is 0 (off) or a positive finite number, got %r" % out["gate"])
    for key in ("q_scale", "r_scale", "dt_default"):
        if not 0 < out[key] < float("inf"):
            raise ValueError("%s must be a positive finite number, got %r" % (key, out[key]))
    return out


def lane_order(offsets):
    """The stable argsort of descending tracklet length, int32 [N]: the lanes of a wave finish together."""
    return np.argsort(-np.diff(np.asarray(offsets, np.int64)), kind="stable").astype(np.int32)


def smooth_packed(offsets, cols, direction, model, params, device=None):
    """The device half: host arrays in, host arrays out.  One upload, two launches, one copy back -> dict(status, filt, nis, flag,
    out)."""
    import datareader
    dev = datareader._cuda(device)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    d_off, d_order, d_cols, d_dir, d_model = datareader._upload(dev, [offsets, lane_order(offsets), np.asarray(cols, np.float64).reshape(-1, 7),
                                                                      np.asarray(direction, np.int32).reshape(-1),
                                                                      np.asarray(model, np.float64).reshape(-1)])
    with torch.cuda.device(dev):
        filt, nis, flag, status = ops.smooth_filter(d_off, d_order, d_cols, d_dir, d_model, params["gate"], params["dt_default"])
        out, status = ops.smooth_rts(d_off, d_order, d_cols, d_dir, d_model, params["dt_default"], filt, status=status)
        host = dict(zip(("status", "filt", "nis", "flag", "out"), datareader._download([status, filt, nis, flag, out])))
    ops.smooth_check(int(host["status"][0]))
    return host


def _report(pk, host):
    N = len(pk["ids"])
    sums = np.add.reduceat(pk["direction"].astype(np.int64), pk["offsets"][:-1]) if N else np.zeros(0, np.int64)
    return dict(ids=pk["ids"], offsets=pk["offsets"], direction=np.where(sums >= 0, 1, -1).astype(np.int32), flag=host["flag"],
                nis=host["nis"], var=host["out"][:, 6:], filtered=host["filt"], status=int(host["status"][0]))


def rebuild(data, pk, out):
    """The host's last step -> new_data: every datum copied, x, y, l, w, h, v replaced by the smoothed means ``out[:, :6]`` of its
    packed row as Python floats; the id, the time stamp and everything else untouched."""
    row_of = [{} for _ in data]                                    # per frame: dict key -> packed row
    offsets, frame_of = pk["offsets"], pk["frame"].tolist()
    for i, key in enumerate(pk["ids"].tolist()):
        for r in range(int(offsets[i]), int(offsets[i + 1])):
            row_of[frame_of[r]][key] = r
    values = np.asarray(out)[:, :6].tolist()                       # Python floats
    new_data = []
    for f, frame in enumerate(data):
        fresh = {}
        for key, item in frame.items():                            # the frame's own order
            item = item.copy()
            item.update(zip(FIELDS, values[row_of[f][key]]))
            fresh[key] = item
        new_data.append(fresh)
    return new_data


def smooth_tracks(data, kf_params, params=None, device=None):
    """-> (new_data, report).  ``report``: ``ids`` (the tracklet ids, ascending), ``offsets`` int64 [N+1] into the packed rows,
    ``direction`` int32 [N] (+1 / -1), per packed row ``flag`` uint8 (1: the row failed the gate and was treated as missing), ``nis``
    (the innovation's chi-square, 0 at a first row), ``var`` [R,6] (the smoothed variances), ``filtered`` [R,27] (the forward
    filter's means and covariance triangle); ``status`` (0: anything else raised).  ``data`` is not modified."""
    import datareader
    params = resolve_params(params)
    model = ops.smooth_model(kf_params, params["q_scale"], params["r_scale"])
    pk = track_stitch.pack_tracklets(data)
    if len(pk["ids"]) == 0:
        datareader._cuda(device)
        empty = dict(status=np.zeros(1, np.int32), filt=np.zeros((0, ops.SMOOTH_FILT)), nis=np.zeros(0), flag=np.zeros(0, np.uint8),
                     out=np.zeros((0, ops.SMOOTH_OUT)))
        return [dict(frame) for frame in data], _report(pk, empty)
    host = smooth_packed(pk["offsets"], pk["cols"], pk["direction"], model, params, device)
    return rebuild(data, pk, host["out"]), _report(pk, host)

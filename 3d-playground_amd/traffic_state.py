"""Traffic state from tracking output: what ``stitch`` and ``smooth`` leave behind is a set of trajectories; this turns them into
traffic measures.  ``traffic_fields(data, params=None, device=None)`` gives Edie's generalised flow, density and space-mean speed
per direction and lane over a space-time grid; ``car_following(data, params=None, device=None)`` gives, for every vehicle at every
instant, its leader, space gap, time headway and time to collision.  Both take ``Data_Reader.data`` and leave it alone.  The
reference's annotator looks at its data the same way, lane by lane over time and x (``plot_one_lane``,
``plot_trajectories_unified``), but computes none of this: it goes beyond the reference.

Rules (csrc/traffic.hip; include/retinanet_mi355x.h states them, tests/traffic_cases.py restates them; DESIGN.md "Traffic state"
has the rationale):
  host   track_stitch.pack_tracklets: a tracklet = all rows of one id, rows in frame order -- ONE packed upload
  1      ops.traffic_lanes    the direction of every tracklet (the sign of its summed directions, ``track_stitch.bounds``' rule) and
                              the lane of every row: the k with edges[k] <= y < edges[k+1] under that direction, else -1
  2a     ops.traffic_cells    every segment (two consecutive rows of a tracklet, 0 < t_b - t_a <= max_gap, with a lane at its mean y)
                              is cut at the grid lines it crosses; each piece adds its time and distance to one cell as integers
                              in units of 1 / ops.TRAFFIC_Q, so the sums are exact and independent of the order of the atomics
  2b     ops.traffic_leaders  every frame as one instant: the nearest row ahead in the same direction and lane
  host   ONE copy back; density = T / (Q dx dt), flow = D / (Q dx dt), speed = D / T in fp64.
State x is the rear of a vehicle and its front is x + dir l (homography.i24_state_to_space), so gap = spacing - own length.
There is no CPU path.  A NaN or infinite field raises RuntimeError.
"""
import math

import numpy as np
import torch

from retinanet_mi355x import ops
import track_stitch

DEFAULTS = {"dx": 100.0, "dt": 5.0, "max_gap": 1.0, "x_range": None, "t_range": None,
            "lane_edges": {1: [0, 12, 24, 36, 48, 60], -1: [60, 72, 84, 96, 108, 120]}}     # a default, not a claim about a road


def _range(name, value):
    if value is None:
        return None
    lo, hi = (float(v) for v in value)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError("%s is None or (lo, hi) with lo < hi, both finite, got %r" % (name, value))
    return lo, hi


def resolve_params(params=None):
    """DEFAULTS overridden by ``params``; ValueError on an unknown key, a non-positive or infinite dx, dt or max_gap, a range that is
    not (lo, hi) with lo < hi, or lane edges that are not {1: [...], -1: [...]} with finite, strictly ascending entries (at most
    ops.TRAFFIC_MAX_EDGES each)."""
    out = dict(DEFAULTS)
    for key, value in (params or {}).items():
        if key not in DEFAULTS:
            raise ValueError("unknown traffic parameter %r (known: %s)" % (key, ", ".join(DEFAULTS)))
        out[key] = value
    for key in ("dx", "dt", "max_gap"):
        out[key] = float(out[key])
        if not 0 < out[key] < float("inf"):
            raise ValueError("%s must be a positive finite number, got %r" % (key, out[key]))
    out["x_range"], out["t_range"] = _range("x_range", out["x_range"]), _range("t_range", out["t_range"])
    edges = out["lane_edges"]
    if not isinstance(edges, dict) or set(edges) != {1, -1}:
        raise ValueError("lane_edges is {1: [...], -1: [...]}, got %r" % (edges,))
    fixed = {}
    for sgn in (1, -1):
        e = np.asarray(edges[sgn], np.float64).reshape(-1)
        if len(e) > ops.TRAFFIC_MAX_EDGES or not np.isfinite(e).all() or not (np.diff(e) > 0).all():
            raise ValueError("lane_edges[%d] holds at most %d finite, strictly ascending values, got %r" % (sgn, ops.TRAFFIC_MAX_EDGES, edges[sgn]))
        fixed[sgn] = e
    out["lane_edges"] = fixed
    return out


def _axis(values, step, explicit):
    """-> (origin, cells): the explicit range from lo in ceil((hi - lo) / step) cells, else the origin floored to a multiple of the
    step and as many cells as put the maximum inside; (0.0, 0) without finite values."""
    if explicit is not None:
        return explicit[0], int(math.ceil((explicit[1] - explicit[0]) / step))
    values = values[np.isfinite(values)]                           # a NaN or an infinity is the kernels' to refuse
    if len(values) == 0:
        return 0.0, 0
    lo, hi = float(values.min()), float(values.max())
    origin = math.floor(lo / step) * step
    return origin, int(math.floor((hi - origin) / step)) + 1


def grid_of(cols, params):
    """The grid of the packed rows -> dict(t0, dt, nt, x0, dx, nx): x over all rows, t over the rows with a time stamp > 0 (the
    shipped files hold rows stamped -1)."""
    cols = np.asarray(cols, np.float64).reshape(-1, 7)
    x0, nx = _axis(cols[:, 1], params["dx"], params["x_range"])
    t0, nt = _axis(cols[:, 0][cols[:, 0] > 0], params["dt"], params["t_range"])
    return dict(t0=t0, dt=params["dt"], nt=nt, x0=x0, dx=params["dx"], nx=nx)


def frames_csr(frame, F):
    """The packed rows by frame: a stable argsort of the rows' frame indices -> (frame_off int64 [F+1], frame_rows int32 [R])."""
    frame = np.asarray(frame, np.int64).reshape(-1)
    off = np.zeros(F + 1, np.int64)
    np.cumsum(np.bincount(frame, minlength=F), out=off[1:])
    return off, np.argsort(frame, kind="stable").astype(np.int32)


def fields_packed(offsets, cols, direction, params, grid, device=None):
    """The device half of ``traffic_fields``: host arrays in, host arrays out.  One upload, two launches, one copy back -> dict(status,
    T, D, n, counters)."""
    import datareader
    dev = datareader._cuda(device)
    d_off, d_cols, d_dir, d_ep, d_en = datareader._upload(dev, [np.asarray(offsets, np.int64).reshape(-1), np.asarray(cols, np.float64).reshape(-1, 7),
                                                                np.asarray(direction, np.int32).reshape(-1), params["lane_edges"][1],
                                                                params["lane_edges"][-1]])
    with torch.cuda.device(dev):
        tdir, _, status = ops.traffic_lanes(d_off, d_cols, d_dir, d_ep, d_en)
        T, D, n, counters, status = ops.traffic_cells(d_off, d_cols, tdir, d_ep, d_en, grid["t0"], grid["dt"], grid["nt"], grid["x0"], grid["dx"],
                                                      grid["nx"], params["max_gap"], status=status)
        host = dict(zip(("status", "T", "D", "n", "counters"), datareader._download([status, T, D, n, counters])))
    ops.traffic_check(int(host["status"][0]))
    return host


def following_packed(offsets, cols, direction, frame_off, frame_rows, params, device=None):
    """The device half of ``car_following`` -> dict(status, dir, lane, leader, spacing, gap, headway, ttc, counters)."""
    import datareader
    dev = datareader._cuda(device)
    d_off, d_cols, d_dir, d_ep, d_en, d_foff, d_frows = datareader._upload(dev, [np.asarray(offsets, np.int64).reshape(-1),
                                                                                 np.asarray(cols, np.float64).reshape(-1, 7),
                                                                                 np.asarray(direction, np.int32).reshape(-1), params["lane_edges"][1],
                                                                                 params["lane_edges"][-1], np.asarray(frame_off, np.int64),
                                                                                 np.asarray(frame_rows, np.int32)])
    with torch.cuda.device(dev):
        tdir, lane, status = ops.traffic_lanes(d_off, d_cols, d_dir, d_ep, d_en)
        out = ops.traffic_leaders(d_off, d_cols, tdir, lane, d_foff, d_frows, status=status)
        names = ("status", "dir", "lane", "leader", "spacing", "gap", "headway", "ttc", "counters")
        host = dict(zip(names, datareader._download([out[6], tdir, lane] + list(out[:6]))))
    ops.traffic_check(int(host["status"][0]))
    return host


def traffic_fields(data, params=None, device=None):
    """-> dict: ``T``, ``D`` int64 [2,L,nt,nx] (time spent and distance travelled in units of 1 / ops.TRAFFIC_Q s or ft; index 0 of
    the first axis is direction +1, L = the lanes of the longer edge list) and ``n`` int32 (pieces); ``grid`` (t0, dt, nt, x0, dx,
    nx); ``counters`` (segments, used, skipped_gap, skipped_lane, pieces, outside); ``density`` = T / (Q dx dt) in veh/ft, ``flow`` =
    D / (Q dx dt) in veh/s, ``speed`` = D / T in ft/s (NaN where T == 0), formed on the host in fp64; ``lane_edges``.  ``data`` is
    not modified."""
    import datareader
    params = resolve_params(params)
    pk = track_stitch.pack_tracklets(data)
    grid = grid_of(pk["cols"], params)
    if len(pk["ids"]) == 0:
        datareader._cuda(device)
        shape = (2, max(len(params["lane_edges"][1]), len(params["lane_edges"][-1]), 1) - 1, grid["nt"], grid["nx"])
        host = dict(T=np.zeros(shape, np.int64), D=np.zeros(shape, np.int64), n=np.zeros(shape, np.int32),
                    counters=np.zeros(ops.TRAFFIC_COUNTERS, np.int64))
    else:
        host = fields_packed(pk["offsets"], pk["cols"], pk["direction"], params, grid, device)
    T, D = host["T"], host["D"]
    area = ops.TRAFFIC_Q * grid["dx"] * grid["dt"]
    with np.errstate(divide="ignore", invalid="ignore"):
        speed = np.where(T == 0, np.nan, D.astype(np.float64) / T.astype(np.float64))
    return dict(T=T, D=D, n=host["n"], grid=grid, counters={k: int(v) for k, v in zip(ops.TRAFFIC_CELL_COUNTERS, host["counters"])},
                density=T.astype(np.float64) / area, flow=D.astype(np.float64) / area, speed=speed, lane_edges=params["lane_edges"])


def car_following(data, params=None, device=None):
    """Every frame of ``data`` taken as one instant (meant for reinterpolated data) -> dict: ``ids`` (the tracklet ids, ascending),
    ``offsets`` int64 [N+1] into the packed rows, ``dir`` int32 [N]; per packed row ``frame``, ``lane`` int32 (-1: none), ``leader``
    (packed row, -1: none), ``leader_id`` int64 (the leader's dict key, -1: none), ``spacing`` (rear to rear), ``gap`` = spacing - own
    length, ``headway`` = spacing / v, ``ttc`` = gap / closing speed (fp64, inf where undefined or without a leader); ``with_leader``
    and ``overlaps`` (rows with gap < 0); ``frame_spread`` = the largest max - min time stamp inside a frame, which tells whether
    "one instant" holds.  ``data`` is not modified."""
    import datareader
    params = resolve_params(params)
    pk = track_stitch.pack_tracklets(data)
    R = len(pk["cols"])
    if len(pk["ids"]) == 0:
        datareader._cuda(device)
        host = dict(dir=np.zeros(0, np.int32), lane=np.zeros(0, np.int32), leader=np.zeros(0, np.int32), spacing=np.zeros(0), gap=np.zeros(0),
                    headway=np.zeros(0), ttc=np.zeros(0), counters=np.zeros(ops.TRAFFIC_COUNTERS, np.int64))
        spread = 0.0
    else:
        frame_off, frame_rows = frames_csr(pk["frame"], len(data))
        host = following_packed(pk["offsets"], pk["cols"], pk["direction"], frame_off, frame_rows, params, device)
        t, first = pk["cols"][frame_rows, 0], frame_off[:-1][np.diff(frame_off) > 0]
        spread = float((np.maximum.reduceat(t, first) - np.minimum.reduceat(t, first)).max())
    leader = host["leader"]
    owner = np.searchsorted(pk["offsets"], np.maximum(leader, 0), side="right") - 1
    leader_id = np.where(leader >= 0, pk["ids"][owner] if R else np.zeros(0, np.int64), -1).astype(np.int64)
    counters = dict(zip(ops.TRAFFIC_LEADER_COUNTERS, (int(v) for v in host["counters"])))
    return dict(ids=pk["ids"], offsets=pk["offsets"], frame=pk["frame"], lane=host["lane"], dir=host["dir"], leader=leader, leader_id=leader_id,
                spacing=host["spacing"], gap=host["gap"], headway=host["headway"], ttc=host["ttc"], with_leader=counters["with_leader"],
                overlaps=counters["overlaps"], frame_spread=spread)

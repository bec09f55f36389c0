"""Track stitching: join the fragments a vehicle leaves behind when the tracker loses it -- at an occlusion or a camera
hand-over -- and starts a new id when it reappears.  ``stitch_tracks(data, params=None, fill=True, device=None)`` takes
``Data_Reader.data`` (a list of ``{id: datum}`` dicts, one per unique rounded time stamp, ascending) and returns ``(new_data,
report)``: the same rows under one id per chain, and with ``fill`` the gap of every link filled at ``fill_rate``.  This goes
beyond the reference, whose ``reinterpolate`` only interpolates between adjacent frames that both hold the id.

Stages (csrc/stitch.hip; tests/stitch_cases.py restates each one; DESIGN.md "Track stitching" has the rationale):
  host   a tracklet = all rows of one id (the dict key), tracklets in ascending id, rows in frame order: offsets int64 [N+1],
         fp64 (t, x, y, l, w, h, v) and int32 direction per row -- ONE packed upload
  1      ops.stitch_endpoints   a line fit through the ``fit_n`` rows nearest each end: time, fitted x and slope, mean y, l, w, h
  2      ops.stitch_candidates  every ordered pair (a's tail -> b's head) of one direction: which tails and heads have a candidate
         ops.stitch_compact     ... and the matrix W = cost - max_cost over those only (the dense one is ops.stitch_costs)
  3      ops.stitch_assign      scipy's linear_sum_assignment per direction on one wave64; a link is an assigned cell with W < 0:
         the partial matching that maximises sum(max_cost - cost)
  4      ops.stitch_chains      root, rank and new id of every tracklet by pointer jumping
  5      ops.stitch_fill_count / stitch_fill_rows   the rows of every gap: x a cubic Hermite through the end rows with the fitted
         slopes, v its derivative, the others linear
  host   ONE copy back; the dict keys and ``datum["id"]`` are rewritten, the new rows go into the frame of their rounded time
         stamp or into a new frame, and ``data`` stays sorted.
There is no CPU path.  A NaN or infinite field raises RuntimeError and nothing is replaced.

Limits: ``ops.STITCH_MAX_TRACKLETS`` tracklets (raised before any launch); per direction at most ``ops.LSAP_MAX_MIN`` tails or
heads with a candidate, whichever is fewer -- that count exists only on the device, so it is raised after the run, from the
status word, and nothing is replaced.
"""
import numpy as np
import torch

from retinanet_mi355x import ops

DEFAULTS = {"fit_n": 8, "max_gap": 3.0, "back_tol": 5.0, "sigma_x0": 10.0, "sigma_x1": 10.0, "sigma_y": 4.0, "sigma_size": 10.0,
            "max_cost": 3.0, "fill_rate": 30.0}
COLS = ("timestamp", "x", "y", "l", "w", "h", "v")             # the packed fp64 columns
FIELDS = ("x", "y", "l", "w", "h", "v")                        # datareader.FIELDS: the order of the filled fields


def resolve_params(params=None):
    """DEFAULTS overridden by ``params``; ValueError on an unknown key, a fit_n outside 1 .. 64 or a non-positive scale
    (back_tol, a tolerance, may be 0)."""
    out = dict(DEFAULTS)
    for key, value in (params or {}).items():
        if key not in DEFAULTS:
            raise ValueError("unknown stitching parameter %r (known: %s)" % (key, ", ".join(DEFAULTS)))
        out[key] = value
    fit_n = out["fit_n"]
    if isinstance(fit_n, bool) or int(fit_n) != fit_n or not 1 <= int(fit_n) <= ops.STITCH_MAX_FIT:
        raise ValueError("fit_n is an integer in 1 .. %d, got %r" % (ops.STITCH_MAX_FIT, fit_n))
    out["fit_n"] = int(fit_n)
    scales = ops.stitch_scales([out[k] for k in ops.STITCH_SCALES])
    out.update(zip(ops.STITCH_SCALES, scales))
    out["fill_rate"] = float(out["fill_rate"])
    if not 0 < out["fill_rate"] < float("inf"):
        raise ValueError("fill_rate must be a positive finite number, got %r" % out["fill_rate"])
    return out


def scales_of(params):
    return [params[k] for k in ops.STITCH_SCALES]


def pack_tracklets(data):
    """``Data_Reader.data`` by tracklet: ids int64 [N] ascending (the dict keys), offsets int64 [N+1], cols fp64 [R,7] in COLS
    order, direction int32 [R], and per packed row its datum (``rows``) and frame index (``frame``)."""
    by_id = {}
    for f, frame in enumerate(data):
        for key, item in frame.items():
            by_id.setdefault(key, []).append((f, item))
    ids = sorted(by_id)
    offsets, rows, frames = [0], [], []
    for key in ids:
        for f, item in by_id[key]:
            rows.append(item)
            frames.append(f)
        offsets.append(len(rows))
    cols = np.array([[item[k] for k in COLS] for item in rows], np.float64).reshape(-1, 7)
    direction = np.array([item["direction"] for item in rows], np.int64).reshape(-1)
    if len(direction) and (np.abs(direction) >= 2 ** 31).any():
        raise ValueError("a direction does not fit int32")
    return dict(ids=np.asarray(ids, np.int64).reshape(-1), offsets=np.asarray(offsets, np.int64), cols=cols,
                direction=direction.astype(np.int32), rows=rows, frame=np.asarray(frames, np.int64))


def bounds(offsets, direction, params, fill=True):
    """What the host can know before the run -> (cap = the cells of both compressed matrices at most, U = the new rows at most)."""
    N = len(offsets) - 1
    if N > ops.STITCH_MAX_TRACKLETS:
        raise RuntimeError("stitching takes at most %d tracklets, got %d" % (ops.STITCH_MAX_TRACKLETS, N))
    if N == 0:
        return 0, 0
    sums = np.add.reduceat(np.asarray(direction, np.int64), offsets[:-1]) if len(direction) else np.zeros(N, np.int64)
    plus = int((sums >= 0).sum())
    cap = plus * plus + (N - plus) * (N - plus)
    if not fill:
        return cap, 0
    per = params["max_gap"] * params["fill_rate"] + 1.0            # rows of one link: k < g * rate <= max_gap * rate
    if not per < ops.STITCH_MAX_FILL:
        raise ValueError("max_gap * fill_rate allows %g new rows per link, the limit is %d" % (per, ops.STITCH_MAX_FILL))
    links = N - (1 if plus in (0, N) else 2)                       # a chain of n tracklets holds n - 1 links
    return cap, max(links, 0) * (int(per) + 1)


def stitch_packed(ids, offsets, cols, direction, params, fill=True, device=None):
    """The device half: host arrays in, host arrays out.  One upload, the stages, one copy back -> dict(status, ep, ncand, next,
    prev, link_cost, root, rank, new_id and, with fill, count, prefix, fields, time, link, side)."""
    import datareader
    dev = datareader._cuda(device)
    cap, U = bounds(offsets, direction, params, fill)
    scales = scales_of(params)
    d_ids, d_off, d_cols, d_dir = datareader._upload(dev, [np.asarray(ids, np.int64).reshape(-1), np.asarray(offsets, np.int64).reshape(-1),
                                                           np.asarray(cols, np.float64).reshape(-1, 7),
                                                           np.asarray(direction, np.int32).reshape(-1)])
    with torch.cuda.device(dev):
        ep, status = ops.stitch_endpoints(d_off, d_cols, d_dir, params["fit_n"])
        cand, ncand = ops.stitch_candidates(ep, scales)
        Wc, status = ops.stitch_compact(ep, scales, cand, ncand, cap, status=status)
        nxt, prev, link_cost, status = ops.stitch_assign(ep, scales, cand, ncand, Wc, status=status)
        root, rank, new_id, status = ops.stitch_chains(prev, d_ids, status=status)
        names = ["status", "ep", "ncand", "next", "prev", "link_cost", "root", "rank", "new_id"]
        out = [status, ep, ncand, nxt, prev, link_cost, root, rank, new_id]
        if fill:
            count, prefix, status = ops.stitch_fill_count(ep, nxt, params["fill_rate"], status=status)
            rows = ops.stitch_fill_rows(ep, nxt, prefix, params["fill_rate"], U, status=status)
            names += ["count", "prefix", "fields", "time", "link", "side"]
            out += [count, prefix] + list(rows[:4])
        host = dict(zip(names, datareader._download(out)))
    ops.stitch_check(int(host["status"][0]))
    if fill:
        n = int(host["prefix"][-1])
        for k in ("fields", "time", "link", "side"):
            host[k] = host[k][:n]
    return host


def _report(pk, host, fill):
    links = [(int(a), int(host["next"][a]), float(host["link_cost"][a])) for a in np.nonzero(host["next"] >= 0)[0]]
    report = dict(ids=pk["ids"], ep=host["ep"], root=host["root"], rank=host["rank"], new_id=host["new_id"], next=host["next"],
                  prev=host["prev"], links=links, status=int(host["status"][0]), fill=None)
    if fill:
        report["fill"] = dict(fields=host["fields"], time=host["time"], link=host["link"], side=host["side"], count=host["count"],
                              skipped=0)
    return report


def _frame_key(frame):
    for item in frame.values():
        return item["timestamp"]
    return None


def rebuild(data, pk, host, fill):
    """The host's last step -> new_data: every datum copied under its chain's id, then the filled rows, frames sorted by time
    stamp.  -> (new_data, the filled rows that were left out because their frame already holds the chain's id)."""
    new_of = {int(k): int(v) for k, v in zip(pk["ids"], host["new_id"])}
    new_data = []
    for frame in data:
        out = {}
        for key, item in frame.items():
            item = item.copy()
            item["id"] = new_of[key]
            out[new_of[key]] = item
        new_data.append(out)
    if not fill or len(host["time"]) == 0:
        return new_data, 0
    where = {}
    for f, frame in enumerate(new_data):
        ts = _frame_key(frame)
        if ts is not None:
            where.setdefault(ts, f)
    keys = [_frame_key(frame) for frame in new_data]
    for f in range(len(keys)):                                     # an empty frame sorts with the frame before it
        if keys[f] is None:
            keys[f] = keys[f - 1] if f and keys[f - 1] is not None else -np.inf
    offsets, n_old, skipped = pk["offsets"], len(new_data), 0
    for u in range(len(host["time"])):
        a = int(host["link"][u])
        b = int(host["next"][a])
        src = pk["rows"][offsets[a + 1] - 1] if host["side"][u] == 0 else pk["rows"][offsets[b]]
        item = src.copy()
        for k, name in enumerate(FIELDS):
            item[name] = float(host["fields"][u, k])
        item["direction"] = int(host["ep"][a, 1, 12])
        item["timestamp"] = np.round(host["time"][u], 4)
        item["id"] = int(host["new_id"][a])
        f = where.get(item["timestamp"])
        if f is None:
            where[item["timestamp"]] = f = len(new_data)
            new_data.append({})
            keys.append(item["timestamp"])
        if item["id"] in new_data[f]:
            skipped += 1
            continue
        new_data[f][item["id"]] = item
    order = sorted(range(len(new_data)), key=lambda f: (keys[f], f >= n_old, f))
    return [new_data[f] for f in order], skipped


def stitch_tracks(data, params=None, fill=True, device=None):
    """-> (new_data, report).  ``report``: ``ids`` (the tracklet ids, ascending), per tracklet ``ep`` (the end-point block [N,2,16],
    layout in include/retinanet_mi355x.h), ``root``, ``rank``, ``new_id``, ``next`` / ``prev``; ``links`` [(a, b, cost)] by tracklet
    index; ``fill`` (fields [U,6], time, link, side, count, skipped) or None; ``status`` (0: anything else raised).  ``data`` is
    not modified."""
    import datareader
    params = resolve_params(params)
    pk = pack_tracklets(data)
    if len(pk["ids"]) == 0:
        datareader._cuda(device)
        empty = dict(status=np.zeros(1, np.int32), ep=np.zeros((0, 2, ops.STITCH_EP)), ncand=np.zeros(4, np.int32),
                     next=np.zeros(0, np.int32), prev=np.zeros(0, np.int32), link_cost=np.zeros(0), root=np.zeros(0, np.int32),
                     rank=np.zeros(0, np.int32), new_id=np.zeros(0, np.int64), count=np.zeros(0, np.int32), fields=np.zeros((0, 6)),
                     time=np.zeros(0), link=np.zeros(0, np.int32), side=np.zeros(0, np.uint8))
        return [dict(frame) for frame in data], _report(pk, empty, fill)
    host = stitch_packed(pk["ids"], pk["offsets"], pk["cols"], pk["direction"], params, fill, device)
    report = _report(pk, host, fill)
    new_data, skipped = rebuild(data, pk, host, fill)
    if fill:
        report["fill"]["skipped"] = skipped
    return new_data, report

"""Track stitching (track_stitch.py, csrc/stitch.hip): the plain restatement of every stage in Python floats -- fp64 with one
rounding per operation, every expression in the order the device evaluates it --, the scenes and their expected values.

Layout.  A tracklet is all rows of one id in time order: offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v), direction
int32 [R].  An end point is EP = 16 doubles, ep [N,2,EP] with end 0 = the head and end 1 = the tail:
  0 t of the end row, 1 fitted x at that time, 2 fitted slope, 3..6 mean y, l, w, h, 7..11 the end row's x, y, l, w, h, 12 sgn, 13 k.
The scales of a link cost are P = (max_gap, back_tol, sigma_x0, sigma_x1, sigma_y, sigma_size, max_cost).
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

EP = 16
T, XH, VX, Y, L, W, H, RX, RY, RL, RW, RH, SGN, K = range(14)
DEFAULTS = {"fit_n": 8, "max_gap": 3.0, "back_tol": 5.0, "sigma_x0": 10.0, "sigma_x1": 10.0, "sigma_y": 4.0, "sigma_size": 10.0,
            "max_cost": 3.0, "fill_rate": 30.0}
SCALES = ("max_gap", "back_tol", "sigma_x0", "sigma_x1", "sigma_y", "sigma_size", "max_cost")
P0 = tuple(DEFAULTS[k] for k in SCALES)


# ------------------------------------------------------------------------------------------------ the restatement
def endpoints(offsets, cols, direction, fit_n):
    N = len(offsets) - 1
    ep = np.zeros((N, 2, EP))
    for i in range(N):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        sgn = 1.0 if sum(int(d) for d in direction[lo:hi]) >= 0 else -1.0
        k = min(hi - lo, fit_n)
        for end in (0, 1):
            r0, rend = (lo, lo) if end == 0 else (hi - k, hi - 1)
            s = [0.0] * 6
            for r in range(r0, r0 + k):                         # sequential, ascending: not np.sum
                for q in range(6):
                    s[q] = s[q] + float(cols[r, q])
            mt, mx = s[0] / k, s[1] / k
            Stt = Stx = 0.0
            for r in range(r0, r0 + k):
                dt = float(cols[r, 0]) - mt
                Stt = Stt + dt * dt
                Stx = Stx + dt * (float(cols[r, 1]) - mx)
            e = [float(v) for v in cols[rend]]
            vx = Stx / Stt if (k >= 2 and Stt > 0.0) else sgn * e[6]
            ep[i, end, :14] = [e[0], mx + vx * (e[0] - mt), vx, s[2] / k, s[3] / k, s[4] / k, s[5] / k, e[1], e[2], e[3], e[4], e[5],
                               sgn, float(k)]
    return ep


def pair(A, B, P):
    """a's tail A -> b's head B (a != b is the caller's): (linkable, cost)."""
    max_gap, back_tol, sx0, sx1, sy, ss, max_cost = P
    A, B = [float(v) for v in A], [float(v) for v in B]
    gap = B[T] - A[T]
    if not gap > 0.0 or not gap <= max_gap or A[SGN] != B[SGN]:
        return False, 0.0
    if not A[SGN] * (B[XH] - A[XH]) >= -back_tol:
        return False, 0.0
    cost = ((abs(A[XH] + A[VX] * gap - B[XH]) + abs(B[XH] - B[VX] * gap - A[XH])) / 2.0) / (sx0 + sx1 * gap) \
        + abs(A[Y] - B[Y]) / sy + (abs(A[L] - B[L]) + abs(A[W] - B[W]) + abs(A[H] - B[H])) / ss
    return cost < max_cost, cost


def costs(ep, P):
    N = len(ep)
    Wm = np.zeros((N, N))
    for a in range(N):
        for b in np.nonzero((ep[:, 0, T] > ep[a, 1, T]) & (ep[:, 0, T] - ep[a, 1, T] <= P[0] + 1.0))[0]:   # a prefilter only
            ok, c = pair(ep[a, 1], ep[b, 0], P)
            if ok and a != b:
                Wm[a, b] = c - P[6]
    return Wm


def candidates(Wm, ep):
    N = len(ep)
    cand, ncand = np.full((2, 2, N), -1, np.int32), np.zeros(4, np.int32)
    link = Wm < 0
    for d in (0, 1):
        mine = (ep[:, 0, SGN] > 0.0) == (d == 0)
        for side, has in ((0, link.any(axis=1)), (1, link.any(axis=0))):
            idx = np.nonzero(has & mine)[0]
            cand[d, side, :len(idx)] = idx
            ncand[2 * d + side] = len(idx)
    return cand, ncand


def compact(Wm, cand, ncand):
    return [Wm[np.ix_(cand[d, 0, :ncand[2 * d]], cand[d, 1, :ncand[2 * d + 1]])].copy() for d in (0, 1)]


def assign(ep, P, cand, ncand, Wcs):
    N = len(ep)
    nxt, prev, link_cost = np.full(N, -1, np.int32), np.full(N, -1, np.int32), np.zeros(N)
    for d in (0, 1):
        Wc = Wcs[d]
        if Wc.size == 0:
            continue
        for r, c in zip(*linear_sum_assignment(Wc)):
            if Wc[r, c] < 0:
                a, b = int(cand[d, 0, r]), int(cand[d, 1, c])
                nxt[a], prev[b], link_cost[a] = b, a, pair(ep[a, 1], ep[b, 0], P)[1]
    return nxt, prev, link_cost


def chains(prev, ids):
    N = len(prev)
    root, rank = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for i in range(N):
        j, n = i, 0
        while prev[j] >= 0:
            j, n = int(prev[j]), n + 1
            assert n <= N
        root[i], rank[i] = j, n
    return root, rank, np.asarray(ids, np.int64)[root] if N else np.zeros(0, np.int64)


def fill_count(ep, nxt, fill_rate):
    N = len(ep)
    count = np.zeros(N, np.int32)
    dt = 1.0 / fill_rate
    for a in range(N):
        if nxt[a] >= 0:
            te, ts = float(ep[a, 1, T]), float(ep[nxt[a], 0, T])
            k = 1
            while te + k * dt < ts:
                k += 1
            count[a] = k - 1
    return count, np.concatenate(([0], np.cumsum(count, dtype=np.int64))).astype(np.int64)


def fill_rows(ep, nxt, prefix, fill_rate):
    U = int(prefix[-1])
    fields, time, link, side = np.zeros((U, 6)), np.zeros(U), np.zeros(U, np.int32), np.zeros(U, np.uint8)
    dt = 1.0 / fill_rate
    for a in range(len(ep)):
        for k in range(1, int(prefix[a + 1] - prefix[a]) + 1):
            A, B = [float(v) for v in ep[a, 1]], [float(v) for v in ep[nxt[a], 0]]
            te, ts = A[T], B[T]
            g = ts - te
            tk = te + k * dt
            u = (tk - te) / g
            om = 1.0 - u
            xa, xb, va, vb = A[RX], B[RX], A[VX], B[VX]
            h00, h10, h01, h11 = (1.0 + 2.0 * u) * (om * om), u * (om * om), (u * u) * (3.0 - 2.0 * u), (u * u) * (u - 1.0)
            d00, d10, d01, d11 = 6.0 * u * u - 6.0 * u, 3.0 * u * u - 4.0 * u + 1.0, 6.0 * u - 6.0 * u * u, 3.0 * u * u - 2.0 * u
            row = int(prefix[a]) + k - 1
            fields[row] = [h00 * xa + h10 * g * va + h01 * xb + h11 * g * vb, om * A[RY] + u * B[RY], om * A[RL] + u * B[RL],
                           om * A[RW] + u * B[RW], om * A[RH] + u * B[RH],
                           abs((d00 * xa + d10 * g * va + d01 * xb + d11 * g * vb) / g)]
            time[row], link[row], side[row] = tk, a, 0 if u <= 0.5 else 1
    return fields, time, link, side


def scales_of(params):
    p = dict(DEFAULTS, **(params or {}))
    return p, tuple(float(p[k]) for k in SCALES)


def run_all(ids, offsets, cols, direction, params=None, fill=True):
    """Every stage on packed arrays -> dict of all intermediate and final arrays."""
    p, P = scales_of(params)
    ep = endpoints(offsets, cols, direction, p["fit_n"])
    return run_from_ep(ep, ids, params, fill)


def run_from_ep(ep, ids, params=None, fill=True):
    p, P = scales_of(params)
    Wm = costs(ep, P)
    cand, ncand = candidates(Wm, ep)
    Wcs = compact(Wm, cand, ncand)
    nxt, prev, link_cost = assign(ep, P, cand, ncand, Wcs)
    root, rank, new_id = chains(prev, ids)
    out = dict(ep=ep, W=Wm, cand=cand, ncand=ncand, Wc=np.concatenate([w.reshape(-1) for w in Wcs]), next=nxt, prev=prev,
               link_cost=link_cost, root=root, rank=rank, new_id=new_id)
    if fill:
        out["count"], out["prefix"] = fill_count(ep, nxt, p["fill_rate"])
        out["fields"], out["time"], out["link"], out["side"] = fill_rows(ep, nxt, out["prefix"], p["fill_rate"])
    return out


# ------------------------------------------------------------------------------------------------ scenes: packed rows
def pack_lists(tracklets):
    """[(id, rows [n,7], directions [n])] -> (ids, offsets, cols, direction), tracklets in ascending id."""
    tracklets = sorted(tracklets, key=lambda t: t[0])
    ids = np.array([t[0] for t in tracklets], np.int64)
    offsets = np.concatenate(([0], np.cumsum([len(t[1]) for t in tracklets]))).astype(np.int64)
    cols = np.concatenate([np.asarray(t[1], np.float64).reshape(-1, 7) for t in tracklets]) if tracklets else np.zeros((0, 7))
    direction = np.concatenate([np.asarray(t[2], np.int32).reshape(-1) for t in tracklets]) if tracklets else np.zeros(0, np.int32)
    return ids, offsets, cols, direction.astype(np.int32)


def endpoint_scene():
    """Tracklets of 1, 2, 7, 8, 9 and 70 rows in both directions (the fit window of 8 is shorter than, equal to and longer than a
    tracklet; 70 is longer than fit_n = 64), two rows with EQUAL times (Stt = 0: the slope falls back to sgn * v), a tracklet
    whose directions sum to 0 (sgn = +1) and one whose sum is negative with mixed signs."""
    rng = np.random.RandomState(11)
    out, tid = [], 100
    for n in (1, 2, 7, 8, 9, 70):
        for sgn in (1, -1):
            t = 1623877000.0 + np.round(np.cumsum(0.02 + 0.03 * rng.rand(n)), 4)
            x = 500.0 + sgn * 95.0 * (t - t[0]) + rng.randn(n) * 0.8
            rows = np.stack([t, x, 30.0 + rng.randn(n), 15.0 + rng.rand(n), 6.0 + rng.rand(n), 5.0 + rng.rand(n), 90.0 + rng.randn(n)], 1)
            out.append((tid, rows, np.full(n, sgn)))
            tid -= 7                                            # ids descend: packing sorts them
    same = np.array([[5.0, 10.0, 1.0, 15.0, 6.0, 5.0, 88.0], [5.0, 12.0, 3.0, 16.0, 7.0, 6.0, 77.0]])
    out.append((500, same, [-1, -1]))
    out.append((501, np.column_stack([np.arange(4.0), 100.0 * np.arange(4.0), np.zeros(4), np.ones(4), np.ones(4), np.ones(4), np.ones(4)]),
                [1, -1, -1, 1]))
    out.append((502, np.column_stack([np.arange(3.0), -50.0 * np.arange(3.0), np.zeros(3), np.ones(3), np.ones(3), np.ones(3), np.ones(3)]),
                [1, -1, -1]))
    return pack_lists(out)


def lane_scene(n, seed, both=True):
    """n short fragments of vehicles at about 100 ft/s in four lanes 12 ft apart (and, with ``both``, as many again the other
    way), starting within a few seconds of each other: many candidates per tail, heads shared by several tails."""
    rng = np.random.RandomState(seed)
    out, tid = [], 0
    for sgn in ((1, -1) if both else (1,)):
        for _ in range(n):
            t0 = 100.0 + np.round(rng.rand() * (2.0 + n / 10.0), 4)
            m = rng.randint(1, 6)
            t = t0 + np.round(np.arange(m) / 30.0, 4)
            x0 = 1000.0 + sgn * 100.0 * (t0 - 100.0) + rng.randn() * 15.0
            x = x0 + sgn * (100.0 + rng.randn() * 3.0) * (t - t0)
            y = sgn * (6.0 + 12.0 * rng.randint(0, 4)) + rng.randn(m) * 0.3
            rows = np.stack([t, x, y, 15.0 + rng.rand(m), 6.0 + rng.rand(m) * 0.5, 5.0 + rng.rand(m) * 0.5, np.full(m, 100.0)], 1)
            out.append((tid, rows, np.full(m, sgn)))
            tid += 1
    return pack_lists(out)


def make_ep(t_s, t_e, x, y, vx=0.0, size=(15.0, 6.0, 5.0), sgn=1.0, x_e=None):
    """A hand-made end-point pair of one stationary-or-uniform tracklet: head at (t_s, x), tail at (t_e, x_e or x)."""
    e = np.zeros((2, EP))
    for end, (t, xx) in enumerate(((t_s, x), (t_e, x if x_e is None else x_e))):
        e[end, :14] = [t, xx, vx, y, size[0], size[1], size[2], xx, y, size[0], size[1], size[2], sgn, 1.0]
    return e


def edge_ep():
    """Hand-made end points, pairs kept apart by lanes 100 ft from each other -> (ep, {(a, b): linkable}).  With the defaults:
    gap exactly 0 (not linkable) and exactly max_gap (linkable); y apart by exactly sigma_y * max_cost = 12 ft with everything else
    equal, so the cost is max_cost exactly (not linkable), and one ulp less (linkable); a head exactly back_tol behind the tail
    (linkable, cost 5 / 20) and one ulp further (not); the same in the other direction; equal ends in opposite directions (not)."""
    eps, want = [], {}

    def add(a, b, ok):
        eps.extend((a, b))
        want[(len(eps) - 2, len(eps) - 1)] = ok
    add(make_ep(8.0, 10.0, 50.0, 0.0), make_ep(10.0, 11.0, 50.0, 0.0), False)                       # gap 0
    add(make_ep(8.0, 10.0, 50.0, 100.0), make_ep(13.0, 14.0, 50.0, 100.0), True)                    # gap max_gap
    add(make_ep(8.0, 10.0, 50.0, 200.0), make_ep(13.0 + 2.0 ** -48, 14.0, 50.0, 200.0), False)      # just above
    add(make_ep(8.0, 10.0, 50.0, 300.0), make_ep(11.0, 12.0, 50.0, 312.0), False)                   # cost == max_cost
    add(make_ep(8.0, 10.0, 50.0, 400.0), make_ep(11.0, 12.0, 50.0, np.nextafter(412.0, 0.0)), True)
    add(make_ep(8.0, 10.0, 50.0, 500.0), make_ep(11.0, 12.0, 45.0, 500.0), True)                    # exactly on back_tol
    add(make_ep(8.0, 10.0, 50.0, 600.0), make_ep(11.0, 12.0, np.nextafter(45.0, 0.0), 600.0), False)
    add(make_ep(8.0, 10.0, 50.0, -700.0, sgn=-1.0), make_ep(11.0, 12.0, 55.0, -700.0, sgn=-1.0), True)
    add(make_ep(8.0, 10.0, 50.0, -800.0, sgn=-1.0), make_ep(11.0, 12.0, np.nextafter(55.0, 60.0), -800.0, sgn=-1.0), False)
    add(make_ep(8.0, 10.0, 50.0, 900.0, sgn=1.0), make_ep(11.0, 12.0, 50.0, 900.0, sgn=-1.0), False)
    return np.stack(eps), want


def greedy_trap_ep():
    """Tails A1 (0), A2 (1), heads B1 (2), B2 (3), all at one x, costs |dy| / 4: A1-B1 0.1 (the nearest pair), A1-B2 0.3, A2-B1 0.2,
    A2-B2 not linkable (B2 starts before A2 ends).  Greedy takes A1-B1 and leaves A2 alone (benefit 2.9); the optimum is A1-B2 +
    A2-B1 (2.7 + 2.8).  -> (ep, links)."""
    ep = np.stack([make_ep(8.0, 10.0, 50.0, 0.0), make_ep(8.0, 11.0, 50.0, 1.2), make_ep(12.0, 13.0, 50.0, 0.4),
                   make_ep(10.5, 10.75, 50.0, -1.2)])
    return ep, {(0, 3), (1, 2)}


def funnel_ep(n_tails, n_heads, seed, sgn=1.0):
    """n_tails tracklets ending at t = 10 and n_heads starting at t = 11, all in one lane: every pair is a candidate, nr' x nc'."""
    rng = np.random.RandomState(seed)
    return np.stack([make_ep(8.0, 10.0, 50.0, sgn * (20.0 + rng.rand() * 4.0), sgn=sgn) for _ in range(n_tails)]
                    + [make_ep(11.0, 12.0, 50.0, sgn * (20.0 + rng.rand() * 4.0), sgn=sgn) for _ in range(n_heads)])


def no_candidate_ep(n=5):
    return np.stack([make_ep(8.0 + i, 9.0 + i, 50.0, 100.0 * i) for i in range(n)])


def chain_prev(lengths=(2, 9, 33), singles=3, seed=5):
    """prev of chains of the given lengths and some single tracklets under a shuffled numbering -> (prev, ids, want_root,
    want_rank).  9 and 33 need pointer jumping's last round for one tracklet only (distance 2^k)."""
    rng = np.random.RandomState(seed)
    N = sum(lengths) + singles
    perm = rng.permutation(N)
    prev, root, rank, at = np.full(N, -1, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32), 0
    for n in tuple(lengths) + (1,) * singles:
        members = perm[at:at + n]
        for k, m in enumerate(members):
            prev[m] = members[k - 1] if k else -1
            root[m], rank[m] = members[0], k
        at += n
    ids = (rng.permutation(N) * 3 + 1000).astype(np.int64)
    return prev, ids, root, rank


def fill_ep():
    """Hand-made links at 30 Hz -> (ep, next): new rows 0 (gap below one step), 1, 70 and twenty more of 70 (1 471 in all, more
    than the 1 024 of four workgroups), tracklets that link to nothing in between.  x moves and the slopes differ at both ends."""
    eps, nxt = [], []

    def link(t_e, t_s, lane):
        a = make_ep(t_e - 2.0, t_e, 300.0, lane, vx=90.0, x_e=480.0)
        b = make_ep(t_s, t_s + 1.0, 480.0 + 100.0 * (t_s - t_e), lane + 0.5, vx=110.0, size=(16.0, 6.5, 5.5))
        eps.extend((a, b))
        nxt.extend((len(eps) - 1, -1))
    link(10.0, 10.02, 0.0)
    link(10.0, 10.05, 12.0)
    eps.append(make_ep(1.0, 2.0, 0.0, 500.0))
    nxt.append(-1)
    link(10.0, 12.35, 24.0)
    for i in range(20):
        link(20.0 + 0.01 * i, 22.35 + 0.01 * i, 36.0)
    return np.stack(eps), np.array(nxt, np.int32)


def quarter_ep():
    """t_e = 1.0, t_s = 1.5 at fill_rate 4: t_2 lands on t_s (excluded: one new row), and its u is exactly 0.5 (side 0)."""
    return np.stack([make_ep(0.0, 1.0, 10.0, 0.0, vx=8.0, x_e=18.0), make_ep(1.5, 2.0, 22.0, 0.0, vx=8.0)]), np.array([1, -1], np.int32)


# ------------------------------------------------------------------------------------------------ end to end, closed form
LANES = 8                                                       # one vehicle per lane and direction, lanes 12 ft apart
FRAMES = 600                                                    # 20 s at 30 Hz


def highway(seed):
    """Eight vehicles at noise-free constant speed, each cut into fragments of 1 .. 59 rows with gaps of 1 .. 84 frames (at most
    2.8 s, inside max_gap) -> (data as Data_Reader holds it with shuffled fragment ids, {fragment id: vehicle}, the time stamps).
    Cross-lane pairs cost at least max_cost (12 ft / sigma_y), every true link costs about 1e-13, and a matching with as many links
    as the true one must be the time-ordered chain: stitching recovers the vehicles exactly."""
    rng = np.random.RandomState(seed)
    stamps = [np.round(j / 30.0, 4) for j in range(FRAMES)]
    pieces = []
    for v in range(LANES):
        sgn = 1 if v < LANES // 2 else -1
        y = sgn * (6.0 + 12.0 * (v % (LANES // 2)))
        speed, x0 = 90.0 + 5.0 * v, 1000.0 + 37.0 * v
        j = int(rng.randint(0, 10))
        while j < FRAMES:
            n = int(rng.randint(1, 60))
            pieces.append((v, sgn, y, speed, x0, j, min(j + n, FRAMES)))
            j += n + int(rng.randint(1, 85))
    frag_ids = rng.permutation(len(pieces)) + 1
    data, owner = [{} for _ in range(FRAMES)], {}
    for fid, (v, sgn, y, speed, x0, j0, j1) in zip(frag_ids, pieces):
        owner[int(fid)] = v
        for j in range(j0, j1):
            data[j][int(fid)] = {"timestamp": stamps[j], "id": int(fid), "class": "sedan", "x": x0 + sgn * speed * float(stamps[j]), "y": y,
                                 "l": 15.0 + v, "w": 6.0, "h": 5.0, "direction": sgn, "v": speed, "ts_bias": {"p1c1": 0.0},
                                 "camera": "p1c1", "frame": str(j), "vehicle": v}      # "vehicle": the truth, for the tests only
    keep = [f for f in range(FRAMES) if data[f]]
    return [data[f] for f in keep], owner, [stamps[f] for f in keep]


def assoc_scene(truth_frames, pred_data, label):
    """A scene for mot_assoc_cases.scene_rows: the ground truth holds every vehicle in every frame of ``truth_frames`` (time stamps),
    the prediction the rows of ``pred_data`` under ``label(id)``; IoU 1 between a vehicle and its own row, 0 otherwise."""
    by_ts = {}
    for frame in pred_data:
        for key, item in frame.items():
            by_ts.setdefault(item["timestamp"], []).append((label(key), item["vehicle"]))
    gt_ids, pred_ids, ious = [], [], []
    for ts in truth_frames:
        preds = by_ts.get(ts, [])
        gt_ids.append(list(range(1, LANES + 1)))
        pred_ids.append([p[0] for p in preds])
        ious.append(np.array([[1.0 if p[1] == g else 0.0 for p in preds] for g in range(LANES)]) if preds else None)
    return dict(gt_ids=gt_ids, pred_ids=pred_ids, ious=ious)

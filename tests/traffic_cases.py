"""Traffic state (traffic_state.py, csrc/traffic.hip): the plain restatement of every rule in Python and numpy -- fp64 with one
rounding per operation, the sums of T and D as Python integers -- and the scenes of tests/test_traffic_host.py and
tests/test_gpu_traffic.py.

Packed input as for stitching and smoothing: offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v), direction int32 [R].
``edges`` = {1: ascending lane edges of direction +1, -1: those of direction -1}; ``grid`` = (t0, dt, nt, x0, dx, nx).
"""
import math

import numpy as np

Q = 1 << 20
MAX_CUTS = 4096
NONFINITE, BAD_OFFSETS, BAD_FRAME, TOO_MANY_CUTS, RANGE, BAD_DIR = 1, 2, 4, 8, 16, 32
CELL_COUNTERS = ("segments", "used", "skipped_gap", "skipped_lane", "pieces", "outside")
DEFAULT_EDGES = {1: [0.0, 12.0, 24.0, 36.0, 48.0, 60.0], -1: [60.0, 72.0, 84.0, 96.0, 108.0, 120.0]}
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the rules
def lane_of(edges, y):
    """The first k with edges[k] <= y < edges[k+1], else -1."""
    for k in range(len(edges) - 1):
        if edges[k] <= y < edges[k + 1]:
            return k
    return -1


def n_lanes(edges):
    return max(len(edges[1]), len(edges[-1]), 1) - 1


def lanes(offsets, cols, direction, edges):
    """-> (dir int32 [N]: +1 when the tracklet's directions sum to >= 0 else -1; lane int32 [R] from each row's own y; status)."""
    N, R = len(offsets) - 1, len(cols)
    d = np.ones(N, np.int32)
    lane = np.full(R, -1, np.int32)
    status = 0
    for i in range(N):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        d[i] = 1 if sum(int(v) for v in direction[lo:hi]) >= 0 else -1
        for r in range(lo, hi):
            if not all(math.isfinite(v) for v in cols[r]):
                status |= NONFINITE
                continue
            lane[r] = lane_of(edges[int(d[i])], float(cols[r, 2]))
    return d, lane, status


def segment_pieces(ta, xa, tb, xb, grid):
    """The pieces of one used segment -> [(it, ix, u, v)] with it, ix floats (not yet checked against the grid), or None when the
    segment crosses more than MAX_CUTS grid lines."""
    t0, dt, nt, x0, dx, nx = grid
    Tt, X = tb - ta, xb - xa
    ka, kb = math.floor((ta - t0) / dt), math.floor((tb - t0) / dt)
    ma, mb = math.floor((min(xa, xb) - x0) / dx), math.floor((max(xa, xb) - x0) / dx)
    if not (float(kb) - float(ka)) + (float(mb) - float(ma)) <= MAX_CUTS:
        return None
    cuts = [((t0 + (float(ka) + float(i + 1)) * dt) - ta) / Tt for i in range(kb - ka)]
    if X != 0:
        cuts += [((x0 + (float(ma) + float(i + 1)) * dx) - xa) / X for i in range(mb - ma)]
    points = [0.0] + sorted(s for s in cuts if 0 < s < 1) + [1.0]
    out = []
    for u, v in zip(points[:-1], points[1:]):
        if v <= u:
            continue
        sm = (u + v) * 0.5
        out.append((math.floor(((ta + sm * Tt) - t0) / dt), math.floor(((xa + sm * X) - x0) / dx), u, v))
    return out


def cells(offsets, cols, d, edges, grid, max_gap):
    """Every segment of every tracklet -> dict(T, D int64 [2,L,nt,nx] (from Python integers), n int32, counters {name: int}, status,
    max_pieces, whole = (sum of rint(Tt Q), sum of rint(|X| Q)) over the used segments: what the conservation rule compares with)."""
    t0, dt, nt, x0, dx, nx = grid
    L = n_lanes(edges)
    T, D, n = {}, {}, {}
    c = dict.fromkeys(CELL_COUNTERS, 0)
    status, max_pieces, whole_T, whole_D = 0, 0, 0, 0
    for i in range(len(offsets) - 1):
        for r in range(int(offsets[i]), int(offsets[i + 1]) - 1):
            c["segments"] += 1
            ta, xa, ya = (float(v) for v in cols[r, :3])
            tb, xb, yb = (float(v) for v in cols[r + 1, :3])
            if not all(math.isfinite(v) for v in (ta, xa, ya, tb, xb, yb)):
                status |= NONFINITE
                continue
            if int(d[i]) not in (1, -1):
                status |= BAD_DIR
                continue
            Tt, X = tb - ta, xb - xa
            if not 0 < Tt <= max_gap:
                c["skipped_gap"] += 1
                continue
            ln = lane_of(edges[int(d[i])], (ya + yb) * 0.5)
            if ln < 0:
                c["skipped_lane"] += 1
                continue
            if not (Tt * Q < 2.0 ** 40 and abs(X) * Q < 2.0 ** 40):
                status |= RANGE
                continue
            pieces = segment_pieces(ta, xa, tb, xb, grid)
            if pieces is None:
                status |= TOO_MANY_CUTS
                continue
            c["used"] += 1
            whole_T += int(np.rint(Tt * Q))
            whole_D += int(np.rint(abs(X) * Q))
            max_pieces = max(max_pieces, len(pieces))
            for it, ix, u, v in pieces:
                c["pieces"] += 1
                if not (0 <= it < nt and 0 <= ix < nx):
                    c["outside"] += 1
                    continue
                key = (0 if d[i] == 1 else 1, ln, it, ix)
                T[key] = T.get(key, 0) + int(np.rint(((v - u) * Tt) * Q))
                D[key] = D.get(key, 0) + int(np.rint(((v - u) * abs(X)) * Q))
                n[key] = n.get(key, 0) + 1
    out = dict(counters=c, status=status, max_pieces=max_pieces, whole=(whole_T, whole_D))
    for name, src, dtype in (("T", T, np.int64), ("D", D, np.int64), ("n", n, np.int32)):
        a = np.zeros((2, L, nt, nx), dtype)
        for key, v in src.items():
            a[key] = v                                                     # OverflowError if a sum left int64
        out[name] = a
    return out


def frames_csr(frame):
    """The packed rows by frame: a stable argsort of ``frame`` -> (frame_off int64 [F+1], frame_rows int32 [R]); F = the largest
    frame index + 1."""
    frame = np.asarray(frame, np.int64).reshape(-1)
    F = int(frame.max()) + 1 if len(frame) else 0
    rows = np.argsort(frame, kind="stable").astype(np.int32)
    off = np.zeros(F + 1, np.int64)
    np.cumsum(np.bincount(frame, minlength=F), out=off[1:])
    return off, rows


def leaders(offsets, cols, d, lane, frame_off, frame_rows):
    """-> dict(leader int32 [R], spacing, gap, headway, ttc fp64 [R], with_leader, overlaps, ties = the rows whose leader had a rival
    at the same spacing, status)."""
    R = len(cols)
    trk = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    out = dict(leader=np.full(R, -1, np.int32), with_leader=0, overlaps=0, ties=0, status=0)
    for k in ("spacing", "gap", "headway", "ttc"):
        out[k] = np.full(R, INF)
    for f in range(len(frame_off) - 1):
        rows = [int(r) for r in frame_rows[int(frame_off[f]):int(frame_off[f + 1])]]
        ok = {r: all(math.isfinite(float(cols[r, q])) for q in (1, 3, 6)) for r in rows}
        if not all(ok.values()):
            out["status"] |= NONFINITE
        for i in rows:
            if not ok[i]:
                continue
            di, best = int(d[trk[i]]), None
            for j in rows:
                if j == i or not ok[j] or int(d[trk[j]]) != di or lane[j] != lane[i] or lane[i] < 0:
                    continue
                s = di * (float(cols[j, 1]) - float(cols[i, 1]))
                if not s > 0:
                    continue
                cand = (s, int(trk[j]), j)
                if best is not None and cand[0] == best[0]:
                    out["ties"] += 1
                if best is None or cand < best:
                    best = cand
            if best is None:
                continue
            s, _, j = best
            li, vi, vj = float(cols[i, 3]), float(cols[i, 6]), float(cols[j, 6])
            g = s - li
            out["leader"][i], out["spacing"][i], out["gap"][i] = j, s, g
            out["headway"][i] = s / vi if vi > 0 else INF
            out["ttc"][i] = g / (vi - vj) if vi > vj and g > 0 else INF
            out["with_leader"] += 1
            out["overlaps"] += g < 0
    return out


def derive_grid(cols, dx, dt):
    """traffic_state.grid_of with no explicit range, restated: x0 over all rows, t0 over the rows with a time stamp > 0."""
    x, t = cols[:, 1], cols[:, 0][cols[:, 0] > 0]
    x0, t0 = math.floor(x.min() / dx) * dx, math.floor(t.min() / dt) * dt
    return (t0, dt, math.floor((t.max() - t0) / dt) + 1, x0, dx, math.floor((x.max() - x0) / dx) + 1)


# ------------------------------------------------------------------------------------------------ scenes
def pack(tracks, directions):
    """tracks: list of [n,7] arrays (or lists of rows); directions: one int or a list of ints per tracklet."""
    offsets, rows, dirs = [0], [], []
    for tr, d in zip(tracks, directions):
        tr = np.asarray(tr, np.float64).reshape(-1, 7)
        rows.append(tr)
        dirs += [d] * len(tr) if np.isscalar(d) else list(d)
        offsets.append(offsets[-1] + len(tr))
    return np.asarray(offsets, np.int64), np.concatenate(rows).reshape(-1, 7), np.asarray(dirs, np.int32)


def row(t, x, y=6.0, l=16.0, v=64.0):
    return [t, x, y, l, 6.0, 5.0, v]


def frames_of(cols):
    """The frame index of every packed row as Data_Reader holds it: one frame per unique rounded time stamp, ascending."""
    ts = np.round(cols[:, 0], 4)
    return np.searchsorted(np.unique(ts), ts).astype(np.int64)


CLOSED = dict(speed=64.0, headway=2.0, rate=32, seconds=16, vehicles=12, base=1024.0, dx=64.0, dt=2.0, length=16.0)


def closed_form_scene():
    """Vehicles of one lane at a constant 64 ft/s, 2 s apart, sampled every 1/32 s for 16 s each: every number is dyadic.  Over the
    grid dx = 64, dt = 2 the cell (it, ix) is crossed by vehicle it - ix // 2 alone, for one second and 64 ft.
    -> (offsets, cols, direction, frame)."""
    c = CLOSED
    tracks = []
    for k in range(c["vehicles"]):
        tau = np.arange(c["seconds"] * c["rate"] + 1) / c["rate"]
        tracks.append([row(c["base"] + c["headway"] * k + s, c["speed"] * s, l=c["length"], v=c["speed"]) for s in tau])
    offsets, cols, direction = pack(tracks, [1] * c["vehicles"])
    return offsets, cols, direction, frames_of(cols)


def closed_form_interior(grid):
    """The cells (it, ix) of the closed-form scene that a vehicle crosses completely."""
    c = CLOSED
    t0, dt, nt, x0, dx, nx = grid
    assert (t0, x0) == (c["base"], 0.0)
    return [(it, ix) for it in range(nt) for ix in range(int(c["speed"] * c["seconds"] / dx)) if 0 <= it - ix // 2 < c["vehicles"]]


EDGE_GRID = (100.0, 2.0, 6, 0.0, 64.0, 6)
EDGE_MAX_GAP = 8.0


def cell_edge_scene():
    """One tracklet per edge of the cell rule, over EDGE_GRID with EDGE_MAX_GAP -> (offsets, cols, direction, names)."""
    tr = [
        ("one_row", 1, [row(101, 10)]),
        ("no_cut", 1, [row(100.5, 10), row(101, 20)]),
        ("time_cut", 1, [row(101.5, 70), row(102.5, 100)]),
        ("x_cut", 1, [row(102.25, 60), row(102.75, 70)]),
        ("both_cuts_same_s", 1, [row(101.5, 48), row(102.5, 80)]),
        ("eight_pieces", 1, [row(100.5, 10), row(107.5, 300)]),
        ("no_motion", 1, [row(103, 100), row(105, 100)]),
        ("backwards", 1, [row(104.5, 200), row(105.5, 100)]),
        ("on_grid_lines", 1, [row(102, 64), row(103, 128)]),
        ("ym_on_an_edge", 1, [row(106, 10, y=11), row(106.5, 20, y=13)]),
        ("ym_on_the_last_edge", 1, [row(106, 10, y=59), row(106.5, 20, y=61)]),
        ("outside_in_x", 1, [row(109, 350), row(110, 420)]),
        ("outside_late", 1, [row(111.5, 10), row(112.5, 20)]),
        ("outside_early", 1, [row(99.5, 10), row(100.5, 20)]),
        ("bad_stamps", 1, [row(-1, 10), row(-1, 12), row(105, 14), row(105, 15), row(105.5, 16)]),
        ("too_far_apart", 1, [row(100.5, 10), row(109, 20)]),
        ("other_direction", -1, [row(103, 300, y=66), row(103.5, 250, y=66)]),
        ("direction_zero", [1, -1], [row(108, 130), row(108.5, 140)]),
        ("inexact", 1, [row(100.1, 0.3), row(100.7, 77.7), row(101.3, 131.9), row(103.9, 333.3)]),
    ]
    offsets, cols, direction = pack([t[2] for t in tr], [t[1] for t in tr])
    return offsets, cols, direction, [t[0] for t in tr]


def many_scene(seed=5):
    """65 and 300 segments in one tracklet and 65 short tracklets, inexact numbers, both directions, every lane and none: past a
    wave and past a workgroup -> (offsets, cols, direction, frame)."""
    rng = np.random.default_rng(seed)
    tracks, dirs = [], []
    for n in [66, 301] + [int(v) for v in rng.integers(2, 6, 65)]:
        sgn = 1 if rng.random() < 0.5 else -1
        t = 1000.0 + rng.integers(0, 300) / 30.0 + np.cumsum(rng.choice([1, 1, 1, 2, 40], n)) / 30.0
        x = (0.0 if sgn == 1 else 2000.0) + sgn * np.cumsum(rng.normal(3.0, 1.5, n))
        y = (30.0 if sgn == 1 else 90.0) + rng.normal(0.0, 18.0) + np.cumsum(rng.normal(0.0, 0.4, n))
        tracks.append(np.stack([np.round(t, 4), x, y, rng.uniform(12, 60, n), np.full(n, 6.0), np.full(n, 5.0), rng.normal(60, 40, n)], axis=1))
        dirs.append(sgn)
    offsets, cols, direction = pack(tracks, dirs)
    return offsets, cols, direction, frames_of(cols)


LEADER_FRAMES = (0, 1, 2, 65, 300)


def leader_edge_scene(seed=11):
    """Frames of 0, 1, 2, 65 and 300 rows (vehicle j is in the frames with more than j rows).  x comes from 40 values and the lanes
    from 6 + none per direction, so equal x, equal spacings, overlaps (l up to 60 at spacings from 8), v <= 0, lane -1 and the same
    lane index under both directions all occur; test_traffic_host.py checks that they do.
    -> (offsets, cols, direction, frame_off, frame_rows)."""
    rng = np.random.default_rng(seed)
    tracks, dirs, frames = [], [], []
    for j in range(max(LEADER_FRAMES)):
        fs = [f for f, n in enumerate(LEADER_FRAMES) if j < n]
        sgn = 1 if j % 3 else -1
        y = (0.0 if sgn == 1 else 60.0) + rng.choice([6.0, 18.0, 30.0, 42.0, 54.0, 200.0], len(fs))
        v = rng.choice([0.0, -1.0, 40.0, 64.0, 64.0, 90.5], len(fs))
        tracks.append(np.stack([100.0 + np.asarray(fs, np.float64), rng.integers(0, 40, len(fs)) * 8.0, y, rng.choice([12.0, 16.0, 60.0], len(fs)),
                                np.full(len(fs), 6.0), np.full(len(fs), 5.0), v], axis=1))
        dirs.append(sgn)
        frames += fs
    offsets, cols, direction = pack(tracks, dirs)
    frame_off, frame_rows = frames_csr(frames)
    return offsets, cols, direction, frame_off, frame_rows


def golden_scene(g):
    """The reference's shipped tracking output (tests/golden/track_stitch.npz), all of it."""
    return np.asarray(g["offsets"], np.int64), np.asarray(g["cols"], np.float64), np.asarray(g["direction"], np.int32), np.asarray(g["frame"], np.int64)


GOLDEN_PARAMS = {"dx": 50.0, "dt": 2.0, "max_gap": 1.0}
GOLDEN_COUNTS = dict(segments=6684, used=6645, skipped_gap=3, skipped_lane=36)     # exact; at most 3 pieces per segment, 575 cells


def as_data_frames(offsets, cols, direction, ids, frame):
    """The packed arrays as ``Data_Reader.data`` with every row in the frame ``frame`` names and its time stamp untouched (the shipped
    output holds several rows stamped -1 under one id: grouping by time stamp would merge them)."""
    data = [{} for _ in range(int(np.max(frame)) + 1 if len(frame) else 0)]
    for i in range(len(offsets) - 1):
        for r in range(int(offsets[i]), int(offsets[i + 1])):
            item = {"id": int(ids[i]), "timestamp": float(cols[r, 0]), "class": "sedan", "camera": "p1c1", "direction": int(direction[r]),
                    "ts_bias": {"p1c1": 0.0}, "frame": "0"}
            item.update(zip(("x", "y", "l", "w", "h", "v"), (float(v) for v in cols[r, 1:7])))
            assert int(ids[i]) not in data[int(frame[r])]
            data[int(frame[r])][int(ids[i])] = item
    return data

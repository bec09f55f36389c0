"""Scripted label sets, a synthetic pair of homographies and a plain numpy restatement of the label re-basing passes
(label_rewrite.py / csrc/label_rebase.hip): replace_homgraphy, replace_y / offset_box_y and replace_timestamps of the
reference's annotator.  No GPU, no package import: tools/make_golden_label_rewrite.py runs the reference's own methods on
``golden_scenes()`` (-> tests/golden/label_rewrite.npz), the tests rebuild the same scenes here, and the restatement is the
oracle of the kernel's edge cases and of the fuzz scene.

The restatement is written one IEEE operation per numpy call, in the reference's order: float32 scalars for the old box (the
reference builds it with torch.tensor of Python floats), float64 arrays over the grid's candidates whose corner sums are
rounded once to float32 (the reference writes them into a float32 tensor), float64 for the projection and the error.  numpy
rounds every elementwise operation once and never fuses two, so arrays over the candidates compute what scalars would.

golden_scenes():
  "rebase"  4 cameras, 36 frames, last_frame 30, ids 0..4 and 7 (5 is the first unused id: 7 is ignored).  Every third box is
            "Manual", the others "Interpolation" (dropped and re-interpolated).  id 1 drives at y = 55: its grid straddles the
            y > 60 switch of the wrapper, whose two sides differ; ids 2 and 3 drive west (direction -1, y > 60).  The new
            homography perturbs every P of the old one, per camera and per side.
  "curve"   3 cameras, 30 frames, last_frame 20 and an empty frame 25 (the break of replace_y), boxes without "gen" beside
            manual and interpolated ones, both directions, one manual box behind the break."""
import copy

import numpy as np

import label_audit_cases as lc

F32, F64 = np.float32, np.float64
SEARCH_RAD, GRID = 50, 11
STATE_KEYS = ("x", "y", "l", "w", "h", "direction")


# ------------------------------------------------------------------------------------------------ homographies
class Side():
    """What the passes read of a Homography: ``correspondence[camera]["P"]`` and ``["space_pts"]``."""

    def __init__(self):
        self.correspondence = {}


class Pair():
    def __init__(self, hg1=None, hg2=None):
        self.hg1, self.hg2 = hg1, hg2


def camera_P(c, side):
    """A camera that looks down on x in [60 c - 15, 60 c + 85]: pixels grow with x (u) and y (v), mild perspective."""
    x0 = 60.0 * c + 35.0
    s = 0.1 * side
    return np.array([[14.0 + s, 2.0 - s, 0.5, 900.0 - (14.0 + s) * x0],
                     [1.5 - s, 9.0 + 2 * s, -10.0, 200.0 + 30.0 * side - (1.5 - s) * x0],
                     [0.003, 0.004 - 0.01 * s, 0.0005, 1.0 - 0.003 * x0]], np.float64)


def hg_spec(names, seed=None, scale=0.004):
    """{"P1": {camera: P}, "P2": ..., "space_pts": {camera: [n,2]}}; seed: every entry of every P perturbed by up to
    ``scale`` of itself, per camera and per side."""
    rng = None if seed is None else np.random.RandomState(seed)
    spec = {"P1": {}, "P2": {}, "space_pts": {}}
    for c, n in enumerate(names):
        for side, key in enumerate(("P1", "P2")):
            P = camera_P(c, side)
            if rng is not None:
                P = P * (1.0 + rng.uniform(-scale, scale, P.shape))
            spec[key][n] = P
        spec["space_pts"][n] = np.array([[60.0 * c, 72.0 + 0.5 * c], [60.0 * c + 40.0, 120.0]], np.float64)
    return spec


def build_hg(spec, side_cls=Side, pair_cls=Pair):
    """The wrapper of a spec out of any pair of classes: the stand-ins above, the package's, the reference's."""
    sides = []
    for key in ("P1", "P2"):
        hg = side_cls()
        for n, P in spec[key].items():
            hg.correspondence[n] = {"P": P.copy(), "space_pts": spec["space_pts"][n].copy()}
        sides.append(hg)
    return pair_cls(hg1=sides[0], hg2=sides[1])


class Labels(lc.Labels):
    """lc.Labels with ``hg`` = the scene's old homography."""

    def __init__(self, scene, side_cls=Side, pair_cls=Pair):
        lc.Labels.__init__(self, scene)
        self.hg = build_hg(scene["hg_old"], side_cls, pair_cls)


# ------------------------------------------------------------------------------------------------ scenes
def drive(s, oid, f0, n, x0, dx, y, manual_every=3, gens=("Manual", "Interpolation"), cams=None):
    """An object along x through the cameras that see it; every ``manual_every``-th box of a camera is gens[0]."""
    for c in range(len(s["names"])) if cams is None else cams:
        k = 0
        for f in range(f0, f0 + n):
            x = x0 + dx * (f - f0)
            if 60.0 * c - 15.0 <= x <= 60.0 * c + 85.0:
                lc.put(s, f, c, oid, x + 0.03 * c, y + 0.02 * (f - f0) + 0.05 * c, cls=oid,
                       gen=gens[0] if k % manual_every == 0 else gens[1])
                k += 1


def scene_rebase():
    s = lc.empty_scene(4, 36, seed=21, last_frame=30)
    drive(s, 0, 0, 36, -5.0, 6.1, 30.0)
    drive(s, 1, 2, 30, 20.0, 5.3, 55.0)                         # straddles y > 60
    drive(s, 2, 1, 34, 250.0, -6.7, 84.0)                       # west
    drive(s, 3, 5, 25, 180.0, -4.9, 100.0, manual_every=2)
    drive(s, 4, 0, 36, 40.0, 3.7, 12.0, manual_every=4)
    drive(s, 7, 3, 10, 10.0, 5.0, 40.0)                         # above the first unused id (5)
    s["hg_old"] = hg_spec(s["names"])
    s["hg_new"] = hg_spec(s["names"], seed=31, scale=0.04)      # far enough that every round of the search moves
    return s


def scene_curve():
    s = lc.empty_scene(3, 30, seed=22, last_frame=20)
    drive(s, 0, 0, 30, 0.0, 5.9, 35.0, gens=(None, "Interpolation"))
    drive(s, 1, 0, 30, 170.0, -5.2, 90.0, gens=("Manual", "Interpolation"))
    drive(s, 2, 4, 20, 30.0, 4.4, 20.0, manual_every=2, gens=("Manual", None))
    s["data"][25] = {}                                          # the walk of replace_y ends here; frames 26.. are lost
    s["hg_old"] = hg_spec(s["names"])
    s["hg_new"] = hg_spec(s["names"], seed=32)
    return s


def golden_scenes():
    return {"rebase": scene_rebase(), "curve": scene_curve()}


def fuzz_scene(seed):
    """About 3 cameras x 40 frames x 6 ids of lc.fuzz_scene's traffic; one box in three manual, the others interpolated."""
    rng = np.random.RandomState(500 + seed)
    s = lc.fuzz_scene(seed)
    for fd in s["data"]:
        for item in fd.values():
            item["gen"] = "Manual" if rng.rand() < 0.34 else "Interpolation"
    s["hg_old"] = hg_spec(s["names"], seed=600 + seed, scale=0.002)
    s["hg_new"] = hg_spec(s["names"], seed=700 + seed, scale=0.04)
    return s


# ------------------------------------------------------------------------------------------------ restatement: the search
def radii(search_rad=SEARCH_RAD):
    out = []
    while search_rad > 1:                                       # :1684, :1706
        out.append(search_rad)
        search_rad /= 5
    return out


def linspace(start, stop, n):
    """np.linspace restated: step = (stop - start) / (n - 1), element k = k * step + start, the last element is stop."""
    step = (F64(stop) - F64(start)) / F64(n - 1)
    out = np.arange(n).astype(F64) * step
    out = out + F64(start)
    out[-1] = stop
    return out


def project(P, X, Y, Z):
    """homography.py:438-476 on fp64 values: one row of P at a time, products added left to right, then the divide."""
    u = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3]
    v = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7]
    w = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11]
    return u / w, v / w


def old_footprint(state, P1, P2):
    """:1677-1678 -> the image of the four bottom corners, [(u, v)] * 4: a float32 state, float32 corners."""
    x, y, l, w, h, d = (F32(v) for v in state)
    xf = x + d * l
    half = d * w / F32(2.0)
    ylo, yhi = y - half, y + half
    P = P2 if P2 is not None and ylo > F32(60.0) else P1
    return [project(P, F64(cx), F64(cy), F64(0.0)) for cx, cy in ((xf, ylo), (xf, yhi), (x, ylo), (x, yhi))]


def round_errors(cx, cy, rad, grid, state, old_im, P1, P2):
    """One round (:1685-1701) -> (x [grid], y [grid], error [grid * grid], candidate = ix * grid + iy)."""
    l, w, h, d = (F64(v) for v in state[2:])
    xs, ys = linspace(cx - rad, cx + rad, grid), linspace(cy - rad, cy + rad, grid)
    X, Y = np.repeat(xs, grid), np.tile(ys, grid)
    xf, xr = (X + d * l).astype(F32), X.astype(F32)             # fp64 sums, rounded once to float32
    half = d * w / F64(2.0)
    ylo, yhi = (Y - half).astype(F32), (Y + half).astype(F32)
    use2 = (ylo > F32(60.0)) if P2 is not None else np.zeros(len(X), bool)
    Z = np.zeros(len(X), F64)
    total = None
    for k, (ax, ay) in enumerate(((xf, ylo), (xf, yhi), (xr, ylo), (xr, yhi))):
        u, v = project(P1, ax.astype(F64), ay.astype(F64), Z)
        if use2.any():
            u2, v2 = project(P2, ax.astype(F64), ay.astype(F64), Z)
            u, v = np.where(use2, u2, u), np.where(use2, v2, v)
        dx, dy = u - old_im[k][0], v - old_im[k][1]
        m = (dx * dx + dy * dy) / F64(2.0)
        total = m if total is None else total + m
    return xs, ys, total / F64(4.0)


def rebase_boxes(state6, cam, P1_old, P2_old, P1_new, P2_new, rads=None, grid=GRID):
    """What ops.label_rebase returns: state6 fp64 [n,6], cam [n], P* fp64 [C,12] (P2*: or None) -> (centre fp64 [n,2], err
    fp64 [n], idx int32 [n, rounds], errors per box and round).  A camera outside the tables: NaN, NaN, -1."""
    rads = radii() if rads is None else rads
    n = len(state6)
    centre, err, idx = np.full((n, 2), np.nan), np.full(n, np.nan), np.full((n, len(rads)), -1, np.int32)
    every = []
    with np.errstate(all="ignore"):
        for b in range(n):
            m = int(cam[b])
            every.append([])
            if not 0 <= m < len(P1_old):
                continue
            pick = lambda T: None if T is None else T[m].reshape(12)
            old_im = old_footprint(state6[b], pick(P1_old), pick(P2_old))
            cx, cy = F64(state6[b][0]), F64(state6[b][1])
            for r, rad in enumerate(rads):
                xs, ys, e = round_errors(cx, cy, F64(rad), grid, state6[b], old_im, pick(P1_new), pick(P2_new))
                i = int(np.argmin(e))                           # the first smallest, as torch.argmin
                every[-1].append(e)
                if not np.isfinite(e[i]):                       # the kernel's refusal: the box is left out as a whole
                    cx = cy = np.nan
                    err[b], idx[b] = np.nan, -1
                    break
                idx[b, r] = i
                cx, cy = xs[i // grid], ys[i % grid]
                err[b] = e[i]
            centre[b] = (cx, cy)
    return centre, err, idx, every


def visit(me, n_frames):
    """(frame, key, datum) in the reference's order: frame, camera, id below the first unused one; truthy data only."""
    n_ids = lc.unused_id(me.data)
    for f in range(min(n_frames, len(me.data))):
        for cam in me.cameras:
            for oid in range(n_ids):
                key = "{}_{}".format(cam.name, oid)
                if me.data[f].get(key):
                    yield f, key, me.data[f][key]


def tables(hg, names):
    return [np.stack([np.asarray(side.correspondence[n]["P"], F64).reshape(12) for n in names]) for side in (hg.hg1, hg.hg2)]


def ref_replace_homgraphy(me, hg_new, grid=GRID):
    """-> (centre, err, idx, errors per box and round) of the manual boxes, in order; rewrites me.data and me.hg."""
    names = [c.name for c in me.cameras]
    boxes = [(f, key, obj) for f, key, obj in visit(me, me.last_frame + 1) if obj["gen"] == "Manual"]
    state6 = np.array([[float(o[k]) for k in STATE_KEYS] for _, _, o in boxes], F64).reshape(-1, 6)
    cam = [names.index(o["camera"]) for _, _, o in boxes]
    got = rebase_boxes(state6, cam, *(tables(me.hg, names) + tables(hg_new, names)), grid=grid)
    new = [{} for _ in range(min(me.last_frame + 1, len(me.data)))]
    for (f, key, obj), (x, y) in zip(boxes, got[0].tolist()):
        new[f][key] = dict(copy.deepcopy(obj), x=x, y=y)
    me.data, me.hg = new, hg_new
    lc.ref_interpolate(me)
    return got


# ------------------------------------------------------------------------------------------------ restatement: y, timestamps
def offset_y(x, y, coef, y_straight, direction, reverse):
    """:1792-1802 in fp64, one rounding per operation."""
    x, y = F64(x), F64(y)
    p2, p1, p0 = (F64(v) for v in coef)
    y_offset = (x * x * p2 + x * p1) + p0
    if direction == -1:
        y_offset = y_offset - F64(y_straight)
    return float(y + y_offset if reverse else y - y_offset)


def ref_offset_box_y(me, box, reverse=False):
    d = box["direction"]
    straight = me.hg.hg2.correspondence[box["camera"]]["space_pts"][0][1] if d == -1 else 0.0
    box["y"] = offset_y(box["x"], box["y"], me.poly_params[box["camera"] + ("_EB" if d == 1 else "_WB")], straight, d, reverse)
    return box


def ref_replace_y(me, reverse=False):
    stop = lc.visited(me.data, me.last_frame)
    new = [{} for _ in range(stop)]
    for f, key, obj in visit(me, stop):
        if "gen" not in obj or obj["gen"] == "Manual":
            new[f][key] = ref_offset_box_y(me, copy.deepcopy(obj), reverse)
    me.data = new
    lc.ref_interpolate(me)


def ref_replace_timestamps(me):
    start = [me.all_ts[0][k] for k in me.seq_keys]
    fps = [len(me.all_ts) / (me.all_ts[-1][k] - me.all_ts[0][k]) for k in me.seq_keys]
    for i, row in enumerate(me.all_ts):
        for j, k in enumerate(me.seq_keys):
            row[k] = start[j] + 1.0 / fps[j] * i
    new = []
    for f, fd in enumerate(me.data):
        new.append({})
        for key, item in fd.items():
            item["timestamp"] = me.all_ts[f][item["camera"]]
            if "gen" not in item or item["gen"] == "Manual":
                new[f][key] = copy.deepcopy(item)
    me.data = new
    lc.ref_interpolate(me)


# ------------------------------------------------------------------------------------------------ dumps (arrays only)
def all_have_gen(scene):
    return all("gen" in item for fd in scene["data"] for item in fd.values())


def dumped(out, tag, me, names):
    out[tag + "_idx"], out[tag + "_val"] = lc.dump(me.data, names)


def restated(name, scene):
    """Every array tools/make_golden_label_rewrite.py writes for one scene, from the restatement: {key: array}."""
    out, names = {}, scene["names"]
    if all_have_gen(scene):                                     # replace_homgraphy reads obj["gen"] of every datum
        me = Labels(scene)
        centre, err, idx, _ = ref_replace_homgraphy(me, build_hg(scene["hg_new"]))
        out["rebase_xy"], out["rebase_err"], out["rebase_win"] = centre, err, idx.astype(np.int64)
        dumped(out, "hg", me, names)
    for tag, reverse in (("y0", False), ("y1", True)):
        me = Labels(scene)
        ref_replace_y(me, reverse)
        dumped(out, tag, me, names)
    me = Labels(scene)
    boxes = [ref_offset_box_y(me, copy.deepcopy(o), rev) for rev in (False, True) for _, _, o in visit(me, len(me.data))]
    out["box_y"] = np.array([b["y"] for b in boxes], F64).reshape(-1)
    me = Labels(scene)
    ref_replace_timestamps(me)
    dumped(out, "ts", me, names)
    out["ts_table"] = lc.ts_table(me.all_ts, names)
    return {name + "_" + k: v for k, v in out.items()}

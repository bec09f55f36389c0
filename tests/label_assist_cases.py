"""Scripted scenes, fuzz generators and a plain numpy restatement of the annotator's detector-assisted labelling path
(label_assist.py / csrc/label_assist.hip): box_to_state, find_box, copy_paste, paste_in_2D_bbox, the crop window and the
best-anchor pick of crop_detect, and automate of the reference's manual_annotator_state_v3.py.  No GPU, no package import:
tools/make_golden_label_assist.py runs the reference's own methods on ``golden_scripts()`` (-> tests/golden/label_assist.npz),
the tests replay the same scripts here, and the restatement is the oracle of the kernels' edge cases and of the fuzz.

Arithmetic kinds, one IEEE operation per numpy call, in the reference's order:
  float64  the camera matrices and everything inside state_to_im / im_to_space (products added left to right, one divide);
  float32  everything else: the centre (box_to_state(...).mean), np.linspace of float32 torch scalars (arange * step + start,
           the last element stop), the candidate state and its corners, the 2D extent (the float64 min / max rounded once on
           assignment into a float32 tensor), the difference to the target (an int64 target is converted to float32 first), the
           squares, their sum in index order 0, 1, 2, 3 and the division by 4; the crop window; the best anchor's box.
numpy rounds every elementwise operation once and never fuses two, so arrays over the candidates compute what scalars would."""
import copy

import numpy as np

import label_audit_cases as lc
import label_rewrite_cases as rc

F32, F64 = np.float32, np.float64
SEARCH_RAD, GRID = 50, 11
BAD_CAMERA, BAD_ERROR = 8, 16
FRAME_W, FRAME_H = 1920, 1080
STATE_KEYS = rc.STATE_KEYS
GEN_CODES = {None: 0, "Interpolation": 1, "Manual": 2}


# ------------------------------------------------------------------------------------------------ homographies
def inverse3(M):
    """The inverse of a 3 x 3 matrix by its adjugate, in plain float64 operations: the same bits on every machine."""
    a, b, c, d, e, f, g, h, i = (F64(v) for v in np.asarray(M, F64).reshape(9))
    A, B, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = (a * A + b * B) + c * C
    adj = np.array([[A, -(b * i - c * h), b * f - c * e], [B, a * i - c * g, -(a * f - c * d)], [C, -(a * h - b * g), a * e - b * d]])
    return adj / det


def hg_spec(names, seed=None, scale=0.004):
    """rc.hg_spec plus "H1" / "H2": the image -> road plane matrices that undo columns 0, 1 and 3 of every P."""
    spec = rc.hg_spec(names, seed, scale)
    for side in ("1", "2"):
        spec["H" + side] = {n: inverse3(P[:, [0, 1, 3]]) for n, P in spec["P" + side].items()}
    return spec


def build_hg(spec, side_cls=rc.Side, pair_cls=rc.Pair):
    hg = rc.build_hg(spec, side_cls, pair_cls)
    for side, key in ((hg.hg1, "H1"), (hg.hg2, "H2")):
        for n, H in spec[key].items():
            side.correspondence[n]["H"] = H.copy()
    return hg


def tables(hg, names, key="P"):
    return [np.stack([np.asarray(s.correspondence[n][key], F64).reshape(-1) for n in names]) for s in (hg.hg1, hg.hg2)]


class Labels(rc.Labels):
    """rc.Labels with the "H" of every camera in ``hg``, plus what the assisted path reads of the annotator: the view, the
    clicked camera, the copied box, the frame buffer."""

    def __init__(self, scene, side_cls=rc.Side, pair_cls=rc.Pair):
        rc.Labels.__init__(self, scene, side_cls, pair_cls)
        self.hg = build_hg(scene["hg_old"], side_cls, pair_cls)
        self.frame_idx = scene.get("frame_idx", 0)
        self.active_cam = 0
        self.clicked_camera = self.seq_keys[0]
        self.copied_box = None
        self.AUTO = False
        self.buffer_frame_idx = 0
        self.buffer = [[(np.zeros((2, 2, 3), np.uint8),) for _ in self.seq_keys]]


# ------------------------------------------------------------------------------------------------ restatement: projections
def corners32(state):
    """homography.py:305-320 on float32 arrays -> x, y, z of the eight corners, lists of float32 arrays."""
    x, y, l, w, h, d = state
    xf = x + d * l
    half = d * w / F32(2.0)
    ylo, yhi = y - half, y + half
    zt, z0 = -h, np.zeros_like(h)
    return ([xf, xf, x, x] * 2, [ylo, yhi, ylo, yhi] * 2, [z0] * 4 + [zt] * 4)


def state_to_extent(state, P1, P2):
    """state_to_im of float32 states ([6] arrays of equal length) through the wrapper, then the 2D extent as the reference
    stores it: min / max over the eight float64 corners, rounded once to float32 -> (x1, y1, x2, y2)."""
    X, Y, Z = corners32(state)
    use2 = (Y[0] > F32(60.0)) if P2 is not None else np.zeros(np.shape(Y[0]), bool)
    us, vs = [], []
    for k in range(8):
        a = [c.astype(F64) for c in (X[k], Y[k], Z[k])]
        u, v = rc.project(P1, *a)
        if np.any(use2):
            u2, v2 = rc.project(P2, *a)
            u, v = np.where(use2, u2, u), np.where(use2, v2, v)
        us.append(u)
        vs.append(v)
    return [f(np.stack(c), axis=0).astype(F32) for f, c in ((np.min, us), (np.min, vs), (np.max, us), (np.max, vs))]


def im_to_xy(H1, H2, u, v):
    """im_to_state of one image point repeated over the eight corners, height 0 -> float32 (x, y): homography.py:388-435 in
    float64 with the wrapper switch on hg1's y, then i24_space_to_state's sums of equal terms, rounded once to float32."""
    u, v = F64(u), F64(v)

    def through(H):
        H = np.asarray(H, F64).reshape(9)
        a, b, w = (H[0] * u + H[1] * v) + H[2], (H[3] * u + H[4] * v) + H[5], (H[6] * u + H[7] * v) + H[8]
        return a / w, b / w
    x, y = through(H1)
    if H2 is not None and y > 60.0:
        x, y = through(H2)
    return F32((x + x) / F64(2.0)), F32((((y + y) + y) + y) / F64(4.0))


def view_camera(me, x0):
    """The > 1920 rule of box_to_state / find_box -> (camera name, shift)."""
    return (me.seq_keys[me.active_cam + 1], True) if x0 > 1920 else (me.seq_keys[me.active_cam], False)


def _H(me, cam):
    return me.hg.hg1.correspondence[cam]["H"], me.hg.hg2.correspondence[cam]["H"]


def _P(me, cam):
    return (np.asarray(me.hg.hg1.correspondence[cam]["P"], F64).reshape(12),
            np.asarray(me.hg.hg2.correspondence[cam]["P"], F64).reshape(12))


def ref_box_to_state(me, point):
    """:521-543 -> float32 [2,2]."""
    point = point.copy()
    cam, shift = view_camera(me, point[0])
    if shift:
        point[0] -= 1920
        point[2] -= 1920
    H1, H2 = _H(me, cam)
    return np.array([im_to_xy(H1, H2, point[0], point[1]), im_to_xy(H1, H2, point[2], point[3])], F32)


def ref_find_box(me, point):
    """:1005-1028: the first smallest float32 squared distance over the frame's dict order."""
    point = point.copy()
    cam, shift = view_camera(me, point[0])
    if shift:
        point[0] -= 1920
    sx, sy = im_to_xy(*_H(me, cam), point[0], point[1])
    min_dist, min_id = np.inf, None
    for box in me.data[me.frame_idx].values():
        dx, dy = F32(box["x"]) - sx, F32(box["y"]) - sy
        dist = dx * dx + dy * dy
        if dist < min_dist:
            min_dist, min_id = dist, box["id"]
    return min_id


def ref_copy_paste(me, point, detect=None):
    """:798-848."""
    if me.copied_box is None:
        obj_idx = ref_find_box(me, point)
        if obj_idx is None:
            return
        sp = ref_box_to_state(me, point)[0]
        obj = me.data[me.frame_idx].get("{}_{}".format(me.clicked_camera, obj_idx))
        if obj is None:
            return
        me.copied_box = (obj_idx, obj.copy(), [sp[0], sp[1]])
    else:
        sp = ref_box_to_state(me, point)[0]
        obj_idx = me.copied_box[0]
        new_obj = copy.deepcopy(me.copied_box[1])
        new_obj["x"] = float(F32(new_obj["x"]) + (sp[0] - me.copied_box[2][0]))
        new_obj["y"] = float(F32(new_obj["y"]) + (sp[1] - me.copied_box[2][1]))
        new_obj["timestamp"] = me.all_ts[me.frame_idx][me.clicked_camera]
        new_obj["camera"] = me.clicked_camera
        new_obj["gen"] = "Manual"
        me.data[me.frame_idx]["{}_{}".format(me.clicked_camera, obj_idx)] = new_obj
        if me.AUTO:
            ref_automate(me, obj_idx, detect)
            me.AUTO = False


# ------------------------------------------------------------------------------------------------ restatement: the search
def radii(search_rad=SEARCH_RAD):
    return rc.radii(search_rad)


def linspace32(start, stop, n):
    """np.linspace of two 0-d float32 torch tensors: torch evaluates arange * step + start in float32, the last is stop."""
    start, stop = F32(start), F32(stop)
    step = (stop - start) / F32(n - 1)
    out = np.arange(n).astype(F32) * step
    out = out + start
    out[-1] = stop
    return out


def fit_round(cx, cy, rad, grid, tmpl, target, P1, P2):
    """One round (:606-627) -> (x [grid], y [grid], error float32 [grid * grid]); candidate = ix * grid + iy."""
    cx, cy, rad = F32(cx), F32(cy), F32(rad)
    xs, ys = linspace32(cx - rad, cx + rad, grid), linspace32(cy - rad, cy + rad, grid)
    X, Y = np.repeat(xs, grid), np.tile(ys, grid)
    state = [X, Y] + [np.full(len(X), F32(v), F32) for v in tmpl]
    ext = state_to_extent(state, P1, P2)
    total = None
    for k in range(4):
        d = ext[k] - F32(target[k])
        sq = d * d
        total = sq if total is None else total + sq
    return xs, ys, total / F32(4.0)


def fit_boxes(tmpl, cam, centre, target, P1, P2, rads=None, grid=GRID):
    """What ops.label_fit_box2d returns: tmpl float32 [n,4] = (l, w, h, direction), cam [n], centre float32 [n,2], target float32
    [n,4], P* float64 [C,12] (P2: or None) -> (centre float32 [n,2], err float32 [n], idx int32 [n, rounds], status, the errors
    per box and round).  A camera outside the tables or a winning error that is not finite: NaN, NaN, -1 and a status bit."""
    rads = radii() if rads is None else rads
    n = len(tmpl)
    out_c, err, idx = np.full((n, 2), np.nan, F32), np.full(n, np.nan, F32), np.full((n, len(rads)), -1, np.int32)
    status, every = 0, []
    with np.errstate(all="ignore"):
        for b in range(n):
            m = int(cam[b])
            every.append([])
            if not 0 <= m < len(P1):
                status |= BAD_CAMERA
                continue
            cx, cy = F32(centre[b][0]), F32(centre[b][1])
            won = []
            for r, rad in enumerate(rads):
                xs, ys, e = fit_round(cx, cy, rad, grid, tmpl[b], target[b], P1[m].reshape(12), None if P2 is None else P2[m].reshape(12))
                i = int(np.argmin(e))                           # the first smallest; a NaN counts as smallest, as torch.argmin
                every[-1].append(e)
                if not np.isfinite(e[i]):
                    status |= BAD_ERROR
                    won = None
                    break
                won.append(i)
                cx, cy = xs[i // grid], ys[i % grid]
                last = e[i]
            if won is not None:
                out_c[b], err[b], idx[b] = (cx, cy), last, won
    return out_c, err, idx, status, every


def ref_paste_in_2D_bbox(me, box, grid=GRID):
    """:588-642 -> [(errors, winning index)] per round, or None without a copied box."""
    if me.copied_box is None:
        return None
    base = me.copied_box[1].copy()
    st = ref_box_to_state(me, box)
    centre = np.array([(st[0, 0] + st[1, 0]) / F32(2.0), (st[0, 1] + st[1, 1]) / F32(2.0)], F32)
    if box[0] > 1920:
        box[[0, 2]] -= 1920
    P1, P2 = _P(me, me.clicked_camera)
    tmpl = np.array([[base[k] for k in STATE_KEYS[2:]]], F32)
    c, _, idx, status, every = fit_boxes(tmpl, [0], centre[None], box.astype(F32)[None], P1[None], P2[None], grid=grid)
    assert status == 0
    base["x"], base["y"] = float(c[0, 0]), float(c[0, 1])
    base["camera"] = me.clicked_camera
    base["gen"] = "Manual"
    base["timestamp"] = me.all_ts[me.frame_idx][me.clicked_camera]
    me.data[me.frame_idx]["{}_{}".format(me.clicked_camera, base["id"])] = base
    return [(e, int(i)) for e, i in zip(every[0], idx[0])]


# ------------------------------------------------------------------------------------------------ restatement: crop_detect
def crop_windows(state, cam, P1, P2, ber=1.2, width=FRAME_W, height=FRAME_H):
    """:662-673 and :707-717 for float32 states [n,6] -> (crop_box float32 [n,4], rois float32 [n,5], window float32 [n,3] =
    (minx, miny, scale), skipped uint8 [n], status).  A skipped box keeps NaN in rois and window."""
    n = len(state)
    crop, rois, win = np.full((n, 4), np.nan, F32), np.full((n, 5), np.nan, F32), np.full((n, 3), np.nan, F32)
    skipped, status = np.ones(n, np.uint8), 0
    with np.errstate(all="ignore"):
        for b in range(n):
            m = int(cam[b])
            if not 0 <= m < len(P1):
                status |= BAD_CAMERA
                continue
            s = [np.array([v], F32) for v in state[b]]
            x1, y1, x2, y2 = (v[0] for v in state_to_extent(s, P1[m].reshape(12), None if P2 is None else P2[m].reshape(12)))
            crop[b] = (x1, y1, x2, y2)
            if x1 < 0 or y1 < 0 or x2 > width or y2 > height:
                continue
            w, h = x2 - x1, y2 - y1
            scale = (h if h > w else w) * F32(ber)              # Python's max(w, h): w unless h > w
            half = scale / F32(2.0)
            mx, my = (x2 + x1) / F32(2.0), (y2 + y1) / F32(2.0)
            skipped[b] = 0
            rois[b] = (F32(m), mx - half, my - half, mx + half, my + half)
            win[b] = (mx - half, my - half, scale)
    return crop, rois, win, skipped, status


def best_anchor(cls, reg, win, cs):
    """:731-740: cls float32 [n,A,C], reg float32 [n,A,4], win float32 [n,3] = (minx, miny, scale) -> (box float32 [n,4], anchor
    int32 [n], confidence float32 [n], class int32 [n]).  torch.max / torch.argmax: a NaN counts as largest, equal values go to
    the lower index."""
    n, A, C = cls.shape
    box, anchor = np.zeros((n, 4), F32), np.zeros(n, np.int32)
    conf, klass = np.zeros(n, F32), np.zeros(n, np.int32)

    def first_largest(v):
        nan = np.nonzero(np.isnan(v))[0]
        return int(nan[0]) if len(nan) else int(np.argmax(v))
    with np.errstate(all="ignore"):
        for b in range(n):
            ks = [first_largest(cls[b, a]) for a in range(A)]
            confs = np.array([cls[b, a, k] for a, k in enumerate(ks)], F32)
            a = first_largest(confs)
            anchor[b], conf[b], klass[b] = a, confs[a], ks[a]
            v = reg[b, a].astype(F32) * F32(win[b, 2]) / F32(cs)
            box[b] = (v[0] + win[b, 0], v[1] + win[b, 1], v[2] + win[b, 0], v[3] + win[b, 1])
    return box, anchor, conf, klass


def scripted_detect(crop, delta):
    """The stand-in for crop_detect in the golden: the crop box moved by ``delta``, float32."""
    return (np.asarray(crop, F32) + np.asarray(delta, F32)).astype(F32)


def ref_automate(me, obj_idx, detect):
    """:644-697 -> {"crop_box", "box_2D", "skipped"} (None without the box); ``detect(c_idx, crop_box) -> float32 [4]``."""
    cam = me.clicked_camera
    prev = me.data[me.frame_idx].get("{}_{}".format(cam, obj_idx))
    if prev is None:
        return None
    names = [c.name for c in me.cameras]
    c_idx = names.index(cam) if cam in names else len(names) - 1
    P1, P2 = _P(me, cam)
    state = np.array([[prev[k] for k in STATE_KEYS]], F32)
    crop, _, _, skipped, _ = crop_windows(state, [0], P1[None], P2[None])
    crop_box = crop[0].copy()
    if skipped[0]:
        return {"crop_box": crop_box, "box_2D": None, "skipped": True}
    box_2D = np.asarray(detect(c_idx, crop_box.copy()), F32).copy()
    if me.active_cam != c_idx:
        crop_box[[0, 2]] += 1920
        box_2D[[0, 2]] += 1920
    ref_paste_in_2D_bbox(me, box_2D.copy())
    return {"crop_box": crop_box, "box_2D": box_2D, "skipped": False}


# ------------------------------------------------------------------------------------------------ scenes and scripts
def put(s, f, c, oid, x, y, l, w, h, gen="Manual", direction=None):
    lc.put(s, f, c, oid, x, y, cls=oid, gen=gen)
    item = s["data"][f]["{}_{}".format(s["names"][c], oid)]
    item["l"], item["w"], item["h"] = float(l), float(w), float(h)
    if direction is not None:
        item["direction"] = direction


def scene_assist():
    """4 cameras, 3 frames, everything in frame 1.  ids 0, 1 east (y < 60), 2, 3 west (y > 60), 4 east at y = 62.5 and 6 ft wide: its
    corner-0 y is y - 3, so its last round (radius 2) still straddles the wrapper switch at y = 63; ids 5..8 in camera 0 leave the frame by one
    edge each."""
    s = lc.empty_scene(4, 3, seed=41)
    s["frame_idx"] = 1
    for c in range(4):
        x0 = 60.0 * c + 35.0
        put(s, 1, c, 0, x0 - 20.0, 20.0 + c, 16.0, 6.5, 5.0)
        put(s, 1, c, 1, x0 + 15.0, 42.5, 22.0, 7.0, 7.5, gen="Interpolation")
        put(s, 1, c, 2, x0 + 30.0, 80.0 - c, 15.0, 6.0, 4.5)
        put(s, 1, c, 3, x0 - 5.0, 101.0, 48.0, 8.5, 12.0)
        put(s, 1, c, 4, x0 + 2.0, 62.5, 14.0, 6.0, 4.8, direction=1)
    put(s, 1, 0, 5, -40.0, 30.0, 16.0, 6.0, 5.0)                # x1 < 0
    put(s, 1, 0, 6, 20.0, -30.0, 16.0, 6.0, 5.0)                # y1 < 0
    put(s, 1, 0, 7, 250.0, 10.0, 16.0, 6.0, 5.0)                # x2 > 1920
    put(s, 1, 0, 8, 35.0, 250.0, 16.0, 6.0, 5.0)                # y2 > 1080
    s["hg_old"] = hg_spec(s["names"])
    return s


def image_point(me, cam, x, y):
    """The image of the road point (x, y) in ``cam``, rounded to whole pixels (what a click gives), int64 [2]."""
    P1, P2 = _P(me, cam)
    u, v = rc.project(P2 if y > 60.0 else P1, F64(x), F64(y), F64(0.0))
    return np.array([int(round(float(u))), int(round(float(v)))], np.int64)


def target_of(me, cam, obj, dx, dy, grow, dtype):
    """The 2D extent of ``obj`` moved by (dx, dy) on the road, grown by ``grow`` pixels: a box a labeller would draw."""
    state = [np.array([F32(v)], F32) for v in (obj["x"] + dx, obj["y"] + dy, obj["l"], obj["w"], obj["h"], obj["direction"])]
    x1, y1, x2, y2 = (float(v[0]) for v in state_to_extent(state, *_P(me, cam)))
    box = np.array([x1 - grow, y1 - grow, x2 + grow, y2 + grow])
    return np.round(box).astype(np.int64) if dtype == np.int64 else box.astype(F32)


def golden_script(scene):
    """The steps both sides replay on one Labels: (kind, arguments...).  Built from the scene alone."""
    me = Labels(scene)
    f, names = scene["frame_idx"], scene["names"]
    steps = []

    def at(c, oid):
        o = scene["data"][f]["{}_{}".format(names[c], oid)]
        return image_point(me, names[c], o["x"], o["y"])

    def four(c, oid, shift=0):
        p = at(c, oid)
        return np.array([p[0] + shift, p[1], p[0] + shift + 40, p[1] + 25], np.int64)
    # box_to_state / find_box in both views, int64 and float32 points
    steps.append(("view", 1, names[1]))
    for c, shift in ((1, 0), (2, 1920)):
        for oid in (0, 2, 4):
            steps.append(("box_to_state", four(c, oid, shift)))
            steps.append(("box_to_state", four(c, oid, shift).astype(F32) + F32(0.25)))
            steps.append(("find_box", four(c, oid, shift)))
    # copy and paste: first view, then the second view (clicked camera = the view's right half)
    steps += [("view", 1, names[1]), ("copy_paste", four(1, 0)), ("copy_paste", four(1, 0) + np.array([30, 12, 30, 12])), ("drop",)]
    steps += [("view", 1, names[2]), ("copy_paste", four(2, 3, 1920)), ("copy_paste", four(2, 3, 1920) + np.array([-25, 4, -25, 4])),
              ("drop",)]
    # paste_in_2D_bbox: both directions, the switch, both views, both target types
    k = 0
    for c, oid, dx, dy, view in ((0, 0, 7.3, -2.1, 0), (0, 2, -11.0, 3.4, 0), (1, 4, 1.7, 0.4, 1), (2, 3, 5.5, -1.5, 1),
                                 (3, 1, -6.2, 1.1, 2), (1, 2, 3.1, 2.2, 1), (2, 4, -0.8, 0.9, 1), (3, 0, 9.9, 4.0, 3)):
        cam = names[c]
        obj = scene["data"][f]["{}_{}".format(cam, oid)]
        for dtype in (np.int64, F32):
            box = target_of(me, cam, obj, dx, dy, 1.5 + 0.5 * k, dtype)
            if view != c:
                box[[0, 2]] += 1920
            steps += [("view", view, cam), ("copy_paste", four(c, oid, 1920 if view != c else 0)), ("paste2d", box), ("drop",)]
            k += 1
    # automate: in the view, in the second view, and the four edge tests
    for c, oid, view, delta in ((0, 0, 0, (3.5, -2.25, 6.0, 1.5)), (1, 2, 1, (-4.0, 2.0, -1.5, 3.0)), (2, 4, 1, (2.0, 1.0, 2.5, -1.0)),
                                (3, 3, 2, (-3.0, -2.0, 1.0, 2.0)), (1, 0, 0, (1.0, 1.0, -2.0, -1.0))):
        steps += [("view", view, names[c]), ("copy_paste", four(c, oid, 1920 if view != c else 0)), ("automate", oid, delta), ("drop",)]
    for oid in (5, 6, 7, 8):
        steps += [("view", 0, names[0]), ("copy", oid), ("automate", oid, (1.0, 1.0, 1.0, 1.0)), ("drop",)]
    return steps


def golden_scenes():
    return {"assist": scene_assist()}


def dump(data, names):
    """``data`` in dict order -> (index int64 [n,7] = (frame, camera, id, class, gen code, x is a Python float, y is one), values
    float64 [n,7] = (x, y, l, w, h, direction, timestamp))."""
    idx, val = [], []
    for f, fd in enumerate(data):
        for key, item in fd.items():
            assert key == "{}_{}".format(item["camera"], item["id"])
            idx.append((f, names.index(item["camera"]), item["id"], lc.CLASSES.index(item["class"]), GEN_CODES.get(item.get("gen"), 3),
                        int(type(item["x"]) is float), int(type(item["y"]) is float)))
            val.append([float(item[k]) for k in STATE_KEYS + ("timestamp",)])
    return np.array(idx, np.int64).reshape(-1, 7), np.array(val, F64).reshape(-1, 7)


def replay(me, steps, ops):
    """Runs a script on ``me`` with the functions of ``ops`` (a dict: box_to_state, find_box, copy_paste, paste2d -> rounds,
    automate(me, oid, detect) -> dict) -> the arrays of the golden file, {key: array}."""
    b2s, found, win, err, centre, auto_box, auto_skip = [], [], [], [], [], [], []
    for step in steps:
        kind = step[0]
        if kind == "view":
            me.active_cam, me.clicked_camera = step[1], step[2]
        elif kind == "drop":
            me.copied_box = None
        elif kind == "copy":                                    # a copied box without a click: find_box is not part of the case
            obj = me.data[me.frame_idx]["{}_{}".format(me.clicked_camera, step[1])]
            me.copied_box = (step[1], obj.copy(), [F32(0.0), F32(0.0)])
        elif kind == "box_to_state":
            b2s.append(np.asarray(ops["box_to_state"](me, step[1].copy()), F32).reshape(2, 2))
        elif kind == "find_box":
            got = ops["find_box"](me, step[1].copy())
            found.append(-1 if got is None else got)
        elif kind == "copy_paste":
            ops["copy_paste"](me, step[1].copy())
        elif kind == "paste2d":
            rounds = ops["paste2d"](me, step[1].copy())
            base_id = me.copied_box[1]["id"]
            item = me.data[me.frame_idx]["{}_{}".format(me.clicked_camera, base_id)]
            if rounds is not None:
                win.append([i for _, i in rounds])
                err.append([F32(e[i]) for e, i in rounds])
            centre.append((item["x"], item["y"]))
        elif kind == "automate":
            delta = step[2]
            got = ops["automate"](me, step[1], lambda c_idx, crop: scripted_detect(crop, delta))
            auto_skip.append(int(got["skipped"]))
            auto_box.append(np.concatenate([np.asarray(got["crop_box"], F32),
                                            np.full(4, np.nan, F32) if got["skipped"] else np.asarray(got["box_2D"], F32)]))
    names = [c.name for c in me.cameras]
    out = {"b2s": np.array(b2s, F32).reshape(-1, 2, 2), "found": np.array(found, np.int64), "win": np.array(win, np.int64),
           "err": np.array(err, F32), "centre": np.array(centre, F64).reshape(-1, 2),
           "auto_box": np.array(auto_box, F32).reshape(-1, 8), "auto_skip": np.array(auto_skip, np.int64)}
    out["data_idx"], out["data_val"] = dump(me.data, names)
    return out


RESTATED = {"box_to_state": ref_box_to_state, "find_box": ref_find_box, "copy_paste": ref_copy_paste,
            "paste2d": ref_paste_in_2D_bbox, "automate": ref_automate}


def restated(name, scene):
    got = replay(Labels(scene), golden_script(scene), RESTATED)
    return {name + "_" + k: v for k, v in got.items()}


# ------------------------------------------------------------------------------------------------ fuzz
def fuzz_fit(n, seed, n_cam=4, near_switch=False):
    """n boxes over ``n_cam`` interleaved cameras -> (tmpl, cam, centre, target, P1, P2): targets are the extents of the
    template a few feet away from the starting centre, so that every round of the search moves."""
    rng = np.random.RandomState(seed)
    names = lc.camera_names(n_cam)
    spec = rc.hg_spec(names, seed=seed, scale=0.002)
    P1, P2 = (np.stack([spec[k][m].reshape(12) for m in names]) for k in ("P1", "P2"))
    cam = (np.arange(n) % n_cam).astype(np.int32)
    tmpl = np.zeros((n, 4), F32)
    centre, target = np.zeros((n, 2), F32), np.zeros((n, 4), F32)
    for b in range(n):
        east = rng.rand() < 0.5
        y = rng.uniform(58.0, 62.0) if near_switch else (rng.uniform(8.0, 50.0) if east else rng.uniform(70.0, 110.0))
        x = 60.0 * cam[b] + 35.0 + rng.uniform(-30.0, 30.0)
        tmpl[b] = (rng.uniform(12.0, 50.0), rng.uniform(5.0, 8.5), rng.uniform(4.0, 13.0), 1.0 if east else -1.0)
        state = [np.array([F32(v)], F32) for v in (x + rng.uniform(-20, 20), y + rng.uniform(-8, 8), *tmpl[b])]
        ext = state_to_extent(state, P1[cam[b]], P2[cam[b]])
        target[b] = [v[0] for v in ext]
        centre[b] = (x, y)
    return tmpl, cam, centre, target, P1, P2


def fuzz_detector(n, A, C, seed):
    rng = np.random.RandomState(seed)
    cls = rng.uniform(0.0, 1.0, (n, A, C)).astype(F32)
    reg = rng.uniform(0.0, 112.0, (n, A, 4)).astype(F32)
    win = np.stack([rng.uniform(0, 1500, n), rng.uniform(0, 900, n), rng.uniform(40, 400, n)], axis=1).astype(F32)
    return cls, reg, win


def anchor_edge_cases():
    """{name: (cls, reg, win)}: anchor counts about the wave size and the 112 x 112 crop's own 2 394, one class and eight, the
    maximum in the last anchor, equal maxima, all scores equal, NaN and infinite scores."""
    cases = {}
    for A, C in ((1, 1), (63, 8), (64, 1), (65, 8), (2394, 8)):
        cases["fuzz_%d_%d" % (A, C)] = fuzz_detector(5, A, C, seed=A + C)
    cases["one_crop"] = fuzz_detector(1, 2394, 1, seed=5)
    cls, reg, win = fuzz_detector(5, 130, 8, seed=7)
    cls[0, 129, 3] = 2.0                                        # the maximum in the last anchor
    cls[1, [5, 70, 128], [2, 6, 1]] = 3.0                       # equal maxima: anchor 5 wins
    cls[2] = 0.5                                                # all scores equal: anchor 0, class 0
    cls[3, 77, 4] = np.nan                                      # a NaN counts as largest
    cls[4, 9, 2] = cls[4, 9, 5] = 4.0                           # equal classes inside the winning anchor: class 2
    cases["edges"] = (cls, reg, win)
    cls, reg, win = fuzz_detector(3, 70, 8, seed=8)
    cls[0, [3, 66], [1, 1]] = np.nan                            # two NaN: the first
    cls[1, 20, 6] = np.inf
    cls[2] = -np.inf
    cases["nonfinite"] = (cls, reg, win)
    return cases


def window_of(crop, ber=1.2):
    """:707-716 on a float32 crop box -> (minx, miny, maxx, maxy, scale), float32."""
    c = np.asarray(crop, F32)
    w, h = c[2] - c[0], c[3] - c[1]
    scale = (h if h > w else w) * F32(ber)
    half = scale / F32(2.0)
    mx, my = (c[2] + c[0]) / F32(2.0), (c[3] + c[1]) / F32(2.0)
    return mx - half, my - half, mx + half, my + half, scale


# ------------------------------------------------------------------------------------------------ the end-to-end scene
def small_scene(seed=51, H=64, W=96, cs=16, A=70, C=8):
    """3 cameras that look at 64 x 96 frames (the cameras of rc.camera_P, their pixels divided by 20), 4 boxes each in frame 0
    (both directions, one at the switch) plus one that leaves camera 0 to the left, random frames, and a script of LOCALIZE
    outputs per key: the best anchor holds the crop box in crop pixels, moved a little; the others hold noise."""
    rng = np.random.RandomState(seed)
    s = lc.empty_scene(3, 1, seed=seed)
    s["frame_idx"] = 0
    spec = rc.hg_spec(s["names"])
    for key in ("P1", "P2"):
        for n in spec[key]:
            spec[key][n][:2] *= 0.05
    for side in ("1", "2"):
        spec["H" + side] = {n: inverse3(P[:, [0, 1, 3]]) for n, P in spec["P" + side].items()}
    s["hg_old"] = spec
    for c in range(3):
        x0 = 60.0 * c + 35.0
        put(s, 0, c, 0, x0 - 20.0, 20.0 + c, 16.0, 6.5, 5.0)
        put(s, 0, c, 1, x0 + 5.0, 45.0, 22.0, 7.0, 7.5, gen="Interpolation")
        put(s, 0, c, 2, x0 + 25.0, 80.0 - c, 15.0, 6.0, 4.5)
        put(s, 0, c, 3, x0 - 8.0, 62.5, 14.0, 6.0, 4.8, direction=1)
    put(s, 0, 0, 4, -70.0, 30.0, 16.0, 6.0, 5.0)                # x1 < 0: skipped
    s["frames"] = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    s["cs"] = cs
    me = Labels(s)
    s["keys"] = list(s["data"][0])
    s["script"] = {}
    for key in s["keys"]:
        o = s["data"][0][key]
        state = [np.array([F32(o[k])], F32) for k in STATE_KEYS]
        crop = np.array([v[0] for v in state_to_extent(state, *_P(me, o["camera"]))], F32)
        minx, miny, _, _, scale = window_of(crop)
        cls = rng.uniform(0.0, 0.6, (A, C)).astype(F32)
        reg = rng.uniform(0.0, cs, (A, 4)).astype(F32)
        a = int(rng.randint(0, A))
        cls[a, int(rng.randint(0, C))] = 0.9
        local = (crop - np.array([minx, miny, minx, miny], F32)) / scale * F32(cs)
        reg[a] = local + rng.uniform(-0.4, 0.4, 4).astype(F32)
        s["script"][key] = (reg, cls)
    return s


def ref_crop_detect(crop, reg, cls, ber=1.2, cs=112):
    """:699-741 behind the detector: the window of ``crop``, the best anchor of one crop's LOCALIZE outputs -> float32 [4]."""
    minx, miny, _, _, scale = window_of(crop, ber)
    box, _, _, _ = best_anchor(cls[None], reg[None], np.array([[minx, miny, scale]], F32), cs)
    return box[0]


def ref_automate_keys(me, scene, keys):
    """copy_paste (a click on the box) + automate of every key, its camera the active view -> {key: automate's result}."""
    names = [c.name for c in me.cameras]
    out = {}
    for key in keys:
        o = me.data[me.frame_idx][key]
        cam, oid = o["camera"], o["id"]
        me.active_cam, me.clicked_camera, me.copied_box = names.index(cam), cam, None
        p = image_point(me, cam, o["x"], o["y"])
        ref_copy_paste(me, np.array([p[0], p[1], p[0] + 3, p[1] + 2], np.int64))
        assert me.copied_box is not None and me.copied_box[0] == oid
        reg, cls = scene["script"][key]
        out[key] = ref_automate(me, oid, lambda c_idx, crop: ref_crop_detect(crop, reg, cls, cs=scene["cs"]))
    return out

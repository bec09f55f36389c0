"""The step of the reference's annotator (``seems_to_be_working.py``, class ``Annotator``) that turns audited labels into
ground-truth trajectories, on the GPU: ``create_trajectory`` (:1137-1314), ``get_splines`` (:1338-1350), ``gen_trajectories``
(:1317-1336), ``adjust_ts_with_trajectories`` (:1353-1458) and the later annotator's ``adjust_boxes_with_trajectories``.

The functions take ``self`` exactly like the methods they replace and read the same attributes -- ``data``, ``seq_keys``,
``hg``, ``last_frame``, ``all_ts``, ``ts_bias``, ``splines`` -- so a maintainer binds them into the reference class unchanged::

    import label_trajectory
    for name in label_trajectory.METHODS:
        setattr(Annotator, name, getattr(label_trajectory, name))

or inherits ``LabelTrajectory`` (``get_unused_id`` comes from ``label_audit``).  Per object the reference builds 200 + 100
``scipy.interpolate.UnivariateSpline`` fits (FITPACK curfit), each from scratch for one smoothing factor, scores each and keeps
the first with the smallest error; ``get_splines`` does that object by object.  Here one pass over ``data`` packs every object's
boxes (``label_audit.pack_tracklets`` plus l, w, h, direction and the camera of every row), one copy sends them up, and
csrc/label_spline.hip does the rest: ``ops.label_box_weights`` (one thread per box), ``ops.spline_fit`` (one lane per (object,
axis, candidate): FITPACK's fpcurf restated in fp64 with one rounding per operation, in its order), ``ops.spline_select`` (one
workgroup per (object, axis): scores, the first smallest, the winner's knots, coefficients and error figures),
``ops.spline_eval`` (one thread per box for ``gen_trajectories``) and ``ops.label_ts_shift`` (one wave per (frame, camera)); one
copy brings the winners back.  All objects go through ONE batch of launches, in chunks that keep the fit's workspace inside
``WORKSPACE_BYTES``.  Knots, coefficients, ier and residual equal scipy's bit for bit on the scripted scenes
(``tests/golden/label_trajectory.npz``).  There is no CPU path: without a device every function raises.

Reference behaviour kept on purpose:
  * the fit is weighted with ``x_weight`` / ``y_weight``, pixels per foot: the box rounded to fp32, its fp32 corners through
    ``hg.state_to_im`` (which projects in fp64), differences of corner pairs, their mean, the norm, divided by the fp64 l / w;
  * the end-weighted ``x_weight2`` (x50 on the first and last box, x10 on the second and second-to-last; an index that occurs
    twice multiplies once) enters only the x candidates' SCORE; y candidates are scored with the plain ``y_weight``; with
    ``weight=False`` the x score starts from ones, the fits stay weighted;
  * ``interp`` is all ones, and ``tpex**2*sum(interp)`` is a numpy scalar times a 0-d int64 tensor, which torch computes in
    fp32: s = fp32(tpe * tpe) * fp32(n), widened;
  * the candidate smoothing factors are ``np.logspace(1, 0, 200)`` for x and ``np.logspace(2, 0, 100)`` for y;
  * a candidate is skipped when its value at 0 is NaN or its knot count exceeds the limit -- ``floor(duration) * complexity + 2``
    for x (the reference hard-codes 4), ``floor(duration) + 2`` for y -- and the comparison is a strict ``<``: the first
    smallest wins;
  * with ``metric != "ape"`` x is scored by ``sqrt(max)`` but y by ``mean(max)``, without the root;
  * ``duration < 3`` returns no spline, no boxes returns no spline, and if either axis ends without a spline both are None;
  * boxes are compiled frame-major up to ``last_frame``, cameras in ``seq_keys`` order, then sorted by timestamp;
  * for ier > 0 scipy warns and the reference still uses the spline: so does this (``Spline.ier`` keeps the code);
  * ``gen_trajectories`` without ``self.splines`` fits with ``metric="ape"`` (the default of the ``create_trajectory`` it
    calls) and does not keep the splines.
In ``adjust_ts_with_trajectories``: objects are kept by their x spline only; the spline value is rounded to fp32
(``torch.tensor`` of Python floats) before the fp64 subtraction from the label; the frame loop stops at the first empty frame
or past ``last_frame``; after the trial loop the reference's ``shift`` is the LAST trial (+max_shift), so ``running_error[c]``
grows by that value once per (frame, camera) that had a kept object -- a function of the counts alone, which makes the pass
parallel over (frame, camera); the repeated addition is reproduced in its order on the host, so the values are the same bits;
the shifts are ``np.linspace``'s.

Differences a caller can see: ``plot`` defaults to False and ``plot=True`` raises NotImplementedError (no
matplotlib here); ``verbose=False`` silences the prints; ``complexity`` is the later annotator's parameter; the splines are
``Spline`` objects, not scipy's; the scores are summed in ascending row order where numpy sums pairwise (the winner is the same
wherever the best two scores are further apart than rounding); ValueError, naming object and axis, BEFORE any device work for
a box whose l or w is not positive and finite or whose state is not finite, and for an object that passes the duration test
with fewer than k + 1 boxes (scipy raises there), and for a weight that is not positive and finite (the kernel's arithmetic
is run in numpy on the host for this check alone; the fits take the kernel's weights); k other than 2 and 3 is refused.

``adjust_boxes_with_trajectories`` is the later annotator's (``manual_annotator_state_v3.py:1440-1515``): the limits are l /
x_diff * max_shift_x and w / y_diff * max_shift_y with the diffs of ``ops.label_box_weights``, every spline value comes from one
``ops.spline_eval`` launch, the clamp and the in-place ``+=`` stay on the host in the reference's order.  It indexes
``self.splines`` with EVERY id of a frame, so an id without an entry raises IndexError (before any device work here); a y
spline without an x spline raises as the reference does; ``pixel_shifts`` are feet, despite the name.
"""
import copy
import math

import numpy as np
import torch

from datareader import _cuda, _download, _upload
from label_audit import _device, get_unused_id, pack_tracklets  # noqa: F401
from label_rewrite import _P_table, _sides
from retinanet_mi355x import ops

METHODS = ("create_trajectory", "get_splines", "gen_trajectories", "adjust_ts_with_trajectories", "adjust_boxes_with_trajectories")
WORKSPACE_BYTES = 256 << 20                                    # the budget of the fit's per-lane arrays, per chunk of objects
STATE_KEYS = ("x", "y", "l", "w", "h", "direction")


def tpe_x():
    return np.logspace(1, 0, 200)                               # :1235


def tpe_y():
    return np.logspace(2, 0, 100)                               # :1260


# ------------------------------------------------------------------------------------------------ the spline object
def _bspl(t, k, x, l):
    """FITPACK fpbspl with Python floats, the kernel's arithmetic; t 0-based, l 1-based."""
    h = [0.0] * (k + 2)
    hh = [0.0] * (k + 1)
    h[0] = 1.0
    for j in range(1, k + 1):
        hh[:j] = h[:j]
        h[0] = 0.0
        for i in range(1, j + 1):
            tli, tlj = t[l + i - 1], t[l + i - j - 1]
            if tli == tlj:
                h[i] = 0.0
            else:
                f = hh[i - 1] / (tli - tlj)
                h[i - 1] = h[i - 1] + f * (tli - x)
                h[i] = f * (x - tlj)
    return h


def _splev(t, c, k, x):
    n, k1 = len(t), k + 1
    nk1, l = n - k1, k1
    while not (x < t[l] or l == nk1):
        l += 1
    h = _bspl(t, k, x, l)
    sp = 0.0
    for j in range(k1):
        sp = sp + c[l - k1 + j] * h[j]
    return sp


class Spline():
    """What ``self.splines`` holds: callable like ``UnivariateSpline`` (a float, a list or an array; extrapolating), with
    ``get_knots()``, ``get_coeffs()``, ``get_residual()`` and ``t``, ``c``, ``k``, ``ier``.  Backed by host copies of t and c: a
    single point is evaluated on the host with the kernel's arithmetic, anything else by ``ops.spline_eval`` on the device."""

    def __init__(self, t, c, k, ier=0, fp=0.0, device=None):
        self.t = np.array(t, np.float64).reshape(-1)
        self.c = np.zeros(len(self.t), np.float64)
        self.c[:len(self.t) - k - 1] = np.asarray(c, np.float64).reshape(-1)[:len(self.t) - k - 1]
        self.k, self.ier, self.fp, self.device = int(k), int(ier), float(fp), device
        if self.k not in (2, 3) or len(self.t) < 2 * self.k + 2:
            raise ValueError("a Spline has k in (2, 3) and at least 2k + 2 knots")
        self._t, self._c = self.t.tolist(), self.c.tolist()

    def get_knots(self):
        return self.t[self.k:len(self.t) - self.k]

    def get_coeffs(self):
        return self.c[:len(self.t) - self.k - 1]

    def get_residual(self):
        return self.fp

    def __call__(self, x):
        if np.ndim(x) == 0:
            return np.array(_splev(self._t, self._c, self.k, float(x)), np.float64)
        x = np.asarray(x, np.float64)
        dev = _cuda(self.device)
        st, sc, snk = pack_splines([self])
        up = _upload(dev, [st, sc, snk, np.zeros(x.size, np.int32), x.reshape(-1)])
        return _download([ops.spline_eval(*up)])[0].reshape(x.shape)


def pack_splines(splines):
    """[Spline or None] -> (st fp64 [S, ncap], sc fp64 [S, ncap], snk int32 [S,2] = (n, k); n = 0 for None)."""
    ncap = max([6] + [len(s.t) for s in splines if s is not None])
    st, sc = np.zeros((len(splines), ncap), np.float64), np.zeros((len(splines), ncap), np.float64)
    snk = np.zeros((len(splines), 2), np.int32)
    for i, s in enumerate(splines):
        if s is not None:
            st[i, :len(s.t)], sc[i, :len(s.t)], snk[i] = s.t, s.c, (len(s.t), s.k)
    return st, sc, snk


# ------------------------------------------------------------------------------------------------ packing
def _seq_names(self):
    return list(self.seq_keys)


def pack_objects(self, ids):
    """One pass over ``data`` -> the boxes of the objects ``ids`` up to ``last_frame``, object by object, each sorted by
    timestamp (ties: frame, then camera in ``seq_keys`` order -- the reference's order of compilation): dict(off int64
    [len(ids) + 1], t, state6 fp64 [R,6], cam int32 [R], ids).  ValueError before anything else for a box whose state is not
    finite or whose l or w is not positive."""
    names = _seq_names(self)
    tab = pack_tracklets(self.data, names, ids)
    keep = np.nonzero(tab["frame"] <= self.last_frame)[0]
    slot, cam, frame = tab["slot"][keep], tab["cam"][keep], tab["frame"][keep]
    t = tab["cols"][keep, 2]
    order = np.lexsort((cam, frame, t, slot))
    keep, slot, cam, t = keep[order], slot[order], cam[order], t[order]
    state = np.zeros((len(keep), 6), np.float64)
    for r, src in enumerate(keep.tolist()):
        item = tab["items"][src]
        state[r] = [float(item[k]) for k in STATE_KEYS]
    bad = np.nonzero(~(np.isfinite(state).all(axis=1) & (state[:, 2] > 0) & (state[:, 3] > 0)))[0]
    if len(bad):
        r = int(bad[0])
        axis = "y" if np.isfinite(state[r, 2]) and state[r, 2] > 0 and not (np.isfinite(state[r, 3]) and state[r, 3] > 0) else "x"
        raise ValueError("object {}, axis {}: box {!r} has a state that is not finite or a length / width that is not positive: "
                         "its weight would not be positive and finite".format(tab["ids"][slot[r]], axis, tab["keys"][keep[r]]))
    off = np.zeros(len(tab["ids"]) + 1, np.int64)
    np.cumsum(np.bincount(slot, minlength=len(tab["ids"])), out=off[1:])
    return dict(off=off, t=np.ascontiguousarray(t), state6=state, cam=cam.astype(np.int32), ids=tab["ids"], names=names)


def smoothing(tpe, m):
    """:1236: fp32(tpe * tpe) * fp32(m), the product torch forms for ``tpex**2*sum(interp)``."""
    return (np.asarray(tpe, np.float64) * np.asarray(tpe, np.float64)).astype(np.float32) * np.float32(m)


def _end_multipliers(m):
    """(x50, x10) multipliers of :1220-1223 for a run of m rows; a duplicated index multiplies once."""
    m50, m10 = np.ones(m, np.float64), np.ones(m, np.float64)
    m50[[0, -1]] = 50.0
    m10[[1 % m, -2 % m]] = 10.0
    return m50, m10


def plan_fits(pack, y_order, x_order, complexity, tpex, tpey, budget=None):
    """The launch tables of every object that gets fits -> dict(groups [(object slot, axis)], chunks [dict(grp, waves, s,
    ncap)], m50, m10); ValueError for an object that passes the duration test with fewer than k + 1 boxes, or k outside (2, 3).
    Chunks keep the workspace inside ``budget`` bytes; a single group that needs more than the budget becomes a chunk of its
    own and exceeds it."""
    budget = WORKSPACE_BYTES if budget is None else int(budget)
    if x_order not in (2, 3) or y_order not in (2, 3):
        raise ValueError("spline orders other than 2 and 3 are not supported (x_order {}, y_order {})".format(x_order, y_order))
    off, t, R = pack["off"], pack["t"], len(pack["t"])
    m50, m10 = np.ones(R, np.float64), np.ones(R, np.float64)
    rows = []                                                   # (slot, axis, row0, m, k, ncap, s values)
    for j in range(len(off) - 1):
        lo, hi = int(off[j]), int(off[j + 1])
        m = hi - lo
        if m == 0:
            continue
        duration = t[hi - 1] - t[lo]
        if duration < 3:
            continue
        for axis, k in ((0, x_order), (1, y_order)):
            if m < k + 1:
                raise ValueError("object {}, axis {}: {} boxes over {:.3f} s, a spline of order {} needs {} (scipy raises here)"
                                 .format(pack["ids"][j], "xy"[axis], m, duration, k, k + 1))
        m50[lo:hi], m10[lo:hi] = _end_multipliers(m)
        dur = math.floor(duration)
        for axis, k, limit, tpe in ((0, x_order, dur * complexity + 2, tpex), (1, y_order, dur + 2, tpey)):
            ncap = int(min(math.floor(limit) + 2 * k, m + k + 1))
            rows.append((j, axis, lo + axis * R, m, k, max(ncap, 2 * k + 2), smoothing(tpe, m).astype(np.float64)))
    chunks, cur, waves, cap = [], [], 0, 6                      # a group larger than the budget is a chunk of its own, over budget
    for r in rows:
        w = (len(r[6]) + 63) // 64
        if cur and (waves + w) * 64 * max(cap, r[5]) * ops.SPLINE_WS_COLS * 8 > budget:
            chunks.append(cur)
            cur, waves, cap = [], 0, 6
        cur.append(r)
        waves, cap = waves + w, max(cap, r[5])
    if cur:
        chunks.append(cur)
    out = []
    for ch in chunks:
        grp = np.zeros((len(ch), ops.SPLINE_GRP), np.int32)
        s, c0 = [], 0
        for g, (j, axis, row0, m, k, ncap, sv) in enumerate(ch):
            grp[g] = (row0, m, k, ncap, c0, len(sv), 0, axis)
            s.append(sv)
            c0 += len(sv)
        waves = ops.spline_waves(grp)
        out.append(dict(grp=grp, waves=waves, s=np.concatenate(s) if s else np.zeros(0), ncap=int(max([6] + [r[5] for r in ch])),
                        groups=[(r[0], r[1]) for r in ch]))
    return dict(chunks=out, m50=m50, m10=m10)


def host_weights(state6, cam, P1, P2):
    """The arithmetic of ``rn_label_box_weights`` in numpy, one rounding per operation (fp32 corners, fp64 projection) -> fp64
    [n,2] = (x_weight, y_weight).  Only for the refusal of a weight that is not positive and finite BEFORE any device work: the
    fits take the kernel's weights."""
    f32 = np.float32
    s = state6.astype(f32)
    x, y, l, w, d = s[:, 0], s[:, 1], s[:, 2], s[:, 3], s[:, 5]
    xf = x + d * l
    half = d * w / f32(2.0)
    ylo, yhi = y - half, y + half
    P = P1[cam]
    if P2 is not None:
        P = np.where((ylo > f32(60.0))[:, None], P2[cam], P)
    im = []
    for cx, cy in ((xf, ylo), (xf, yhi), (x, ylo), (x, yhi)):
        X, Y = cx.astype(np.float64), cy.astype(np.float64)
        with np.errstate(all="ignore"):
            u = ((P[:, 0] * X + P[:, 1] * Y) + P[:, 2] * 0.0) + P[:, 3]
            v = ((P[:, 4] * X + P[:, 5] * Y) + P[:, 6] * 0.0) + P[:, 7]
            q = ((P[:, 8] * X + P[:, 9] * Y) + P[:, 10] * 0.0) + P[:, 11]
            im.append((u / q, v / q))
    with np.errstate(all="ignore"):
        yu = ((im[0][0] - im[1][0]) + (im[2][0] - im[3][0])) / 2.0
        yv = ((im[0][1] - im[1][1]) + (im[2][1] - im[3][1])) / 2.0
        xu = ((im[0][0] - im[2][0]) + (im[1][0] - im[3][0])) / 2.0
        xv = ((im[0][1] - im[2][1]) + (im[1][1] - im[3][1])) / 2.0
        return np.stack([np.sqrt(xu * xu + xv * xv) / state6[:, 2], np.sqrt(yu * yu + yv * yv) / state6[:, 3]], axis=1)


def _refuse_weights(pack, wts):
    bad = np.nonzero(~(np.isfinite(wts[:, :2]) & (wts[:, :2] > 0)).all(axis=1))[0]
    if len(bad):
        r = int(bad[0])
        j = int(np.searchsorted(pack["off"], r, side="right") - 1)
        a = 0 if not (np.isfinite(wts[r, 0]) and wts[r, 0] > 0) else 1
        raise ValueError("object {}, axis {}: a weight of {!r} pixels per foot is not positive and finite".format(
            pack["ids"][j], "xy"[a], float(wts[r, a])))


def _tables(self, pack):
    hg1, hg2 = _sides(self.hg)
    used = {pack["names"][c] for c in set(pack["cam"].tolist())}
    return _P_table(hg1, pack["names"], used), None if hg2 is None else _P_table(hg2, pack["names"], used)


def fit_objects(self, ids, y_order=2, x_order=3, weight=True, metric="ape", complexity=4, tpex=None, tpey=None, budget=None,
                keep=False):
    """Every object of ``ids`` through one batch of launches -> [None or dict(t, x: Spline, y: Spline, figs_x, figs_y)] per id
    (None where the reference returns Nones), and with ``keep`` the per-chunk device outputs on the host as well."""
    tpex = tpe_x() if tpex is None else np.asarray(tpex, np.float64)
    tpey = tpe_y() if tpey is None else np.asarray(tpey, np.float64)
    pack = pack_objects(self, list(ids))
    plan = plan_fits(pack, y_order, x_order, complexity, tpex, tpey, budget)
    results, kept = [None] * len(pack["ids"]), []
    if not plan["chunks"]:
        return (results, kept, pack) if keep else results
    P1, P2 = _tables(self, pack)
    fitted = np.zeros(len(pack["t"]), bool)
    for ch in plan["chunks"]:
        for j, _ in ch["groups"]:
            fitted[int(pack["off"][j]):int(pack["off"][j + 1])] = True
    rows = np.nonzero(fitted)[0]
    check = np.ones((len(pack["t"]), 2))
    check[rows] = host_weights(pack["state6"][rows], pack["cam"][rows], P1, P2)
    _refuse_weights(pack, check)
    dev = _device(self)                                         # every refusal above comes before any GPU work
    host = [pack["state6"], pack["cam"], pack["t"], plan["m50"], plan["m10"], P1] + ([] if P2 is None else [P2])
    for ch in plan["chunks"]:
        host += [ch["grp"], ch["waves"], ch["s"]]
    up = _upload(dev, host)
    state6, cam, t, m50, m10, dP1 = up[:6]
    dP2 = None if P2 is None else up[6]
    tables = up[6 + (P2 is not None):]
    wts, status = ops.label_box_weights(state6, cam, dP1, dP2)
    xw, yw = wts[:, 0].contiguous(), wts[:, 1].contiguous()
    base = xw if weight else torch.ones_like(xw)
    tx, val = torch.cat((t, t)), torch.cat((state6[:, 0], state6[:, 1])).contiguous()
    wt, wscore = torch.cat((xw, yw)), torch.cat(((base * m50) * m10, yw))
    outs, ws = [], None
    need = max(ops.SPLINE_WS_COLS * ch["ncap"] * len(ch["waves"]) * 64 for ch in plan["chunks"])
    ws = torch.empty(need, dtype=torch.float64, device=dev)    # one workspace, reused by every chunk
    for i, ch in enumerate(plan["chunks"]):
        grp, waves, s = tables[3 * i:3 * i + 3]
        w, n, ier, fp, iters, status = ops.spline_fit(grp, waves, tx, val, wt, s, ch["ncap"], workspace=ws, status=status)
        scores, win, fig, wt_out, wc_out, status = ops.spline_select(grp, tx, val, wt, wscore, len(ch["s"]), ch["ncap"], w, n, ier,
                                                                      fp, metric, status=status)
        outs += [win, fig, wt_out, wc_out] + ([scores, n, ier, fp, iters, w[:2 * ch["ncap"]].clone()] if keep else [])
    down = _download([status, wts] + outs)
    ops.label_check(int(down[0][0]))
    h_wts, per = down[1], 10 if keep else 4
    _refuse_weights(pack, h_wts)                                # the kernel's own weights: the same bits as the host's check
    found = {}
    for i, ch in enumerate(plan["chunks"]):
        win, fig, wt_out, wc_out = down[2 + per * i:6 + per * i]
        if keep:
            kept.append(dict(zip(("scores", "n", "ier", "fp", "iters", "tc"), down[6 + per * i:12 + per * i]), win=win, fig=fig,
                             t=wt_out, c=wc_out, **ch))
        for g, (j, axis) in enumerate(ch["groups"]):
            if win[g, 0] >= 0:
                n, k = int(win[g, 1]), int(ch["grp"][g, 2])
                found[(j, axis)] = (Spline(wt_out[g, :n], wc_out[g, :n - k - 1], k, int(win[g, 2]), float(fig[g, 0]),
                                           getattr(self, "device", None)), fig[g].copy())
    for j in range(len(pack["ids"])):
        if (j, 0) in found and (j, 1) in found:
            lo, hi = int(pack["off"][j]), int(pack["off"][j + 1])
            results[j] = dict(t=pack["t"][lo:hi].copy(), x=found[(j, 0)][0], y=found[(j, 1)][0], figs_x=found[(j, 0)][1],
                              figs_y=found[(j, 1)][1])
    return (results, kept, pack) if keep else results


def _report(idx, r):
    fx, fy = r["figs_x"], r["figs_y"]
    print("Object {}: Space error: {:.2f}ft x, {:.2f}ft y ------ Pixel Error: {:.2f}/{:.2f}px x, {:.2f}/{:.2f}px y".format(
        idx, fx[2], fy[2], fx[3], fx[4], fy[3], fy[4]))


# ------------------------------------------------------------------------------------------------ the methods
def create_trajectory(self, idx, y_order=2, x_order=3, plot=False, weight=True, metric="ape", verbose=True, complexity=4):
    """:1137-1314 -> [t, x_spline, y_spline, avg_x, avg_xp] or five Nones."""
    if plot:
        raise NotImplementedError("create_trajectory(plot=True) draws with matplotlib, which this port does not carry")
    r = fit_objects(self, [idx], y_order, x_order, weight, metric, complexity)[0]
    if r is None:
        return [None, None, None, None, None]
    if verbose:
        _report(idx, r)
    return [r["t"], r["x"], r["y"], r["figs_x"][2], r["figs_x"][3]]


def get_splines(self, plot=False, metric="mpe"):
    """:1338-1350: every object below ``get_unused_id()`` in one batch of launches; sets ``self.splines``."""
    if plot:
        raise NotImplementedError("get_splines(plot=True) draws with matplotlib, which this port does not carry")
    splines, apes, ases = [], [], []
    for idx, r in enumerate(fit_objects(self, range(get_unused_id(self)), metric=metric)):
        if r is None:
            splines.append([None, None])
            continue
        _report(idx, r)
        splines.append([r["x"], r["y"]])
        ases.append(r["figs_x"][2])
        apes.append(r["figs_x"][3])
    print("Spline errors: {}ft ase, {}px ape".format(sum(ases) / len(ases), sum(apes) / len(apes)))
    self.splines = splines


def _all_boxes(self, n_ids, n_frames=None):
    """(frame, key, datum, object id, camera index) of every box of an id below ``n_ids`` whose key is "{seq_key}_{id}"."""
    index = {}
    for c, name in enumerate(self.seq_keys):
        index.setdefault(name, c)
    out = []
    for f, frame in enumerate(self.data if n_frames is None else self.data[:n_frames]):
        for key, item in frame.items():
            head, sep, tail = key.rpartition("_") if isinstance(key, str) else ("", "", "")
            if sep and head in index and tail.isdigit() and str(int(tail)) == tail and int(tail) < n_ids:
                out.append((f, key, item, int(tail), index[head]))
    return out


def gen_trajectories(self):
    """:1317-1336: ``self.spline_data`` = a deep copy of ``data`` with x, y of every box moved onto its object's splines, one
    launch for all boxes; fits first (metric "ape", not kept) when ``self.splines`` is None."""
    n_ids = get_unused_id(self)
    if self.splines is None:
        splines = [[None, None] if r is None else [r["x"], r["y"]] for r in fit_objects(self, range(n_ids))]
    else:
        splines = self.splines
    spline_data = copy.deepcopy(self.data)
    me = type("_View", (), {})()
    me.data, me.seq_keys = spline_data, self.seq_keys
    boxes = [b for b in _all_boxes(me, n_ids) if splines[b[3]][0] is not None]
    if boxes:
        dev = _device(self)
        flat = [s for pair in splines[:n_ids] for s in (pair[0], pair[1] if pair[0] is not None else None)]
        st, sc, snk = pack_splines(flat)
        ts = np.array([float(b[2]["timestamp"]) for b in boxes], np.float64)
        obj = np.array([b[3] for b in boxes], np.int32)
        up = _upload(dev, [st, sc, snk, np.concatenate((2 * obj, 2 * obj + 1)).astype(np.int32), np.concatenate((ts, ts))])
        xy = _download([ops.spline_eval(*up)])[0].reshape(2, -1)
        for b, x, y in zip(boxes, xy[0].tolist(), xy[1].tolist()):
            b[2]["x"] = x
            b[2]["y"] = y
    self.spline_data = spline_data


def plan_ts_shift(self, n_ids):
    """The (frame, camera) entries of :1358-1414 in the reference's order -> ([(frame, camera index, camera, [ids present],
    [ids kept])], the number of frames the loop enters, the one it breaks in included)."""
    entries, entered = [], 0
    for f_idx, frame in enumerate(self.data):
        entered = f_idx + 1
        if f_idx > self.last_frame or len(frame) == 0:
            break
        for c_idx, cam in enumerate(self.seq_keys):
            ids = [i for i in range(n_ids) if frame.get("{}_{}".format(cam, i)) is not None]
            kept = [i for i in ids if self.splines[i][0] is not None]
            if kept:
                entries.append((f_idx, c_idx, cam, ids, kept))
    return entries, entered


def adjust_ts_with_trajectories(self, max_shift=0.01, trials=21, overwrite_ts_data=False, metric="ape", use_running_error=True,
                                verbose=True):
    """:1353-1458: per (frame, camera) the time shift in ``np.linspace(-max_shift, max_shift, trials)`` that brings the x
    splines closest to the labels; rewrites the boxes' timestamps (and ``all_ts`` with ``overwrite_ts_data``) -> per entry
    (frame, camera index, best time, best error, initial error, best trial or -1)."""
    if not 1 <= int(trials) < 64:
        raise ValueError("adjust_ts_with_trajectories: 1 <= trials < 64")
    shifts = np.linspace(-max_shift, max_shift, trials)
    entries, entered = plan_ts_shift(self, get_unused_id(self))
    running = [self.ts_bias[i] for i in range(len(self.seq_keys))]
    run, base, off, rs, rx = [], [], [0], [], []
    for f_idx, c_idx, cam, ids, kept in entries:
        run.append(float(running[c_idx]))
        base.append(float(self.all_ts[f_idx][cam]))
        for i in kept:
            rs.append(i)
            rx.append(float(self.data[f_idx]["{}_{}".format(cam, i)]["x"]))
        off.append(len(rs))
        if use_running_error:
            running[c_idx] += shifts[-1]                        # :1457: ``shift`` is the last trial
    report, last = [], -1

    def frames_to(f_end):
        for f in range(last + 1, f_end):
            if verbose and f % 100 == 0:
                print("Adjusting ts for frame {}".format(f))
    if entries:
        dev = _device(self)
        st, sc, snk = pack_splines([pair[0] for pair in self.splines])
        up = _upload(dev, [st, sc, snk, np.array(off, np.int64), np.array(rs, np.int32), np.array(rx, np.float64),
                           np.array(base, np.float64), np.array(run, np.float64), shifts.astype(np.float64)])
        best_t, errs, best_i, status = ops.label_ts_shift(*up, use_run=use_running_error, metric=metric)
        h_status, h_t, h_e, h_i = _download([status, best_t, errs, best_i])
        ops.label_check(int(h_status[0]))
        for (f_idx, c_idx, cam, ids, kept), bt, (be, ie), bi, r in zip(entries, h_t.tolist(), h_e.tolist(), h_i.tolist(), run):
            frames_to(f_idx + 1)
            last = max(last, f_idx)
            if verbose:
                with np.errstate(all="ignore"):
                    print("{} frame {}: shifted time by {:.3f}s --- {:.2f}x initial error".format(
                        cam, f_idx, shifts[-1] + r, np.float64(be) / np.float64(ie)))
            for i in ids:
                self.data[f_idx]["{}_{}".format(cam, i)]["timestamp"] = bt
            if overwrite_ts_data:
                self.all_ts[f_idx][cam] = bt
            report.append((f_idx, c_idx, bt, be, ie, bi))
    frames_to(entered)
    return report


def adjust_boxes_with_trajectories(self, max_shift_x=2, max_shift_y=2, verbose=False):
    """manual_annotator_state_v3.py:1440-1515: every box of frames <= ``last_frame`` moves towards its object's splines, by at
    most ``max_shift_x`` pixels along x and ``max_shift_y`` along y (in feet: l / x_diff and w / y_diff per pixel, the box's
    own projection) -> ``pixel_shifts``, sqrt(dx^2 + dy^2) of every box that has a y spline, in the reference's order (frame,
    then the frame's dict order).  One upload, two launches (the weights' diffs, every spline value), one copy back."""
    try:
        splines = self.splines
    except AttributeError:
        print("Splines not yet fit - cannot adjust boxes using splines")
        return
    names = _seq_names(self)
    index = {}
    for c, name in enumerate(names):
        index.setdefault(name, c)
    boxes = []
    for f_idx, frame in enumerate(self.data):
        if f_idx > self.last_frame:
            break
        for item in frame.values():
            if item["camera"] not in index:
                raise ValueError("frame {}: camera {!r} is not one of the cameras".format(f_idx, item["camera"]))
            splines[item["id"]]                                 # the reference's IndexError / TypeError, before any device work
            boxes.append((f_idx, item))
    pixel_shifts = []
    if boxes:
        state = np.array([[float(b[k]) for k in STATE_KEYS] for _, b in boxes], np.float64).reshape(-1, 6)
        cam = np.array([index[b["camera"]] for _, b in boxes], np.int32)
        ts = np.array([float(b["timestamp"]) for _, b in boxes], np.float64)
        ids = sorted({b["id"] for _, b in boxes})
        slot = {oid: j for j, oid in enumerate(ids)}
        flat = [s for oid in ids for s in splines[oid]]
        st, sc, snk = pack_splines(flat)
        obj = np.array([slot[b["id"]] for _, b in boxes], np.int32)
        pack = dict(names=names, cam=cam)
        P1, P2 = _tables(self, pack)
        dev = _device(self)
        up = _upload(dev, [state, cam, P1] + ([] if P2 is None else [P2]) + [st, sc, snk, np.concatenate((2 * obj, 2 * obj + 1)).astype(np.int32),
                                                                            np.concatenate((ts, ts))])
        n_p = 3 + (P2 is not None)
        wts, status = ops.label_box_weights(up[0], up[1], up[2], up[3] if P2 is not None else None)
        val = ops.spline_eval(*up[n_p:])
        h_status, h_wts, h_val = _download([status, wts, val])
        ops.label_check(int(h_status[0]))
        h_val = h_val.reshape(2, -1)
        x_lim = state[:, 2] / h_wts[:, 2] * max_shift_x       # :1472
        y_lim = state[:, 3] / h_wts[:, 3] * max_shift_y       # :1468
        last = -1
        for i, (f_idx, box) in enumerate(boxes):
            xs, ys = splines[box["id"]]
            if xs is not None:
                x_diff = h_val[0, i] - state[i, 0]
                if x_diff < -x_lim[i]:
                    x_diff = -x_lim[i]
                elif x_diff > x_lim[i]:
                    x_diff = x_lim[i]
                box["x"] += x_diff
            if ys is not None:
                y_diff = h_val[1, i] - state[i, 1]
                if y_diff < -y_lim[i]:
                    y_diff = -y_lim[i]
                elif y_diff > y_lim[i]:
                    y_diff = y_lim[i]
                box["y"] += y_diff
                pixel_shifts.append(np.sqrt(x_diff ** 2 + y_diff ** 2))     # NameError without an x spline, as the reference
            if verbose and f_idx != last and f_idx % 100 == 0:
                print("Adusted boxes for frame {}".format(f_idx))
            last = f_idx
    return pixel_shifts


class LabelTrajectory():
    """The functions above as methods: inherit it beside (or assign its members into) the reference's ``Annotator``."""
    get_unused_id = get_unused_id
    create_trajectory = create_trajectory
    get_splines = get_splines
    gen_trajectories = gen_trajectories
    adjust_ts_with_trajectories = adjust_ts_with_trajectories
    adjust_boxes_with_trajectories = adjust_boxes_with_trajectories

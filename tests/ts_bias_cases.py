"""Input recipes of the time-stamp-bias vectors (tests/golden/ts_bias.npz) and a numpy restatement of
MC_Crop_Tracker.estimate_ts_bias (MC3D_crop_tracker.py:237-315), the fuzz oracle of rn_estimate_ts_bias.

The inputs are scripted scenes and ``synth``'s portable generators, so tools/make_golden.py and the tests rebuild them
and the golden file holds outputs only.

  cases()        name -> dict(boxes [d,6] f32, cams [d] i64, objs [n,7] f32 (x y l w h dir v: what
                 Torch_KF.view(with_direction=True) returns), timestamps, ts_bias (lists of floats), phi)
  parse_scene()  tracker state (objs, timestamps, ts_bias) for parse_detections with est_ts on
                 golden_cases.tracker_post_inputs()
  sequence()     8 detection frames of two cameras that both see some vehicles
  restated()     steps 2-6 of the method in numpy, with the dtypes torch's promotion gives the reference
  fuzz_scene()   random scenes for the GPU fuzz test
"""
import numpy as np

import track_cases as tc
from retinanet_mi355x import synth

PHI = 0.2                    # phi_nms_space, MC3D_crop_tracker.py:68
ALPHA = 0.05                 # ts_alpha, :84
MU_V = 80.0                  # track_cases.kf_init()["mu_v"]
F32 = np.float32


# ---------------------------------------------------------------------------------------------- the restatement
def footprints(boxes):
    """[d,6] f32 states -> [d,4] f32 (xmin, ymin, xmax, ymax) of the four bottom corners of state_to_space
    (homography.py:305-320, MC3D_crop_tracker.py:268-275), every operation in fp32."""
    b = np.asarray(boxes, dtype=F32).reshape(-1, 6)
    x, y, l, w, dr = b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 5]
    xf = x + dr * l
    half = dr * w / F32(2.0)
    ylo, yhi = y - half, y + half
    return np.stack((np.minimum(xf, x), np.minimum(ylo, yhi), np.maximum(xf, x), np.maximum(ylo, yhi)), axis=1).astype(F32)


def iou_matrix(fp):
    """md_iou (MC3D_crop_tracker.py:1030-1049) of every pair, fp64, its operation order."""
    a = fp.astype(np.float64)
    A, B = a[:, None, :], a[None, :, :]
    area_a = (A[..., 2] - A[..., 0]) * (A[..., 3] - A[..., 1])
    area_b = (B[..., 2] - B[..., 0]) * (B[..., 3] - B[..., 1])
    minx, maxx = np.maximum(A[..., 0], B[..., 0]), np.minimum(A[..., 2], B[..., 2])
    miny, maxy = np.maximum(A[..., 1], B[..., 1]), np.minimum(A[..., 3], B[..., 3])
    inter = np.maximum(0.0, maxx - minx) * np.maximum(0.0, maxy - miny)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((area_a + area_b) - inter)


def velocities(objs, mu_v=MU_V):
    """(EB_vel, WB_vel) as fp32 (:258-265).  More than two objects of one direction: the summation order of
    torch.mean is not restated (numpy's is used)."""
    o = np.asarray(objs, dtype=F32).reshape(-1, 7)
    e, w = o[o[:, 5] == 1, 6], o[o[:, 5] == -1, 6]
    eb = F32(mu_v) if len(e) == 0 else F32(e.sum(dtype=F32) / F32(len(e)))
    wb = F32(-mu_v) if len(w) == 0 else F32(F32(w.sum(dtype=F32) / F32(len(w))) * F32(-1))
    return eb, wb


def pair_list(boxes, cams, phi):
    """-> [p,2] int64 (i, j): i ascending, j ascending from i+1, different cameras, iou > phi (:284-287)."""
    iou = iou_matrix(footprints(boxes))
    cams = np.asarray(cams)
    hit = np.triu(iou > phi, 1) & (cams[:, None] != cams[None, :])
    return np.argwhere(hit).astype(np.int64).reshape(-1, 2)


def restated(boxes, cams, objs, timestamps, ts_bias, phi=PHI, alpha=ALPHA, mu_v=MU_V, vel=None):
    """-> dict(entries [e,4] i64 (cam1, cam2, i, j), time_error [e] f32, ts_bias list of floats, vel (EB, WB)).
    ``vel`` overrides the two mean velocities (fp32)."""
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 6)
    cams = np.asarray(cams, dtype=np.int64)
    bias = [float(b) for b in ts_bias]
    none = dict(entries=np.zeros((0, 4), np.int64), time_error=np.zeros(0, F32), ts_bias=bias, vel=None)
    if len(cams) == 0 or len(objs) == 0:                                # the early returns (:251-257)
        return none
    eb, wb = velocities(objs, mu_v) if vel is None else (F32(vel[0]), F32(vel[1]))
    entries, te = [], []
    for i, j in pair_list(boxes, cams, phi):
        ci, cj = int(cams[i]), int(cams[j])
        v = wb if boxes[i, 5] == -1 else eb                             # the direction of detection i, both entries
        for c1, c2, dx in ((ci, cj, boxes[j, 0] - boxes[i, 0]), (cj, ci, boxes[i, 0] - boxes[j, 0])):
            dt_expected = F32(timestamps[c2] - timestamps[c1])          # Python doubles, then torch.tensor -> fp32
            with np.errstate(invalid="ignore", divide="ignore"):
                t = F32(F32(dx) / v) - dt_expected
            entries.append((c1, c2, int(i), int(j)))
            te.append(t)
    keep = 1.0 - alpha
    for (c1, c2, _, _), t in zip(entries, te):                          # strictly serial (:311-315)
        if c1 != 0:
            a = F32(keep * bias[c1])                                    # Python double, joins the fp32 tensor as fp32
            s = F32(-t) + F32(bias[c2])
            bias[c1] = float(a + F32(alpha) * s)
    return dict(entries=np.array(entries, np.int64).reshape(-1, 4), time_error=np.array(te, F32), ts_bias=bias, vel=(eb, wb))


def ulp_bound(boxes, cams, objs, timestamps, ts_bias, phi=PHI, alpha=ALPHA, mu_v=MU_V, vel=None, steps=1):
    """The allowed ts_bias difference where the mean's summation order is free: the largest change of the restatement's
    ts_bias when each mean velocity is moved ``steps`` fp32 ulps up or down, times 2 (two sums, each an ulp off)."""
    base = restated(boxes, cams, objs, timestamps, ts_bias, phi, alpha, mu_v, vel)
    if base["vel"] is None:
        return 0.0
    eb, wb = base["vel"]
    worst = 0.0
    for de in (-1, 0, 1):
        for dw in (-1, 0, 1):
            e, w = eb, wb
            for _ in range(steps):
                e = np.nextafter(e, F32(np.inf) * de) if de else e
                w = np.nextafter(w, F32(np.inf) * dw) if dw else w
            r = restated(boxes, cams, objs, timestamps, ts_bias, phi, alpha, mu_v, vel=(e, w))
            worst = max(worst, max(abs(a - b) for a, b in zip(r["ts_bias"], base["ts_bias"])))
    return 2.0 * worst


# ---------------------------------------------------------------------------------------------- scripted cases
def _vehicles(k, seed):
    """k vehicles that do not overlap each other: 90 ft apart, east-bound lanes below y = 60, west-bound above."""
    s = np.zeros((k, 6), F32)
    s[:, 5] = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    s[:, 0] = 150.0 + 90.0 * np.arange(k) + synth.uniform((k,), seed, 0, 20)
    s[:, 1] = np.where(s[:, 5] > 0, 12.0 + 12.0 * (np.arange(k) % 3), 72.0 + 12.0 * (np.arange(k) % 3))
    s[:, 2] = synth.uniform((k,), seed + 1, 14, 40)
    s[:, 3] = synth.uniform((k,), seed + 2, 5.5, 8)
    s[:, 4] = synth.uniform((k,), seed + 3, 4, 10)
    return s


def _second_view(s, seed, shift=1.5):
    """The same vehicles as another camera sees them a few milliseconds apart: shifted along x, a little in y and size."""
    k = len(s)
    t = s.copy()
    t[:, 0] += synth.uniform((k,), seed, -shift, shift)
    t[:, 1] += synth.uniform((k,), seed + 1, -0.3, 0.3)
    t[:, 2] += synth.uniform((k,), seed + 2, -0.5, 0.5)
    return t.astype(F32)


def _objs(rows):
    """rows of (x, y, l, w, h, dir, v) -> [n,7] f32."""
    return np.array(rows, F32).reshape(-1, 7)


_TRACKS_BOTH = _objs([(300, 12, 16, 6, 4.5, 1, 82.5), (500, 24, 18, 6.5, 5.5, 1, 77.25),
                      (700, 72, 19, 6.7, 6, -1, 84.0), (900, 84, 17, 6, 5, -1, 79.5)])


def _threshold_geometry(phi=PHI):
    """Two cross-camera pairs on either side of phi, as close as an fp32 x can place them: bisection on the x of the
    second view over the fp32 grid, against md_iou.  -> (boxes [4,6], cams [4])."""
    out = []
    for k, (x, y, l, w) in enumerate(((400.0, 24.0, 30.0, 6.5), (800.0, 84.0, 22.0, 7.25))):
        a = np.array([x, y, l, w, 5.0, 1.0 if k == 0 else -1.0], F32)

        def iou_at(xb):
            b = a.copy()
            b[0] = xb
            return iou_matrix(footprints(np.stack((a, b))))[0, 1]
        lo, hi = F32(x), F32(x + l)                                     # iou(lo) = 1 > phi, iou(hi) = 0
        for _ in range(200):
            mid = F32((np.float64(lo) + np.float64(hi)) / 2)
            if mid == lo or mid == hi:
                break
            if iou_at(mid) > phi:
                lo = mid
            else:
                hi = mid
        assert np.nextafter(lo, F32(np.inf)) == hi and iou_at(lo) > phi and not iou_at(hi) > phi
        b = a.copy()
        b[0] = lo if k == 0 else hi                                     # pair 0 just above phi, pair 1 just below
        out += [a, b]
    return np.stack(out).astype(F32), np.array([0, 1, 2, 1], np.int64)


def cases():
    """name -> inputs, in a fixed order."""
    out = {}
    # overlap3: 3 cameras, 8 vehicles of both directions; 7 seen twice, in every camera combination and order
    v = _vehicles(8, 400)
    w = _second_view(v, 410)
    first = [1, 0, 2, 1, 0, 2, 1, 0]                                      # camera of the first view
    second = [2, 1, 1, 0, 2, 0, 2, 0]                                     # vehicle 7: both views from camera 0 (no pair)
    boxes = np.concatenate((v, w))
    cams = np.array(first + second, np.int64)
    perm = np.argsort(synth.uniform((16,), 420), kind="stable")           # detector order is not grouped
    out["overlap3"] = dict(boxes=boxes[perm], cams=cams[perm], objs=_TRACKS_BOTH, timestamps=[1000.0, 1000.004, 999.997],
                           ts_bias=[0.0, 0.01, -0.02], phi=PHI)
    # cam0_only: two cameras, camera 0 on either side of the pair
    v = _vehicles(6, 430)
    w = _second_view(v, 440)
    boxes = np.concatenate((v, w))
    cams = np.array([0, 1, 0, 1, 0, 1] + [1, 0, 1, 0, 1, 0], np.int64)
    out["cam0_only"] = dict(boxes=boxes, cams=cams, objs=_TRACKS_BOTH, timestamps=[500.0, 500.0125], ts_bias=[0.0, -0.004],
                            phi=PHI)
    # one_direction: the filter holds east-bound tracks only; vehicles 1, 3 are west-bound
    v = _vehicles(4, 450)
    w = _second_view(v, 460)
    out["one_direction"] = dict(boxes=np.concatenate((v, w)), cams=np.array([1, 2, 0, 2, 2, 1, 1, 0], np.int64),
                                objs=_TRACKS_BOTH[:2], timestamps=[20.0, 20.01, 19.99], ts_bias=[0.0, 0.002, 0.003], phi=PHI)
    # same_camera: overlapping detections, all from camera 1
    v = _vehicles(5, 470)
    w = _second_view(v, 480)
    out["same_camera"] = dict(boxes=np.concatenate((v, w)), cams=np.ones(10, np.int64), objs=_TRACKS_BOTH,
                              timestamps=[7.0, 7.01], ts_bias=[0.0, 0.005], phi=PHI)
    base = out["cam0_only"]
    out["no_tracks"] = dict(base, objs=np.zeros((0, 7), F32))
    out["no_detections"] = dict(base, boxes=np.zeros((0, 6), F32), cams=np.zeros(0, np.int64))
    # threshold: see _threshold_geometry; then the same scene with phi 2 fp64 ulps below / at / 2 ulps above the first
    # pair's own IoU (one fp32 step of x moves the IoU by ~1e-6, so one phi cannot be within ulps of two different pairs)
    tb, tcams = _threshold_geometry()
    thr = dict(boxes=tb, cams=tcams, objs=_TRACKS_BOTH, timestamps=[100.0, 100.002, 100.001], ts_bias=[0.0, 0.001, -0.001])
    out["threshold"] = dict(thr, phi=PHI)
    iou0 = float(iou_matrix(footprints(tb))[0, 1])
    below = np.nextafter(np.nextafter(iou0, 0.0), 0.0)
    above = np.nextafter(np.nextafter(iou0, 1.0), 1.0)
    out["threshold_ulps_below"] = dict(thr, phi=float(below))             # the pair counts
    out["threshold_equal"] = dict(thr, phi=iou0)                          # strict >: it does not
    out["threshold_ulps_above"] = dict(thr, phi=float(above))
    return out


ORDER_FREE = ("overlap3", "cam0_only", "one_direction", "threshold", "threshold_ulps_below", "threshold_equal",
              "threshold_ulps_above")                      # <= 2 tracks per direction or the fallback: bit for bit


def parse_scene():
    """Tracker state for parse_detections(est_ts=True) on golden_cases.tracker_post_inputs(), whose fourth view of
    every vehicle comes from the neighbouring camera (the cross-camera duplicates).  -> (objs, timestamps, ts_bias)."""
    import golden_cases as gc
    n_cam = len(gc.tracker_post_inputs()[4])
    ts = [250.0 + 0.003 * ((7 * c) % 5) for c in range(n_cam)]
    bias = [0.0] + [0.001 * (c % 3) - 0.0015 for c in range(1, n_cam)]
    return _TRACKS_BOTH, ts, bias


def parse_bias_bound(states, r, n_cam, rtol=1e-5, atol=1e-4, bias_max=0.1):
    """Per-camera bound on |ts_bias - the reference's| when the states estimate_ts_bias looks at are the reference's
    only to atol + rtol |x| (the tolerance the parser's states are held to).  ``r`` = restated(...) on those states.
    A dx of entry (i, j) is then off by at most tol(x_i) + tol(x_j) and its time_error by that over |vel|, plus the
    fp32 roundings of the division, the subtraction and the three operations of the update, each at most one fp32
    spacing of a magnitude below |te| + bias_max.  One update is bias1 <- (1 - a) bias1 + a (bias2 - te), so the errors
    follow err1 <- (1 - a) err1 + a (err_te + err2) + roundings, evaluated along the entry list.  -> (bound [n_cam],
    per-entry time_error bound [e])."""
    x = np.abs(np.asarray(states, np.float64)[:, 0])
    tol = atol + rtol * x
    vmin = min(abs(float(v)) for v in r["vel"])
    err, te_err = np.zeros(n_cam), []
    assert max(abs(b) for b in r["ts_bias"]) <= bias_max
    for (c1, c2, i, j), t in zip(r["entries"], r["time_error"]):
        rnd = float(np.spacing(F32(abs(float(t)) + bias_max)))
        e_te = (tol[i] + tol[j]) / vmin + 2 * rnd
        te_err.append(e_te)
        if c1 != 0:
            err[c1] = (1 - ALPHA) * err[c1] + ALPHA * (e_te + err[c2]) + 3 * rnd
    return err, np.array(te_err)


# ---------------------------------------------------------------------------------------------- the sequence
SEQ_SHARED = {0: 1.1, 2: -0.9, 7: 0.8, 8: -1.2}    # vehicle of track_cases._VEHICLES -> x shift of its second view
SEQ_TS_BIAS = [0.0, 0.012]


def sequence():
    """track_cases.sequence() with a second view, from the other camera, of four of its vehicles in every frame in which
    they are detected (lower score: the space NMS drops it again, after estimate_ts_bias has looked at it)."""
    frames = []
    for f, fr in enumerate(tc.sequence()):
        det, lab, sc, cam = (fr[k] for k in ("detections", "labels", "scores", "cameras"))
        vis = [vi for vi, veh in enumerate(tc._VEHICLES) if f in veh[8]]
        rows, labels, scores, cams = list(det), list(lab), list(sc), list(cam)
        r = 0
        for vi in vis:
            if vi in SEQ_SHARED:
                b = det[r].copy()
                b[0] += F32(SEQ_SHARED[vi] + 0.1 * f)
                b[1] += F32(0.15)
                rows.append(b)
                labels.append(lab[r])
                scores.append(F32(sc[r] - 0.2))
                cams.append(1 - cam[r])
            r += 2 if (f == 0 and vi == tc._DUPLICATE) else 1
        frames.append(dict(timestamps=fr["timestamps"], detections=np.array(rows, F32), labels=np.array(labels, np.int64),
                           scores=np.array(scores, F32), cameras=np.array(cams, np.int64)))
    return frames


# ---------------------------------------------------------------------------------------------- fuzz
def fuzz_scene(t, seed=7000):
    """Random scene t: d in 2..300, 2..6 cameras, duplicates planted at random shifts, random starting biases, random
    filter contents including empty directions."""
    s = seed + 17 * t
    u = synth.uniform((8,), s)
    d = 2 + int(u[0] * 299) % 299
    n_cam = 2 + int(u[1] * 5) % 5
    k = max(1, int(d * (0.3 + 0.5 * u[2])))                              # vehicles; the rest are second / third views
    v = synth.vehicle_states(k, seed=s + 1).numpy()
    src = (synth.uniform((d - k,), s + 2) * k).astype(np.int64) % k if d > k else np.zeros(0, np.int64)
    w = v[src].copy()
    w[:, 0] += synth.uniform((len(src),), s + 3, -12, 12)
    w[:, 1] += synth.uniform((len(src),), s + 4, -2, 2)
    boxes = np.concatenate((v, w)).astype(F32)
    cams = (synth.uniform((d,), s + 5) * n_cam).astype(np.int64) % n_cam
    perm = np.argsort(synth.uniform((d,), s + 6), kind="stable")
    n = int(u[3] * 12) % 12                                              # 0 .. 11 tracks
    objs = np.zeros((n, 7), F32)
    if n:
        objs[:, :6] = synth.vehicle_states(n, seed=s + 7).numpy()
        objs[:, 6] = synth.uniform((n,), s + 8, 40, 110)
        mode = int(u[4] * 4) % 4                                         # 1: no west-bound track, 2: no east-bound one
        if mode == 1:
            objs[:, 5] = 1.0
        elif mode == 2:
            objs[:, 5] = -1.0
    ts = [1000.0 + float(x) for x in synth.uniform((n_cam,), s + 9, -0.02, 0.02)]
    bias = [float(F32(x)) for x in synth.uniform((n_cam,), s + 10, -0.05, 0.05)]
    bias[0] = 0.0
    return dict(boxes=boxes[perm], cams=cams[perm], objs=objs, timestamps=ts, ts_bias=bias, phi=PHI)

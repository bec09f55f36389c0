"""Inputs and a numpy restatement for the filter-fitting tests (fit_filter_3D.py; tests/golden/fit_filter.npz is made from
the same inputs by tools/make_golden.py with the reference's own Homography_Wrapper and Torch_KF).

Inputs: seeded synthetic tracklets (three frames of a vehicle with its own speed and acceleration, projected into its
camera, pixel jitter) and detector frames (one ground-truth vehicle, its jittered detection, bystanders) on the camera
matrices of golden_cases.homography_inputs().  Operator-level cases for the nearest-box search and the moments.

Restatement: ``nearest`` is the script's loop (:356-375) in fp32; ``moments`` accumulates in fp64 and rounds once, as the
kernel's contract says (the script sums serially in fp32: tests/test_fit_filter.py measures the distance between the
two); ``gt_states`` is the two-pass conversion through oracle/homography.py; ``q_errors`` one filter step in fp32.
"""
import numpy as np
import torch

import golden_cases as gc
import track_cases as tc
from oracle import homography as ohg
from retinanet_mi355x import synth

CLASS_NAMES = tc.CLASS_NAMES
N_TRACKLETS = 100                  # 25 iterations of the script's batch of 4
FRAME_D = [0, 1, 2, 64, 65, 130] + [3, 5, 0, 8, 4, 6, 1, 7] * 4 + [2, 9]   # detections per frame of the R fit: B = 40
F32 = np.float32


def kf_params():
    """INIT of the filter the Q fit steps (track_cases.kf_init: F = I, H = the first five states)."""
    return tc.kf_init()


def cameras():
    names, _, _, (Ps, Hs), (Ps2, Hs2) = gc.homography_inputs()
    return names, (Ps, Hs), (Ps2, Hs2)


def _near_camera(states, cam, seed, reach=60.0):
    """Put every vehicle within ``reach`` feet (along the road) of the camera that sees it: synth.camera_matrices places
    camera i at x = 200 + 700 u[i,3]; vehicles beyond y = 60 are seen through the second set of matrices."""
    s = np.array(states, dtype=F32)
    x1 = 200 + 700 * synth.uniform((18, 6), 5).astype(np.float64)[:, 3]
    x2 = 200 + 700 * synth.uniform((18, 6), 55).astype(np.float64)[:, 3]
    camx = np.where(s[:, 1] > 60, x2[cam], x1[cam])
    s[:, 0] = (camx + synth.uniform((len(s),), seed, -reach, reach)).astype(F32)
    return s


def _project(states, cam, jitter_px, seed, dtype):
    names, (Ps, Hs), (Ps2, Hs2) = cameras()
    im = ohg.wrapper_space_to_im(ohg.state_to_space(states), Ps[cam], Ps2[cam])                  # [n,8,2] f64
    im = im + (synth.uniform(im.shape, seed).astype(np.float64) - 0.5) * jitter_px
    return np.ascontiguousarray(im.astype(dtype))


def tracklets(n=N_TRACKLETS, seed=301):
    """-> (tracklets_im [n,3,8,2] fp32, classes [n] i64, cams [n] i64): frames 1/30 s apart, speed 60..120 ft/s, an
    acceleration of -25..15 ft/s^2 (its mean is not zero: mu_Q[5] is not), half a pixel of annotation jitter."""
    st = synth.vehicle_states(n, seed=seed).numpy()
    v = synth.uniform((n,), seed + 10, 60, 120).astype(np.float64)
    a = synth.uniform((n,), seed + 11, -25, 15).astype(np.float64)
    cam = (synth.uniform((n,), seed + 12) * 16).astype(np.int64) % 16       # cameras 16, 17 look along the road: ill-conditioned
    st = _near_camera(st, cam, seed + 14)
    frames = []
    for f in range(3):
        t = f / 30.0
        s = st.copy()
        s[:, 0] = (st[:, 0].astype(np.float64) + st[:, 5] * (v * t + 0.5 * a * t * t)).astype(F32)
        frames.append(_project(s, cam, 0.5, seed + 20 + f, F32))
    classes = (synth.uniform((n,), seed + 13) * 8).astype(np.int64) % 8
    return np.stack(frames, axis=1), classes, cam


def detector_frames(seed=401):
    """-> (gt_im [B,1,8,2] fp64, gt_classes [B], cams [B], scores [D], labels [D], boxes20 [D,20] fp32, offsets [B+1]).
    Frame b holds FRAME_D[b] detections; when it has any, one of them (at a seeded position) is the ground truth seen
    with 3 px of jitter, the others are vehicles elsewhere on the road."""
    B = len(FRAME_D)
    gt = synth.vehicle_states(B, seed=seed).numpy()
    cam = (synth.uniform((B,), seed + 1) * 18).astype(np.int64) % 18
    gt = _near_camera(gt, cam, seed + 9)
    gt_im = _project(gt, cam, 0.5, seed + 2, np.float64)[:, None]
    offsets = np.concatenate(([0], np.cumsum(FRAME_D))).astype(np.int64)
    D = int(offsets[-1])
    others = synth.vehicle_states(D, seed=seed + 3).numpy()
    det_cam = np.repeat(cam, FRAME_D)
    others = _near_camera(others, det_cam, seed + 10, reach=120.0)
    where = (synth.uniform((B,), seed + 4) * np.maximum(FRAME_D, 1)).astype(np.int64)
    for b in range(B):
        if FRAME_D[b]:
            others[offsets[b] + min(where[b], FRAME_D[b] - 1)] = gt[b]
    det = _project(others, det_cam, 3.0, seed + 5, F32).reshape(D, 16)
    xs, ys = det[:, 0::2], det[:, 1::2]
    boxes20 = np.concatenate((det, np.stack((xs.min(1), ys.min(1), xs.max(1), ys.max(1)), 1)), 1).astype(F32)
    scores = synth.uniform((D,), seed + 6, 0.3, 1.0)
    labels = (synth.uniform((D,), seed + 7) * 8).astype(np.int64) % 8
    gt_classes = (synth.uniform((B,), seed + 8) * 8).astype(np.int64) % 8
    return gt_im, gt_classes, cam, scores, labels, boxes20, offsets


def nearest_cases():
    """Operator-level inputs of the nearest-box search, in state space: name -> (gt [B,6], det [D,6], offsets [B+1])."""
    out = {}
    d_per = [0, 1, 2, 64, 65, 130]
    gt = synth.vehicle_states(len(d_per), seed=501).numpy()
    off = np.concatenate(([0], np.cumsum(d_per))).astype(np.int64)
    det = synth.vehicle_states(int(off[-1]), seed=502).numpy()
    for b, d in enumerate(d_per):                                  # every candidate overlaps the ground truth a little or a lot
        if d:
            sl = slice(off[b], off[b + 1])
            det[sl] = gt[b]
            det[sl, 0] += synth.uniform((d,), 503 + b, -20, 20)
            det[sl, 1] += synth.uniform((d,), 513 + b, -3, 3)
    out["sizes"] = (gt, det, off)
    # the best box twice: at the lowest and at the highest index of a frame that crosses the wave (the lowest must win),
    # and twice inside one lane's stride (rows 3 and 67)
    g = synth.vehicle_states(3, seed=521).numpy()
    off = np.array([0, 70, 140, 270], dtype=np.int64)
    det = synth.vehicle_states(270, seed=522).numpy()
    for b in range(3):
        sl = slice(off[b], off[b + 1])
        det[sl] = g[b]
        det[sl, 0] += synth.uniform((off[b + 1] - off[b],), 523 + b, 2, 25)
    best = g.copy()
    best[:, 0] += F32(0.5)
    det[0], det[69] = best[0], best[0]
    det[70 + 3], det[70 + 67] = best[1], best[1]
    det[140 + 129], det[140 + 1] = best[2], best[2]
    out["ties"] = (g, det, off)
    # zero-area boxes: 0/0 = NaN distances.  frame 0: a NaN candidate first, then a real one; frame 1: NaN only;
    # frame 2: NaN candidates around the winner; frame 3: empty
    g = synth.vehicle_states(4, seed=531).numpy()
    g[:, 3] = 0                                                    # zero width: zero area
    flat = g.copy()
    real = synth.vehicle_states(4, seed=532).numpy()
    real[:, :2] = g[:, :2]
    det = np.stack((flat[0], real[0], flat[1], flat[2], real[2], flat[2]))
    out["nan"] = (g, det.astype(F32), np.array([0, 2, 3, 6, 6], dtype=np.int64))
    return out


def moments_cases():
    """name -> (E [N,k] fp32, group or None, G): every N and k of the kernel's paths, a large common offset, groups with
    an empty and a one-row group."""
    out = {}
    for N in (1, 2, 3, 63, 64, 65, 257):
        for k in (1, 3, 5, 6):
            out["n%d_k%d" % (N, k)] = (synth.normal((N, k), 600 + N * 7 + k), None, 1)
    out["offset"] = ((synth.normal((257, 5), 641) + F32(1e4)).astype(F32), None, 1)
    grp = (synth.uniform((300,), 651) * 5).astype(np.int32) % 5
    grp[grp == 2] = 4                                              # group 2 empty
    grp[grp == 3] = 0
    grp[17] = 3                                                    # group 3: one row
    out["groups"] = ((synth.normal((300, 3), 652) * F32(3) + F32(20)).astype(F32), grp, 6)     # group 5 empty as well
    return out


# ------------------------------------------------------------------------------------------------ restatement
def footprints(states):
    sp = ohg.state_to_space(states)
    return np.stack((sp[:, 0:4, 0].min(1), sp[:, 0:4, 1].min(1), sp[:, 0:4, 0].max(1), sp[:, 0:4, 1].max(1)), 1).astype(F32)


def iou32(a, b):
    """fit_filter_3D.py:30-61 on two fp32 boxes, every operation rounded to fp32."""
    with np.errstate(invalid="ignore", divide="ignore"):
        area_a = F32(F32(a[2] - a[0]) * F32(a[3] - a[1]))
        area_b = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
        minx, maxx = (b[0] if b[0] > a[0] else a[0]), (b[2] if b[2] < a[2] else a[2])
        miny, maxy = (b[1] if b[1] > a[1] else a[1]), (b[3] if b[3] < a[3] else a[3])
        dx, dy = F32(maxx - minx), F32(maxy - miny)
        inter = F32((dx if dx > 0 else F32(0)) * (dy if dy > 0 else F32(0)))
        union = F32(F32(area_a + area_b) - inter)
        return F32(inter / union)


def nearest(gt, det, offsets, pick=None):
    """-> (rows i32 [B], resid f32 [matched,5], (matched, empty, unmatchable)).  ``pick(dists)`` replaces the script's
    loop (the tests hand in a naive argmin to show what the tie and NaN cases catch)."""
    gt, det = np.asarray(gt, F32), np.asarray(det, F32)
    fg, fd = footprints(gt), (footprints(det) if len(det) else np.zeros((0, 4), F32))
    rows, resid, empty, bad = [], [], 0, 0
    for b in range(len(gt)):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi <= lo:
            rows.append(-1)
            empty += 1
            continue
        dists = np.array([F32(1.0) - iou32(fd[j], fg[b]) for j in range(lo, hi)], F32)
        if pick is not None:
            r = pick(dists)
        else:
            r, m = -1, np.inf
            for j, dist in enumerate(dists):
                if dist < m:
                    m, r = dist, j
        if r < 0:
            rows.append(-1)
            bad += 1
            continue
        rows.append(lo + r)
        resid.append(det[lo + r, :5] - gt[b, :5])
    resid = np.stack(resid).astype(F32) if resid else np.zeros((0, 5), F32)
    return np.array(rows, np.int32), resid, (len(resid), empty, bad)


def moments(E, group=None, G=1):
    """fp64 sums rounded once; centred on the fp32 mean with fp32 differences.  -> (mean [G,k], cov [G,k,k], count [G]);
    without group the leading axis is dropped."""
    E = np.asarray(E, F32)
    k = E.shape[1]
    mean, cov, count = np.zeros((G, k), F32), np.zeros((G, k, k), F32), np.zeros(G, np.int32)
    for g in range(G):
        rows = E if group is None else E[np.asarray(group) == g]
        n = len(rows)
        count[g] = n
        if n == 0:
            continue
        mean[g] = (rows.astype(np.float64).sum(0) / n).astype(F32)
        d = (rows - mean[g]).astype(F32).astype(np.float64)
        cov[g] = ((d[:, :, None] * d[:, None, :]).sum(0) / n).astype(F32)
    return (mean[0], cov[0], count) if group is None else (mean, cov, count)


def heights(classes):
    return ohg.guess_heights([c if isinstance(c, str) else CLASS_NAMES[int(c)] for c in classes])


def gt_states(im, classes, cam):
    """fit_filter_3D.py:262-266 through oracle/homography.py."""
    names, (Ps, Hs), (Ps2, Hs2) = cameras()
    h0 = heights(classes)
    cam = np.asarray(cam)
    temp = ohg.space_to_state(ohg.wrapper_im_to_space(im, Hs[cam], Hs2[cam], h0))
    repro = ohg.wrapper_space_to_im(ohg.state_to_space(temp), Ps[cam], Ps2[cam])
    refined = ohg.height_from_template(repro, h0, im)
    return ohg.space_to_state(ohg.wrapper_im_to_space(im, Hs[cam], Hs2[cam], refined))


def q_errors(states, params=None, dt=1 / 30.0):
    """states [n,3,6] -> (error, prediction, target) [n,6] fp32: speeds by finite differences x 30, one step of the
    filter's X = F_rep X with F_rep[0,5] = D * dt (kf.py:309-311) as a running fp32 dot product, against frame 1."""
    s = np.asarray(states, F32)
    F = (params or kf_params())["F"].numpy().astype(F32)
    n = len(s)
    vel = ((s[:, 1, 0] - s[:, 0, 0]) * F32(30)).astype(F32)
    x = np.concatenate((s[:, 0, :5], vel[:, None]), 1).astype(F32)
    Fr = np.repeat(F[None], n, 0)
    Fr[:, 0, 5] = s[:, 0, 5] * F32(dt)
    pred = np.zeros((n, 6), F32)
    for a in range(6):
        acc = np.zeros(n, F32)
        for b in range(6):
            acc = (acc + (Fr[:, a, b] * x[:, b]).astype(F32)).astype(F32)
        pred[:, a] = acc
    vel2 = ((s[:, 2, 0] - s[:, 1, 0]) * F32(30)).astype(F32)
    target = np.concatenate((s[:, 1, :5], vel2[:, None]), 1).astype(F32)
    return (pred - target).astype(F32), pred, target


def speeds(first, last, n_frames):
    return (np.abs(last[:, 0] - first[:, 0]).astype(F32) / F32((n_frames - 1) / 30.0)).astype(F32)


def filter_probe():
    """A few detections for one add / predict / update of a filter built from the fitted parameters."""
    st = synth.vehicle_states(12, seed=701).numpy()
    classes = [CLASS_NAMES[i % 8] for i in range(12)]
    z = (st[:, :5] + (synth.uniform((12, 5), 702) - F32(0.5)) * F32(2)).astype(F32)
    return st, classes, z


# The script sums its moments serially in fp32, the kernel (and ``moments`` above) in fp64 with one rounding.  The largest
# distance between the two over the golden's cases (mu_Q/Q of 100 rows, mu_R/R of 35, mu_v/var of 100, the eight class
# groups of 21..51 rows), as |difference| / largest magnitude of the array, measured on the CPU by
# tests/test_fit_filter.py::test_moments_of_the_golden: 2.5e-7 (Q; class covariances 1.9e-7, the others below).  Serial
# summation error grows with the row count and these sizes are fixed, so the tests hold every moment to 4x that.
MOMENT_DEV = 2.5e-7
MOMENT_BOUND = 4 * MOMENT_DEV


def moment_dev(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())

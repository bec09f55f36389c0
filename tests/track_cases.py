"""Input recipes of the track-association vectors (tests/golden/tracker_assoc.npz): built from ``synth``'s portable
generators, so tools/make_golden.py and the tests rebuild the same inputs from seeds and the golden file holds outputs.

  lsap_cases()        named cost matrices for linear_sum_assignment (ties, IoU-like, uniform, 1xk, kx1, +inf entries,
                      two large ones)
  hungarian_cases()   (priors [n,7] with direction at column 5 as Torch_KF.view(with_direction=True) gives them,
                      detections [m,6] as parse_detections gives them) for match_hungarian
  sequence()          a scripted run of 8 detection frames through the tracker's association and pruning
"""
import numpy as np
import torch

from retinanet_mi355x import synth

PHI_MATCH = 0.1


def _ties(n, m, seed):
    return synth.randint((n, m), seed, 3).astype(np.float64)


def _iou_like(n, m, seed):
    u = synth.uniform((n, m), seed).astype(np.float64)
    return np.where(synth.uniform((n, m), seed + 1) < 0.8, 1.0, u)


def _uniform(n, m, seed):
    return synth.uniform((n, m), seed).astype(np.float64)


def lsap_cases():
    """-> list of (name, cost [n,m] fp64)."""
    cases = [("ties_5x5", _ties(5, 5, 101)), ("ties_4x7", _ties(4, 7, 102)), ("ties_8x3", _ties(8, 3, 103)),
             ("ties_9x9", _ties(9, 9, 104)), ("iou_6x6", _iou_like(6, 6, 105)), ("iou_7x10", _iou_like(7, 10, 106)),
             ("iou_11x4", _iou_like(11, 4, 107)), ("iou_30x40", _iou_like(30, 40, 108)),
             ("uni_5x5", _uniform(5, 5, 109)), ("uni_3x8", _uniform(3, 8, 110)), ("uni_9x2", _uniform(9, 2, 111)),
             ("row_1x6", _uniform(1, 6, 112)), ("col_6x1", _uniform(6, 1, 113)), ("one_1x1", _uniform(1, 1, 114)),
             ("ties_1x5", _ties(1, 5, 115)), ("ties_5x1", _ties(5, 1, 116))]
    a = _uniform(8, 10, 117)
    a[synth.uniform((8, 10), 118) < 0.3] = np.inf                            # +inf entries, still feasible
    cases.append(("inf_8x10", a))
    b = _iou_like(10, 6, 119)
    b[synth.uniform((10, 6), 120) < 0.25] = np.inf
    cases.append(("inf_10x6", b))
    cases.append(("iou_300x400", _iou_like(300, 400, 121)))
    cases.append(("uni_1000x700", _uniform(1000, 700, 122)))
    return cases


def _states(n, seed, ncol):
    s = synth.vehicle_states(n, seed=seed).numpy()
    if ncol == 7:                                                        # x y l w h dir v
        v = synth.uniform((n,), seed + 20, 60, 100)[:, None]
        s = np.concatenate([s, v], axis=1).astype(np.float32)
    return s


def hungarian_cases():
    """-> list of (name, priors [n,7] f32, detections [m,6] f32)."""
    out = []
    pre = _states(12, 201, 7)
    det = np.concatenate([pre[[3, 0, 7, 9, 1, 11, 5], :6], _states(4, 202, 6)]).astype(np.float32)
    det[:7, 0] += synth.uniform((7,), 203, -2.0, 2.0)                  # the same vehicles a little further on
    det[:7, 1] += synth.uniform((7,), 204, -0.5, 0.5)
    out.append(("normal", pre, det))
    pre_g = pre[:4].copy()
    det_g = pre_g[:, :6].copy()
    det_g[2, 0] += det_g[2, 5] * det_g[2, 2] * 0.95                     # overlaps its prior by ~5 %: gated
    det_g[0, 0] += 1.0
    out.append(("gated", pre_g, det_g))
    pre_z = pre[:3].copy()
    pre_z[1, 2] = 0.0                                                    # zero-length prior
    det_z = det[:4].copy()
    det_z[2, 3] = 0.0                                                    # zero-width detection: 0/0 against the prior
    pre_z[1, :6] = det_z[2, :6]
    pre_z[1, 2] = 0.0
    out.append(("zero_area", pre_z, det_z))
    out.append(("empty", pre[:0], det))
    return out


# ---------------------------------------------------------------------------------------------- the 8-frame script
CLASS_NAMES = ["sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer"]
CLASS_SIZE = {"sedan": (16.0, 6.0, 4.5), "midsize": (18.0, 6.5, 5.5), "van": (19.0, 6.5, 7.0),
              "pickup": (19.0, 6.8, 6.0), "semi": (70.0, 8.5, 13.0), "truck (other)": (35.0, 8.0, 10.0),
              "motorcycle": (7.0, 3.0, 4.5), "trailer": (30.0, 8.0, 10.0)}

PARAMS = dict(phi_match=PHI_MATCH, phi_over=0.1, f_max=3, max_size=torch.tensor([100, 15, 15]), x_range=[0, 1500])
TS_BIAS = [0.0, 0.012]
FRAME_DT = 0.1


def kf_init():
    """INIT of the tracker's filter (6 states x y l w h v, 5 measurements) with the entries add() reads."""
    H = torch.zeros(5, 6)
    H[:5, :5] = torch.eye(5)
    cs = {k: torch.tensor(v, dtype=torch.float32) for k, v in CLASS_SIZE.items()}
    cc = {k: torch.diag(torch.tensor([60.0, 2.0, 3.0])) for k in CLASS_SIZE}
    return {"P": torch.diag(torch.tensor([4.0, 2.0, 40.0, 2.0, 3.0, 200.0])), "F": torch.eye(6), "H": H,
            "Q": torch.diag(torch.tensor([1.0, 0.2, 0.5, 0.05, 0.05, 20.0])), "R": torch.diag(torch.tensor([1.0, 0.5, 2.0, 0.3, 0.3])),
            "mu_Q": torch.zeros(6), "mu_R": torch.zeros(5), "mu_v": torch.tensor(80.0), "class_size": cs,
            "class_covariance": cc}


# vehicle: (label, dir, x at t=0, y, l, w, h, speed, frames in which it is detected, camera, duplicated in frame 0)
_VEHICLES = [
    (0, 1, 200.0, 12.0, 16.5, 6.1, 4.6, 82.0, range(0, 8), 0),          # A: tracked throughout
    (1, 1, 420.0, 24.0, 18.2, 6.4, 5.4, 76.0, range(0, 3), 1),          # B: lost after frame 2, removed by fsld
    (3, -1, 900.0, 80.0, 19.3, 6.7, 6.1, 85.0, [0, 1, 2, 4, 5, 6, 7], 0),  # C: missed once (frame 3), re-matched
    (2, 1, 600.0, 36.0, 18.8, 6.6, 7.2, 79.0, range(2, 8), 1),          # D: enters at frame 2
    (0, -1, 1200.0, 100.0, 16.2, 5.9, 4.4, 81.0, range(5, 8), 1),       # E: enters at frame 5
    (5, 1, 1440.0, 48.0, 34.0, 8.1, 10.2, 95.0, range(0, 8), 0),        # F: drives past x_range (1500) -> anomaly
    (4, -1, 300.0, 92.0, 120.0, 8.4, 12.8, 75.0, range(1, 8), 1),       # G: 120 ft long, class size 70 -> oversized
    (1, 1, 800.0, 12.0, 18.0, 6.4, 5.6, 78.0, range(0, 8), 1),          # H, I, J: tracked throughout
    (2, -1, 700.0, 68.0, 19.0, 6.6, 7.0, 83.0, range(0, 8), 0),
    (0, 1, 1000.0, 24.0, 16.0, 6.0, 4.5, 80.0, range(0, 8), 0),
]
_DUPLICATE = 0                    # vehicle A is detected twice in frame 0 (2 ft apart): remove_overlaps prunes one


def frame_timestamps(f):
    """Per-camera time stamps of detection frame f (the cameras are a few ms apart)."""
    return [1000.0 + f * FRAME_DT, 1000.0 + f * FRAME_DT + 0.004]


def sequence():
    """The scene keeps the filter away from exactly 6 rows whenever a per-object dt is predicted: there the reference's
    ``Torch_KF.predict`` scales Q by broadcasting the [6] dt against Q's last axis instead of per object
    (util_track/kf.py:321-325; any other count raises and takes its per-object branch), which the drop-in filter does
    not reproduce.  -> list of 8 frames; each a dict: timestamps (list of 2 floats), detections [k,6] f32, labels [k] i64,
    scores [k] f32, cameras [k] i64."""
    frames = []
    for f in range(8):
        ts = frame_timestamps(f)
        rows, labels, scores, cams = [], [], [], []
        for vi, (lab, d, x0, y, l, w, h, v, seen, cam) in enumerate(_VEHICLES):
            if f not in seen:
                continue
            t = ts[cam] + TS_BIAS[cam] - 1000.0
            jx = float(synth.uniform((1,), 300 + 10 * f + vi, -0.3, 0.3)[0])
            x = x0 + d * v * t + jx
            rows.append([x, y, l, w, h, float(d)])
            labels.append(lab)
            scores.append(0.5 + 0.05 * vi)
            cams.append(cam)
            if f == 0 and vi == _DUPLICATE:
                rows.append([x + 2.0, y + 0.2, l, w, h, float(d)])
                labels.append(lab)
                scores.append(0.45)
                cams.append(1 - cam)
        frames.append(dict(timestamps=ts, detections=np.array(rows, dtype=np.float32),
                           labels=np.array(labels, dtype=np.int64), scores=np.array(scores, dtype=np.float32),
                           cameras=np.array(cams, dtype=np.int64)))
    return frames


def class_dict():
    d = {i: n for i, n in enumerate(CLASS_NAMES)}
    d.update({n: i for i, n in enumerate(CLASS_NAMES)})
    return d


# ---------------------------------------------------------------------------------------------- the fuzz oracle
def lsap_restated(C):
    """scipy's rectangular_lsap (Crouse 2016, shortest augmenting path) restated in Python, step for step: the
    ``remaining`` list with swap-with-last removal, the tie rule of the column choice, the dual updates.  The oracle of
    the kernel where scipy is absent.  -> (row_ind, col_ind) int64, or raises ValueError as scipy does."""
    import math
    C = np.asarray(C, dtype=np.float64)
    if C.ndim != 2:
        raise ValueError("expected a matrix (2-D array), got a %d array" % C.ndim)
    if C.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if np.isnan(C).any() or (C == -np.inf).any():
        raise ValueError("matrix contains invalid numeric entries")
    tr = C.shape[0] > C.shape[1]
    if tr:
        C = C.T
    nr, nc = C.shape
    u, v = np.zeros(nr), np.zeros(nc)
    path = np.full(nc, -1)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        spc = np.full(nc, math.inf)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        rem = [nc - it - 1 for it in range(nc)]
        nrem, minVal, i, sink = nc, 0.0, cur, -1
        while sink == -1:
            index, lowest = -1, math.inf
            SR[i] = True
            for it in range(nrem):
                j = rem[it]
                r = minVal + C[i, j] - u[i] - v[j]
                if r < spc[j]:
                    path[j], spc[j] = i, r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest, index = spc[j], it
            minVal = lowest
            if minVal == math.inf:
                raise ValueError("cost matrix is infeasible")
            j = rem[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            nrem -= 1
            rem[index] = rem[nrem]
        u[cur] += minVal
        for r in range(nr):
            if SR[r] and r != cur:
                u[r] += minVal - spc[col4row[r]]
        for c in range(nc):
            if SC[c]:
                v[c] -= minVal - spc[c]
        j = sink
        while True:
            r = path[j]
            row4col[j] = r
            col4row[r], j = j, col4row[r]
            if r == cur:
                break
    if tr:
        o = np.argsort(col4row, kind="stable")
        return col4row[o].astype(np.int64), o.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


def fuzz_matrices(count=2000, seed=900):
    """Small tie-heavy matrices (1x1 .. 8x8, wide and tall): integer costs 0/1/2, IoU-like, uniform."""
    out = []
    dims = synth.randint((count, 2), seed, 8) + 1
    for t in range(count):
        n, m = int(dims[t, 0]), int(dims[t, 1])
        kind = t % 3
        s = seed + 1 + 3 * t
        out.append(_ties(n, m, s) if kind == 0 else (_iou_like(n, m, s) if kind == 1 else _uniform(n, m, s)))
    return out

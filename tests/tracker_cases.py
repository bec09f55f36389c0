"""Scenes and plain CPU restatements for the whole tracker (3d-playground_amd/mc3d_tracker.py), shared by
tools/make_golden_tracker.py (which feeds the scene to the reference's own ``track()``), the host tests and the GPU tests.
Built only from the portable generators of ``retinanet_mi355x.synth``, so tests/golden/tracker_run.npz holds outputs.

  crop_prior_case / crop_prior_restated / first_min_nan_wins     inputs and restatements of ops.track_crop_prior
  Scene / ScriptedLoader / StandInDetector / StandInCropDetector  the 14-frame, 3-camera run
  HostTracker                                                    the frame loop restated on the CPU (oracle/ + numpy)
"""
import numpy as np
import torch

from retinanet_mi355x import synth

F32 = np.float32


# ---------------------------------------------------------------------------------------------- crop frame front end
def crop_prior_case(n, c, seed, t_offset=0.0):
    """Filter tensors for n tracks and c cameras.  Centres are integer-valued, 100 ft apart; both directions; rows 3 and 5
    (n >= 8, c >= 2) stand still exactly half way between cameras 0 / 1 and c-2 / c-1, so their two distances tie exactly;
    row 6 (n >= 8) has a NaN position.  T, the stamps and the biases sit on ``t_offset``."""
    X = np.zeros((n, 6), F32)
    X[:, 0] = synth.uniform((n,), seed, 0.0, 100.0 * c + 200.0)
    X[:, 1] = synth.uniform((n,), seed + 1, 0.0, 120.0)
    X[:, 2] = synth.uniform((n,), seed + 2, 12.0, 60.0)
    X[:, 3] = synth.uniform((n,), seed + 3, 5.0, 9.0)
    X[:, 4] = synth.uniform((n,), seed + 4, 4.0, 13.0)
    X[:, 5] = synth.uniform((n,), seed + 5, 60.0, 100.0)
    D = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(F32)
    centers = np.stack((150.0 + 100.0 * np.arange(c), np.full(c, 60.0)), axis=1).astype(F32)
    ties, nan_rows = [], []
    if n >= 8:
        if c >= 2:
            for r, k in ((3, 0), (5, c - 2)):
                X[r, 0], X[r, 5] = centers[k, 0] + F32(50.0), 0.0
                ties.append((r, k))
        X[6, 0] = np.nan
        nan_rows.append(6)
    T = t_offset + synth.uniform((n,), seed + 6, 0.0, 0.05).astype(np.float64)
    stamps = t_offset + 0.03 + 0.004 * (np.arange(c) % 5).astype(np.float64)
    bias = (synth.uniform((c,), seed + 7, -0.01, 0.01)).astype(np.float64)
    bias[0] = 0.0
    return dict(X=X, D=D, T=T, centers=centers, stamps=stamps, bias=bias, ties=ties, nan_rows=nan_rows)


def crop_prior_restated(pre_loc, centers, stamps, bias, T):
    """Nearest camera and per-track dt from the 1/30 s view, as the tracker's crop frame forms them on the host with
    torch: [n,c] matrices of centre minus position, squared, summed, abs, argmin; then one Python float per track
    (time stamp + bias of its camera) minus the filter's T.  pre_loc [n,>=2] fp32 CPU, centers [c,2] (any dtype: integer
    centres are promoted to fp32 by the subtraction), stamps / bias lists of floats, T [n] fp64.  -> (cam i64, dt f64)."""
    n, c = len(pre_loc), len(centers)
    obj_x = pre_loc[:, 0].unsqueeze(1).repeat(1, c)
    obj_y = pre_loc[:, 1].unsqueeze(1).repeat(1, c)
    cc_x = centers[:, 0].unsqueeze(0).repeat(n, 1)
    cc_y = centers[:, 1].unsqueeze(0).repeat(n, 1)
    diff = torch.abs(torch.pow(cc_x - obj_x, 2) + torch.pow(cc_y - obj_y, 2))
    cam = torch.argmin(diff, dim=1)
    times = torch.tensor([stamps[int(k)] + bias[int(k)] for k in cam], dtype=torch.float64)
    return cam, times - T


def first_min_nan_wins(dist):
    """The rule ``rn_track_crop_prior`` implements, spelled out: the first index attaining the minimum, a NaN counting as
    smaller than any number (so the first NaN wins).  dist: a sequence of floats."""
    best_k = 0
    for k in range(1, len(dist)):
        b, d = dist[best_k], dist[k]
        if b == b and (d != d or d < b):
            best_k = k
    return best_k


# ---------------------------------------------------------------------------------------------- the 14-frame scene
import golden_cases as gc                      # noqa: E402
import track_cases as tc                       # noqa: E402
import ts_bias_cases as tb                     # noqa: E402

# three cameras of the homography fixture, each watching a stretch of road on which its two transforms invert each other to
# a fraction of a foot (elsewhere these synthetic cameras put the horizon across the road): p3c1 300-650 ft, p3c2 300-750 ft,
# p1c3 550-1000 ft.  The scene stays between 300 and 1000 ft.
CAMERAS = ["p3c1", "p3c2", "p1c3"]
CAM_CENTERS = {"p3c1": (400, 60), "p3c2": (600, 60), "p1c3": (850, 60)}      # integer-valued, as a user would write them
CAM_EDGES = (500.0, 725.0)                     # half way between the centres: which camera sees a vehicle
TRUE_BIAS = [0.0, 0.012, -0.008]               # what the cameras' clocks are really off by
T0 = 1000.0
N_FRAMES = 15                                  # chunks per loader; camera 2 burns one catching up, so 14 frames are tracked
LAG_FRAME = 4                                  # camera 2 delivers this frame one period late: time_sync_cameras skips it
NONE_STAMP = (1, 7)                            # camera 1 cannot read the stamp of its frame 7
FRAME_HW = (64, 96)
N_CROP_DET = 8
PARAMS = dict(sigma_d=0.1, sigma_c=0.1, phi_nms_space=0.2, phi_nms_im=0.3, phi_match=0.1, phi_over=0.1, W=0.5, cd_max=4,
              f_max=3, f_init=5, cs=112, b=1.25, d=2, s=1, x_range=[0, 1000], max_size=torch.tensor([100, 15, 15]))
STATE_TOL = 1e-4                               # relative bound on X / P (tests/test_gpu_track_assoc.py:174-180)
MARGIN = 100 * STATE_TOL                       # every discrete decision keeps this distance from its runner-up

# vehicle: (label, dir, x at T0, y, l, w, h, speed, frames in which the detector sees it, second view from a neighbour camera)
VEHICLES = [
    (0, 1, 320.0, 12.0, 16.5, 6.1, 4.6, 82.0, range(0, 15), False),        # A: tracked throughout (+ a near-duplicate in frame 0)
    (1, 1, 420.0, 24.0, 18.2, 6.4, 5.4, 76.0, range(0, 3), False),         # B: lost after frame 2, removed by fsld
    (3, -1, 900.0, 80.0, 19.3, 6.7, 6.1, 85.0, [0, 2, 6, 8, 10, 12, 14], False),  # C: missed once (frame 4), re-matched
    (2, 1, 470.0, 36.0, 18.8, 6.6, 7.2, 79.0, range(4, 15), False),        # D: enters at frame 4, changes camera on the way
    (0, -1, 980.0, 100.0, 16.2, 5.9, 4.4, 81.0, range(8, 15), False),      # E: enters at frame 8
    (4, 1, 960.0, 48.0, 70.0, 8.4, 12.8, 90.0, range(0, 9), False),        # F: leaves x_range (1000) -> anomaly, see GLITCH
    (4, -1, 480.0, 92.0, 120.0, 8.4, 12.8, 75.0, range(2, 15), False),     # G: 120 ft long, max_size 100 -> oversized
    (1, 1, 640.0, 12.0, 18.0, 6.4, 5.6, 78.0, range(0, 15), True),         # H: also seen by the neighbouring camera
    (2, -1, 700.0, 68.0, 19.0, 6.6, 7.0, 83.0, range(0, 15), False),       # I
    (0, 1, 860.0, 24.0, 16.0, 6.0, 4.5, 80.0, range(0, 15), False),        # J
    (3, -1, 480.0, 104.0, 19.0, 6.8, 6.0, 84.0, range(0, 15), True),       # K: also seen by the neighbouring camera
    (1, 1, 350.0, 40.0, 18.0, 6.3, 5.5, 77.0, range(0, 15), False),        # L
]
# F cannot drive across x_range's end with MARGIN to spare on both sides (3 ft a frame against 10 ft): in frame 8 the detector
# reports it 45 ft further on (still matched: 70 ft long), and the update carries the track from below 990 to above 1010 ft
GLITCH = (5, 8, 45.0)
EARLY_CUTOFF = 5                               # the second run stops after this frame number
DUPLICATE = (0, 12.0)                          # frame 0: vehicle A again, 12 ft on: below phi_nms_space, above phi_over
CROP_JITTER = 0.1
CROP_SEED = 6000
CROP_LEVELS = (0.9, 0.62, 0.5, 0.4, 0.3, 0.25, 0.2, 0.15)


def camera_matrices():
    """(P1, H1, P2, H2) of the three cameras, from the homography fixture's two matrix sets."""
    names, _, _, (Ps, Hs), (Ps2, Hs2) = gc.homography_inputs()
    k = [names.index(c) for c in CAMERAS]
    return Ps[k], Hs[k], Ps2[k], Hs2[k]


def stamps():
    """Per camera, the time stamp of every chunk of its loader (None where it cannot be read)."""
    out = []
    for c in range(3):
        row = []
        for j in range(N_FRAMES):
            k = j - 1 if (c == 2 and j >= LAG_FRAME) else j            # camera 2 repeats a period from LAG_FRAME on
            row.append(T0 + k / 30.0 + 0.003 * c)
        out.append(row)
    out[NONE_STAMP[0]][NONE_STAMP[1]] = None
    return out


def ts_table():
    """params["ts"]: {sequence: [stamps]} as the reference's pickle holds them."""
    return {name + "_0_4k": row for name, row in zip(CAMERAS, stamps())}


def true_state(vi, t):
    lab, d, x0, y, l, w, h, v = VEHICLES[vi][:8]
    return [x0 + d * v * (t - T0), y, l, w, h, float(d)]


def camera_of(x):
    return 0 if x < CAM_EDGES[0] else (1 if x < CAM_EDGES[1] else 2)


class ScriptedLoader:
    """A frame source with the loader contract of mc3d_tracker: blank frames, scripted time stamps."""

    def __init__(self, cam, device="cpu"):
        self.sequence = "/data/%s_0.mp4" % CAMERAS[cam]
        self.stamps = stamps()[cam]
        self.frame = torch.zeros((3,) + FRAME_HW, dtype=torch.float32, device=device)
        self.i = 0

    def __len__(self):
        return len(self.stamps)

    def __next__(self):
        if self.i >= len(self.stamps):
            return (-1, None, None, None)
        self.i += 1
        return (self.i - 1, self.frame, None, self.stamps[self.i - 1])


class _StandIn:
    """Stand-in networks never look at pixels: they read the tracker they are attached to (``trk``: frame_num,
    timestamps, filter).  ``to`` / ``eval`` as a torch module has them."""

    def __init__(self):
        self.trk = None

    def to(self, device):
        return self

    def eval(self):
        return self


class StandInDetector(_StandIn):
    """detector(frames, MULTI_FRAME=True) -> (scores [d], labels [d], boxes [d,20], camera_idxs [d]): every vehicle the
    script shows in this frame, where it truly is at its camera's true time, projected into that camera; H and K once more
    from the neighbouring camera at a lower score; the duplicate of frame 0; two rows of clutter below sigma_d."""

    def __call__(self, frames, MULTI_FRAME=True):
        from oracle import homography as ohg
        trk = self.trk
        f = trk.frame_num
        P1, _, P2, _ = camera_matrices()
        rows = []                                                    # (state, camera, score, label)
        for vi, veh in enumerate(VEHICLES):
            if f not in veh[8]:
                continue
            cam = camera_of(true_state(vi, trk.timestamps[0])[0])
            views = [(cam, 0.5 + 0.03 * vi)]
            if veh[9]:
                views.append((cam + 1 if cam < 2 else 1, 0.3 + 0.03 * vi))
            for c, score in views:
                st = true_state(vi, trk.timestamps[c] + TRUE_BIAS[c])
                st[0] += float(synth.uniform((1,), 5000 + 40 * f + 3 * vi + c, -0.3, 0.3)[0])
                if (vi, f) == GLITCH[:2]:
                    st[0] += GLITCH[2]
                rows.append((st, c, score, veh[0]))
            if f == 0 and vi == DUPLICATE[0]:
                st = true_state(vi, trk.timestamps[1] + TRUE_BIAS[1])
                st[0] += DUPLICATE[1]
                rows.append((st, 1, 0.45, veh[0]))
        state = np.array([r[0] for r in rows], F32)
        cams = np.array([r[1] for r in rows], np.int64)
        im = ohg.wrapper_space_to_im(ohg.state_to_space(state), P1[cams], P2[cams]).reshape(len(rows), 16)
        im = np.concatenate((im, im[:2] + 35.0))                       # clutter
        cams = np.concatenate((cams, cams[:2]))
        scores = np.array([r[2] for r in rows] + [0.05, 0.07], F32)
        labels = np.array([r[3] for r in rows] + [0, 1], np.int64)
        xs, ys = im[:, 0:16:2], im[:, 1:16:2]
        boxes = np.concatenate((im, np.stack((xs.min(1), ys.min(1), xs.max(1), ys.max(1)), 1)), 1).astype(F32)
        dev = frames.device
        return (torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(boxes).to(dev),
                torch.from_numpy(cams).to(dev))


class StandInCropDetector(_StandIn):
    """cd(crops, LOCALIZE=True) -> (reg_boxes [n,8,20] crop pixels, cls [n,8,8]).  The priors are the tracker's filter as it
    stands after the crop frame's predict (``filter.view(with_direction=True)``); each is projected into its nearest
    camera, and golden_cases.crop_detections jitters 8 candidates around it (scaled by CROP_JITTER).  One class per candidate carries a score
    from CROP_LEVELS, rolled per row and frame.  Every fifth row's most confident candidate keeps the full jitter and its
    runner-up is raised to 0.8, so that the better placed one wins; a track whose vehicle the script no longer shows gets
    5 % of the scores (below sigma_c) and only its most confident candidate is well placed."""

    def __init__(self):
        super().__init__()
        self.cams = None                                              # the cameras used in the last call

    def __call__(self, crops, LOCALIZE=True):
        from oracle import crop_refine as ocr
        from oracle import homography as ohg
        trk = self.trk
        f = trk.frame_num
        _, pri = trk.filter.view(with_direction=True)
        pri = pri.detach().cpu().float()
        n = len(pri)
        centers = torch.tensor([CAM_CENTERS[k] for k in CAMERAS])
        zeros = [0.0] * len(CAMERAS)
        cam = crop_prior_restated(pri, centers, zeros, zeros, torch.zeros(n, dtype=torch.float64))[0].numpy()
        self.cams = cam
        P1, _, P2, _ = camera_matrices()
        im_objs = torch.from_numpy(ohg.wrapper_space_to_im(ohg.state_to_space(pri[:, :6].numpy()), P1[cam], P2[cam]))
        crop_boxes = ocr.get_crop_boxes(im_objs, PARAMS["b"])
        reg_boxes, _ = gc.crop_detections(im_objs, crop_boxes, n_det=N_CROP_DET, seed=CROP_SEED + f, cs=PARAMS["cs"])
        # its +-5 crop pixels are tens of feet for a distant vehicle: keep CROP_JITTER of the offset from the prior's own corners
        local = (im_objs.double() - crop_boxes[:, None, 0:2].double()) / (crop_boxes[:, 2] - crop_boxes[:, 0]).double()[:, None, None]
        local = (local * PARAMS["cs"]).float()
        base = torch.cat((local.reshape(n, 16), local[..., 0].min(1, keepdim=True).values, local[..., 1].min(1, keepdim=True).values,
                          local[..., 0].max(1, keepdim=True).values, local[..., 1].max(1, keepdim=True).values), dim=1)[:, None, :]
        t = sum(trk.timestamps) / len(trk.timestamps)
        cls = torch.zeros((n, N_CROP_DET, 8), dtype=torch.float32)
        keep = torch.full((n, N_CROP_DET), CROP_JITTER)
        for i in range(n):
            truth = np.array([true_state(vi, t)[:2] for vi in range(len(VEHICLES))])
            vi = int(np.argmin(np.abs(truth[:, 0] - float(pri[i, 0])) + 10.0 * np.abs(truth[:, 1] - float(pri[i, 1]))))
            seen = any(g >= f for g in VEHICLES[vi][8])
            levels = list(CROP_LEVELS)
            top = (i + f) % N_CROP_DET                                  # the candidate that gets levels[0]
            if not seen:
                keep[i, :] = 1.0                                        # the best placed of four faint candidates wins
                keep[i, top] = CROP_JITTER
            elif (i + f) % 5 == 0:
                levels[1] = 0.8                                         # the most confident candidate is badly placed and loses
                keep[i, top] = 1.0
            for j in range(N_CROP_DET):
                cls[i, (j + top) % N_CROP_DET, VEHICLES[vi][0]] = levels[j] * (1.0 if seen else 0.05)
        reg_boxes = (base + keep[:, :, None] * (reg_boxes - base)).contiguous()
        dev = crops.device if isinstance(crops, torch.Tensor) else "cpu"
        return reg_boxes.to(dev), cls.to(dev)


def attach(trk, detector, crop_detector):
    detector.trk = crop_detector.trk = trk
    return trk


# ---------------------------------------------------------------------------------------------- the loop on the CPU
class HostFilter:
    """Torch_KF's bookkeeping (util_track/kf.py:120-262) around oracle/kf.py."""

    def __init__(self, init):
        self.init = init
        self.F, self.H, self.Q, self.R = init["F"].float(), init["H"].float(), init["Q"].float()[None], init["R"].float()[None]
        self.mu_R = torch.zeros(1, 5)
        self.P0 = init["P"].float()[None]
        self.mu_v = init["mu_v"]
        self.dt_default = 1 / 30.0
        self.X = self.P = self.D = self.T = None
        self.ids = []

    def __len__(self):
        return len(self.ids)

    def get_dt(self, target, idxs=None):
        if type(target) == float:
            return target - self.T
        target = torch.tensor(target, dtype=torch.double)
        if idxs is None:
            return target - self.T
        dt = torch.zeros(len(self.X)) + self.dt_default
        for k, i in enumerate(idxs):
            dt[i] = target[k] - self.T[i]
        return dt

    def add(self, det, ids, directions, times, classes):
        newX = torch.zeros((len(det), 6))
        newX[:, :5] = det
        newX[:, 5] = float(self.mu_v)
        newP = self.P0.repeat(len(ids), 1, 1)
        for i, c in enumerate(classes):
            newX[i, 2:5] = self.init["class_size"][c]
            newP[i, 2:5, 2:5] = self.init["class_covariance"][c]
        newD, newT = directions.float(), torch.as_tensor(np.asarray(times), dtype=torch.double)
        if len(self.ids):
            self.X, self.P = torch.cat((self.X, newX)), torch.cat((self.P, newP))
            self.D, self.T = torch.cat((self.D, newD)), torch.cat((self.T, newT))
        else:
            self.X, self.P, self.D, self.T = newX, newP, newD, newT
        self.ids += list(ids)

    def remove(self, ids):
        keep = [i for i, oid in enumerate(self.ids) if oid not in set(ids)]
        self.X, self.P, self.D, self.T = self.X[keep], self.P[keep], self.D[keep], self.T[keep]
        self.ids = [self.ids[i] for i in keep]

    def view(self, dt=None, with_direction=False):
        from oracle import kf as okf
        if not self.ids:
            return [], []
        return list(self.ids), okf.view(self.X, self.D, self.F, dt, with_direction)

    def predict(self, dt):
        from oracle import kf as okf
        if self.ids:
            self.X, self.P, self.T = okf.predict(self.X, self.P, self.D, self.T, self.F, self.Q, dt, self.dt_default)

    def update(self, z, ids):
        from oracle import kf as okf
        rows = [self.ids.index(i) for i in ids]
        if rows:
            self.X, self.P = okf.update(self.X, self.P, rows, z, self.H, self.R, self.mu_R)


def _cross_iou(a, b):
    """md_iou of footprints a [n,4] against b [m,4], fp64 -> [n,m]."""
    A, B = a.astype(np.float64)[:, None, :], b.astype(np.float64)[None, :, :]
    area_a = (A[..., 2] - A[..., 0]) * (A[..., 3] - A[..., 1])
    area_b = (B[..., 2] - B[..., 0]) * (B[..., 3] - B[..., 1])
    minx, maxx = np.maximum(A[..., 0], B[..., 0]), np.minimum(A[..., 2], B[..., 2])
    miny, maxy = np.maximum(A[..., 1], B[..., 1]), np.minimum(A[..., 3], B[..., 3])
    inter = np.maximum(0.0, maxx - minx) * np.maximum(0.0, maxy - miny)
    return inter / (area_a + area_b - inter)


class HostTracker:
    """The frame loop of the tracker restated on the CPU from oracle/ and the restatements of the other *_cases modules.
    ``record`` receives one dict per frame with the quantities of tests/golden/tracker_run.npz."""

    def __init__(self, loaders, detector, crop_detector, early_cutoff=1000, ts=None):
        for k, v in PARAMS.items():
            setattr(self, k, v)
        self.loaders, self.detector, self.crop_detector = loaders, detector, crop_detector
        self.cameras = list(CAMERAS)
        self.sequences = [c + "_0_4k" for c in self.cameras]
        self.centers = torch.tensor([CAM_CENTERS[k] for k in self.cameras])
        self.P1, self.H1, self.P2, self.H2 = camera_matrices()
        self.filter = HostFilter(tc.kf_init())
        self.class_dict = tc.class_dict()
        self.ts = ts
        self.ts_alpha = tb.ALPHA
        self.timestamps, self.ts_bias = [0 for _ in loaders], [0 for _ in loaders]
        self.next_obj_id, self.fsld, self.all_classes = 0, {}, {}
        self.all_times, self.all_tracks, self.all_ts_bias = [], [], []
        self.cutoff_frame = early_cutoff
        self.frame_num = 0
        self.frames = []

    # -- MC3D_crop_tracker.py:197-235
    def __next__(self):
        chunks = [next(l) for l in self.loaders]
        if any(c[0] == -1 for c in chunks):
            self.frame_num = -1
            return
        self.frame_num = chunks[0][0]
        prev = list(self.timestamps)
        self.timestamps = [c[3] if c[3] is not None else prev[i] + 1 / 30.0 for i, c in enumerate(chunks)]

    def time_sync_cameras(self):
        if self.frame_num == -1:
            return
        latest = max(self.timestamps)
        for i in range(len(self.timestamps)):
            while latest - self.timestamps[i] >= 0.02:
                fr_num, _, _, stamp = next(self.loaders[i])
                if fr_num == -1:
                    self.frame_num = -1
                    return
                if self.ts is not None:
                    stamp = self.ts[self.sequences[i]][fr_num]
                    if stamp is None:
                        stamp = self.ts[self.sequences[i]][fr_num - 1] + 1 / 30.0
                elif stamp is None:
                    stamp = self.timestamps[i] + 1 / 30.0
                self.timestamps[i] = stamp

    # -- :319-383 with est_ts
    def parse(self, scores, labels, boxes, cams, rec):
        from oracle import homography as ohg
        from oracle import tracker_post as otp
        keep = scores > self.sigma_d
        labels, det, scores, cams = labels[keep], boxes[keep].reshape(-1, 10, 2)[:, :8, :], scores[keep], cams[keep]
        idxs = otp.im_nms(det, scores, groups=cams, threshold=self.phi_nms_im)
        labels, det, scores, cams = labels[idxs], det[idxs], scores[idxs], cams[idxs]
        cam, dn = cams.numpy(), det.numpy()
        heights = ohg.guess_heights(list(labels))

        def to_state(h):
            return ohg.space_to_state(ohg.wrapper_im_to_space(dn, self.H1[cam], self.H2[cam], h))
        state = to_state(heights)
        repro = ohg.wrapper_space_to_im(ohg.state_to_space(state), self.P1[cam], self.P2[cam])
        state = np.asarray(to_state(ohg.height_from_template(repro, heights, dn)), dtype=F32)
        objs = self.filter.view(with_direction=True)[1]
        if len(objs):                                                   # estimate_ts_bias (:237-315)
            r = tb.restated(state, cam, objs.numpy(), self.timestamps, self.ts_bias, self.phi_nms_space, self.ts_alpha,
                            float(self.filter.mu_v))
            if len(r["entries"]):
                self.ts_bias = r["ts_bias"]
        state = torch.from_numpy(state)
        idxs = otp.space_nms(state, scores, threshold=self.phi_nms_space)
        return state[idxs], labels[idxs], scores[idxs], cams[idxs]

    # -- :1100-1137
    def associate(self, det, labels, scores, cams, rec):
        flt = self.filter
        avg = sum(self.timestamps) / len(self.timestamps)
        pre_ids, pre_loc = flt.view(dt=flt.get_dt(avg), with_direction=True) if len(flt) else ([], [])
        m = np.zeros((0, 2), np.int64)
        if len(pre_ids) and len(det):
            cost = 1.0 - _cross_iou(tb.footprints(pre_loc.numpy()[:, :6]), tb.footprints(det.numpy()))
            rows, cols = tc.lsap_restated(cost)
            m = np.array([[r, c] for r, c in zip(rows, cols) if not cost[r, c] > 1 - self.phi_match], np.int64).reshape(-1, 2)
        if len(m):
            times = [self.timestamps[int(cams[b])] + self.ts_bias[int(cams[b])] for b in m[:, 1]]
            flt.predict(flt.get_dt(times, idxs=[int(a) for a in m[:, 0]]))
            ids = [pre_ids[a] for a in m[:, 0]]
            flt.update(det[m[:, 1], :5], ids)
            for oid, b in zip(ids, m[:, 1]):
                self.fsld[oid] = 0
                self.all_classes[oid][int(labels[b])] += 1
        matched = set(int(b) for b in m[:, 1])
        new = [i for i in range(len(det)) if i not in matched]
        updated = set(pre_ids[a] for a in m[:, 0])
        if new:
            ids = list(range(self.next_obj_id, self.next_obj_id + len(new)))
            self.next_obj_id += len(new)
            for oid, i in zip(ids, new):
                self.fsld[oid] = 0
                self.all_classes[oid] = np.zeros(8)
                self.all_classes[oid][int(labels[i])] += 1
                updated.add(oid)
            flt.add(det[new, :5], ids, det[new, 5], [self.timestamps[int(cams[i])] + self.ts_bias[int(cams[i])] for i in new],
                    [self.class_dict[int(labels[i])] for i in new])
        for oid in pre_ids:                                             # the swapped call (:1137): every prior gets +1
            self.fsld[oid] += 1
        gone = [oid for oid in pre_ids if oid not in updated and self.fsld[oid] >= self.f_max]
        for oid in gone:
            self.fsld.pop(oid)
        if gone:
            flt.remove(gone)
        rec.update(pre_ids=list(pre_ids), match=m, rm_fsld=sorted(gone))

    # -- :1146-1254
    def crop_frame(self, rec):
        from oracle import crop_refine as ocr
        from oracle import homography as ohg
        flt = self.filter
        rec.update(pre_ids=[], crop_cams=np.zeros(0, np.int64))
        if not len(flt):
            return
        _, first = flt.view(dt=1 / 30.0, with_direction=True)
        cam, dts = crop_prior_restated(first, self.centers, self.timestamps, self.ts_bias, flt.T)
        flt.predict(dts)
        pre_ids, pre_loc = flt.view(with_direction=True)
        cam_n = cam.numpy()
        im_objs = torch.from_numpy(ohg.wrapper_space_to_im(ohg.state_to_space(pre_loc[:, :6].numpy()), self.P1[cam_n], self.P2[cam_n]))
        crop_boxes = ocr.get_crop_boxes(im_objs, self.b)
        reg_boxes, cls = self.crop_detector(torch.zeros(0), LOCALIZE=True)
        det, classes, confs = ocr.refine_from_detections(reg_boxes, cls, crop_boxes, cam, pre_loc[:, :6], self.H1, self.H2, self.P1,
                                                         self.P2, cs=self.cs, cd_max=self.cd_max, W=self.W)
        flt.update(det[:, :5], pre_ids)
        for i, oid in enumerate(pre_ids):
            self.fsld[oid] = self.fsld[oid] + 1 if confs[i] < self.sigma_c else 0
            self.all_classes[oid][int(classes[i])] += 1
        rec.update(pre_ids=list(pre_ids), crop_cams=cam_n.astype(np.int64))

    # -- :482-557
    def prune(self, rec):
        from oracle import boxes as oboxes
        flt = self.filter
        rec.update(rm_over=[], rm_anom=[])
        for phase in ("over", "anom"):
            if not len(flt):
                return
            ids, b = flt.view(dt=flt.get_dt(max(self.timestamps)), with_direction=True)
            if phase == "over":
                fp = torch.from_numpy(tb.footprints(b.numpy()[:, :6]))
                keep = set(oboxes.greedy_nms(fp, torch.full((len(ids),), 8.0), self.phi_over).tolist())
                gone = [ids[i] for i in range(len(ids)) if i not in keep]
            else:
                ms = self.max_size
                bad = (b[:, 1] > 120) | (b[:, 1] < -10) | (b[:, 2] > ms[0]) | (b[:, 2] < 0) | (b[:, 3] > ms[1]) | (b[:, 3] < 0)
                bad |= (b[:, 4] > ms[2]) | (b[:, 4] < 0) | (b[:, 6] > 150) | (b[:, 6] < -150)
                bad |= (b[:, 0] < self.x_range[0]) | (b[:, 0] > self.x_range[1])
                gone = [ids[i] for i in bad.nonzero().reshape(-1).tolist()]
            if gone:
                flt.remove(gone)
            rec["rm_" + phase] = sorted(gone)

    def track(self, record=None):
        next(self)
        self.time_sync_cameras()
        while self.frame_num != -1:
            rec = dict(frame_num=self.frame_num, timestamps=list(self.timestamps), match=np.zeros((0, 2), np.int64), rm_fsld=[],
                       crop_cams=np.zeros(0, np.int64))
            if self.frame_num % self.d == 0:
                scores, labels, boxes, cams = self.detector(torch.zeros(0), MULTI_FRAME=True)
                self.associate(*self.parse(scores, labels, boxes, cams, rec), rec)
            elif self.frame_num % self.s == 0:
                self.crop_frame(rec)
            self.prune(rec)
            clock = sum(self.timestamps) / len(self.timestamps)
            self.all_times.append(clock)
            rows = np.zeros((0, 7), F32)
            if len(self.filter):
                ids, loc = self.filter.view(dt=self.filter.get_dt(clock), with_direction=True)
                rows = loc.numpy().copy()
                for oid, row in zip(ids, loc):
                    self.all_tracks.append([oid, clock, row.clone()])
                    self.all_ts_bias.append(list(self.ts_bias))
            rec.update(stored=rows, **snapshot(self))
            if record is not None:
                record(rec)
            next(self)
            self.time_sync_cameras()
            if self.frame_num > self.cutoff_frame:
                break


def snapshot(trk):
    """The per-frame state every implementation is compared on: works on HostTracker, on mc3d_tracker.MC_Crop_Tracker and
    on the reference's stand-in (filter.view() gives the ids in row order on all three)."""
    flt = trk.filter
    n = 0 if flt.X is None else len(flt.X)
    ids = list(flt.view()[0]) if n else []

    def host(t, shape):
        return t.detach().cpu().numpy().copy() if n else np.zeros(shape, np.float64 if shape == (0,) else F32)
    fk, ck = sorted(trk.fsld), sorted(trk.all_classes)
    return dict(ids=np.array(ids, np.int64), X=host(flt.X, (0, 6)), P=host(flt.P, (0, 6, 6)), T=host(flt.T, (0,)),
                fsld=np.array([[k, trk.fsld[k]] for k in fk], np.int64).reshape(-1, 2),
                class_ids=np.array(ck, np.int64), classes=np.array([trk.all_classes[k] for k in ck], np.float64).reshape(-1, 8),
                next_obj_id=int(trk.next_obj_id), ts_bias=np.array([float(b) for b in trk.ts_bias], np.float64))


FRAME_KEYS = ("frame_num", "timestamps", "crop_cams", "pre_ids", "match", "rm_fsld", "rm_over", "rm_anom", "fsld", "class_ids",
              "classes", "next_obj_id", "ts_bias", "ids", "X", "P", "T", "stored")
DISCRETE_KEYS = ("frame_num", "timestamps", "crop_cams", "pre_ids", "match", "rm_fsld", "rm_over", "rm_anom", "fsld", "class_ids",
                 "classes", "next_obj_id", "ids")


def run_host(early_cutoff=1000):
    """The scene through HostTracker -> (tracker, list of per-frame records)."""
    det, cd = StandInDetector(), StandInCropDetector()
    trk = attach(HostTracker([ScriptedLoader(c) for c in range(3)], det, cd, early_cutoff=early_cutoff, ts=ts_table()), det, cd)
    recs = []
    trk.track(recs.append)
    return trk, recs

#!/usr/bin/env python3
"""The tracker's frame loop (mc3d_tracker.MC_Crop_Tracker.track) at the reference's scale: 18 cameras, about 100 live
tracks, detection and crop frames alternating, stand-in detectors (tests/tracker_cases.py) that cost no GPU time.

Prints frames/s of the tracker's own work (wall time of track() minus the time spent inside the stand-ins, which are host
numpy; the device is drained before each stand-in call so that queued tracker work is not booked to it), the number of
device -> host copies per detection frame and per crop frame (every Tensor.cpu / item / tolist / int() / float() /
bool() of a device tensor outside the stand-ins), and the same loop through the CPU restatement (tracker_cases.HostTracker)
beside it.

The scene is tracker_cases' with its constants replaced: 18 overhead cameras 150 ft apart (affine, so the image <-> road
transforms invert exactly anywhere), 100 vehicles in 10 lanes, none of the special events of the test scene.

    python tools/bench_tracker.py [--frames 60] [--host-frames 12]
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import track_cases as tc                    # noqa: E402
import tracker_cases as trc                 # noqa: E402

N_CAM, N_LANES, PER_LANE = 18, 10, 10


def install_scene(n_frames):
    names = ["p%dc%d" % (p, c) for p in (1, 2, 3) for c in range(1, 7)]
    cx = [100 + 150 * k for k in range(N_CAM)]
    trc.CAMERAS = names
    trc.CAM_CENTERS = {n: (x, 60) for n, x in zip(names, cx)}
    trc.camera_of = lambda x: int(np.argmin([abs(x - c) for c in cx]))
    trc.TRUE_BIAS = [0.0] + [0.002 * ((5 * k) % 7 - 3) for k in range(1, N_CAM)]
    trc.N_FRAMES = n_frames
    trc.DUPLICATE, trc.GLITCH = (-1, 0.0), (-1, -1, 0.0)
    trc.PARAMS = dict(trc.PARAMS, x_range=[0, 3000])
    sizes = [tc.CLASS_SIZE[tc.CLASS_NAMES[k]] for k in range(4)]
    trc.VEHICLES = []
    for j in range(N_LANES):
        d = 1 if j < N_LANES // 2 else -1
        y = 6.0 + 12.0 * j if d > 0 else 66.0 + 12.0 * (j - N_LANES // 2)
        for i in range(PER_LANE):
            lab = (i + j) % 4
            l, w, h = sizes[lab]
            trc.VEHICLES.append((lab, d, 150.0 + 260.0 * i + 13.0 * j, y, l + 0.4, w + 0.1, h + 0.1, 75.0 + (3 * i + j) % 10,
                                 range(0, n_frames + 1), False))

    def stamps():
        return [[trc.T0 + j / 30.0 + 0.0005 * c for j in range(n_frames)] for c in range(N_CAM)]
    trc.stamps = stamps
    P = np.stack([np.array([[4.0, 0.5, 0.0, 960 - 4.0 * c], [0.3, 6.0, -3.0, 100.0], [0, 0, 0, 1.0]]) for c in cx])
    H = np.stack([np.linalg.inv(p[:, [0, 1, 3]]) for p in P])
    trc.camera_matrices = lambda: (P, H, P, H)
    return names, P, H


class Timed:
    """A stand-in network whose host time and device -> host copies are kept out of the tracker's account."""

    def __init__(self, inner, account):
        self.inner, self.account = inner, account

    def to(self, device):
        return self

    def eval(self):
        return self

    def __call__(self, *a, **k):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.account["counting"] = False
        t0 = time.perf_counter()
        try:
            return self.inner(*a, **k)
        finally:
            self.account["stand_in"] += time.perf_counter() - t0
            self.account["counting"] = True


@contextlib.contextmanager
def count_copies(account):
    names = ("cpu", "item", "tolist", "__int__", "__float__", "__bool__", "__index__")
    keep = {n: getattr(torch.Tensor, n) for n in names}

    def wrap(fn):
        def counted(self, *a, **k):
            if self.is_cuda and account["counting"] and not account["inside"]:
                account["copies"] += 1
                account["inside"] = True
                try:
                    return fn(self, *a, **k)
                finally:
                    account["inside"] = False
            return fn(self, *a, **k)
        return counted
    for n in names:
        setattr(torch.Tensor, n, wrap(keep[n]))
    try:
        yield
    finally:
        for n in names:
            setattr(torch.Tensor, n, keep[n])


def run_gpu(names, P, H, n_frames):
    import homography as hgm
    from mc3d_tracker import MC_Crop_Tracker
    dev = torch.device("cuda:0")
    account = dict(stand_in=0.0, copies=0, counting=True, inside=False)
    per_kind = {"detection": [], "crop": []}

    class Counted(MC_Crop_Tracker):
        def __next__(self):
            if getattr(self, "_started", False):
                kind = "detection" if self.frame_num % self.d == 0 else "crop"
                per_kind[kind].append((account["copies"] - self._mark, 0 if self.filter.X is None else len(self.filter.X)))
            self._started, self._mark = True, account["copies"]
            return super().__next__()

    def make_hg():
        hg = hgm.Homography(device=dev)
        hg.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    det, cd = trc.StandInDetector(), trc.StandInCropDetector()
    params = dict(trc.PARAMS, cam_centers=dict(trc.CAM_CENTERS))
    with contextlib.redirect_stdout(io.StringIO()):
        trk = Counted([trc.ScriptedLoader(c, device=dev) for c in range(N_CAM)], Timed(det, account), tc.kf_init(),
                      hgm.Homography_Wrapper(hg1=make_hg(), hg2=make_hg()), tc.class_dict(), params=params, cd=Timed(cd, account),
                      PLOT=False)
    trc.attach(trk, det, cd)
    with count_copies(account), contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trk.track()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    frames = len(trk.all_times)
    own = wall - account["stand_in"]
    print("GPU tracker: %d frames of %d cameras in %.3f s, %.3f s of it inside the stand-in detectors" % (frames, N_CAM, wall, account["stand_in"]))
    print("  the tracker's own work: %.1f frames/s (%.2f ms per frame)" % (frames / own, 1e3 * own / frames))
    for kind, rows in per_kind.items():
        rows = rows[2:]                                              # the first frame of each kind has no tracks yet
        if rows:
            print("  %-9s frames: %.1f device -> host copies per frame (min %d, max %d), %.0f live tracks"
                  % (kind, np.mean([r[0] for r in rows]), min(r[0] for r in rows), max(r[0] for r in rows), np.mean([r[1] for r in rows])))
    t0 = time.perf_counter()
    n_rows = len(trk.all_tracks)
    print("  all_tracks: %d rows in one device -> host copy, %.2f ms; log chunks %s" % (n_rows, 1e3 * (time.perf_counter() - t0),
                                                                                       [len(c) for c in trk.track_log.chunks]))
    print("  time_metrics (host wall time, s):", {k: round(v, 3) for k, v in trk.time_metrics.items() if v})
    return trk


def run_host(n_frames):
    account = dict(stand_in=0.0, copies=0, counting=True, inside=False)
    det, cd = trc.StandInDetector(), trc.StandInCropDetector()
    trk = trc.attach(trc.HostTracker([trc.ScriptedLoader(c) for c in range(N_CAM)], Timed(det, account), Timed(cd, account),
                                     early_cutoff=n_frames - 2), det, cd)
    t0 = time.perf_counter()
    trk.track()
    wall = time.perf_counter() - t0
    frames = len(trk.all_times)
    own = wall - account["stand_in"]
    print("CPU restatement (tests/tracker_cases.py: HostTracker, numpy / torch CPU): %d frames, own work %.2f frames/s (%.1f ms per frame), "
          "%d live tracks at the end" % (frames, frames / own, 1e3 * own / frames, len(trk.filter)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--host-frames", type=int, default=12)
    a = ap.parse_args()
    names, P, H = install_scene(a.frames)
    print("bench_tracker: %d cameras, %d vehicles, d = %d, s = %d, cd_max = %d with %d crop candidates"
          % (N_CAM, len(trc.VEHICLES), trc.PARAMS["d"], trc.PARAMS["s"], trc.PARAMS["cd_max"], trc.N_CROP_DET))
    if torch.cuda.is_available():
        print(torch.cuda.get_device_name(0))
        run_gpu(names, P, H, 8)                                      # warm-up: library load, allocator
        print("-- timed run")
        install_scene(a.frames)
        run_gpu(names, P, H, a.frames)
    else:
        print("no GPU: only the CPU restatement runs")
    install_scene(a.host_frames)
    run_host(a.host_frames)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/tracker_run.npz by running the REFERENCE's own ``MC_Crop_Tracker.track()`` and
``write_results_csv()`` on the scene of tests/tracker_cases.py -- build container only.

The reference class cannot be constructed here (its ``__init__`` opens a pickle on its author's machine, starts cv2 video
loaders and asks for a CUDA device), so its methods -- ``track``, ``__next__``, ``time_sync_cameras``, ``parse_detections``,
``estimate_ts_bias``, ``match_hungarian``, ``manage_tracks``, ... -- are bound, unmodified, onto a small stand-in class
that carries the attributes ``__init__`` would have set: the reference's own ``Torch_KF`` on the CPU, the reference's
``Homography_Wrapper`` filled with the fixture's camera matrices, the scripted loaders and stand-in detectors of
tests/tracker_cases.py, ``PLOT=False``.  Harness shims, for the duration of the call only: ``torchvision.ops.nms`` /
``roi_align`` are this repository's restatements (oracle/boxes.py, oracle/crop_refine.py; precedent: tools/make_golden.py
gen_tracker_post / gen_crop_refine), ``cv2.destroyAllWindows`` and ``torch.cuda.synchronize`` / ``empty_cache`` are no-ops
(``track()`` calls them at :1295-1296 and :1312; this torch build has no device).  Nothing of the reference is copied.

Thin wrappers around the bound methods record, per frame, what the tests compare (tests/tracker_cases.py: FRAME_KEYS) and
measure how far every discrete decision of the run is from flipping.  The fixture is only written if
  * the filter never holds exactly 6 rows when a per-object dt is predicted (the reference's Q broadcast, see
    tests/track_cases.py: sequence), and
  * every kind of decision keeps a margin of at least 100 x the state tolerance (tracker_cases.MARGIN) over its
    runner-up; the smallest margin of each kind is stored as ``margin_<kind>``.  Margins are relative: a difference of
    IoUs, confidences or selection scores as it stands (they live in [0, 1]); a distance to a removal threshold or between
    two camera distances divided by max(1, |threshold|) resp. max(1, nearest distance).
This script refuses to run without the reference and is never executed on the GPU box.

    python tools/make_golden_tracker.py [--out DIR]
"""
import contextlib
import csv
import io
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402  (REF, the stand-ins; puts the package and tests/ on sys.path)
import track_cases as tc                    # noqa: E402
import tracker_cases as trc                 # noqa: E402
import ts_bias_cases as tb                  # noqa: E402
import golden_cases as gc                   # noqa: E402
from oracle import boxes as oboxes          # noqa: E402
from oracle import crop_refine as ocr       # noqa: E402
from oracle import tracker_post as otp      # noqa: E402

BOUND = ("track", "__next__", "time_sync_cameras", "estimate_ts_bias", "parse_detections", "manage_tracks", "increment_fslds",
         "remove_overlaps", "remove_anomalies", "im_nms", "space_nms", "match_hungarian", "get_crop_boxes", "local_to_global",
         "select_best_box", "md_iou", "write_results_csv")


class Margins(dict):
    def see(self, kind, value):
        self[kind] = min(self.get(kind, np.inf), float(value))


def build_stand_in(trk_mod, hgmod, kfmod, margins, frames, early_cutoff):
    T = trk_mod.MC_Crop_Tracker

    class StandIn:
        """Carries what MC_Crop_Tracker.__init__ (:37-195) sets; a class, because ``next(self)`` looks ``__next__`` up on the type."""
    for name in BOUND:
        setattr(StandIn, name, getattr(T, name))
    me = StandIn()
    for k, v in trc.PARAMS.items():
        setattr(me, k, v)
    me.sigma_min, me.q, me.est_ts, me.ts_alpha = 0.5, 1, True, 0.05
    me.device = torch.device("cpu")
    me.state_size = 7
    me.filter = kfmod.Torch_KF(torch.device("cpu"), INIT=tc.kf_init())
    names, _, _, (Ps, Hs), (Ps2, Hs2) = gc.homography_inputs()

    def make_hg(P, H):
        hg = hgmod.Homography()
        hg.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    me.hg = hgmod.Homography_Wrapper(hg1=make_hg(Ps, Hs), hg2=make_hg(Ps2, Hs2))
    me.class_dict = tc.class_dict()
    me.detector, me.crop_detector = trc.StandInDetector(), trc.StandInCropDetector()
    trc.attach(me, me.detector, me.crop_detector)
    me.cameras = list(trc.CAMERAS)
    me.sequences = [c + "_0_4k" for c in me.cameras]
    me.loaders = [trc.ScriptedLoader(c) for c in range(len(me.cameras))]
    me.n_frames = len(me.loaders[0])
    me.centers = torch.tensor([trc.CAM_CENTERS[k] for k in me.cameras])
    me.output_file = None
    me.next_obj_id, me.fsld = 0, {}
    me.all_tracks, me.all_classes, me.all_confs, me.all_cameras, me.all_times, me.all_ts_bias = [], {}, {}, {}, [], []
    me.time_metrics = {k: 0 for k in ("load", "predict", "crop and align", "localize", "post localize", "detect", "parse", "match",
                                      "update", "add and remove", "store", "plot")}
    me.PLOT = False
    me.cutoff_frame = early_cutoff
    me.ts = trc.ts_table()
    me.timestamps, me.ts_bias = [0 for _ in me.loaders], [0 for _ in me.loaders]

    # ---- recording: thin wrappers that call straight through to the reference's methods
    cur = dict(match=np.zeros((0, 2), np.int64), pre_ids=[], crop_cams=np.zeros(0, np.int64), rm={}, stored_from=0)
    phase = ["none"]
    remove = me.filter.remove

    def logged_remove(ids):
        cur["rm"][phase[0]] = sorted(int(i) for i in ids)
        remove(ids)
    me.filter.remove = logged_remove

    def in_phase(name, ph, before=None):
        fn = getattr(T, name)

        def wrapped(self, *a, **k):
            phase[0] = ph
            if before is not None:
                before(self, *a, **k)
            try:
                return fn(self, *a, **k)
            finally:
                phase[0] = "none"
        setattr(StandIn, name, wrapped)

    def anomaly_margins(self, x_bounds=None):
        if self.filter.X is None or len(self.filter.X) == 0:
            return
        _, b = self.filter.view(with_direction=True, dt=self.filter.get_dt(max(self.timestamps)))
        b = b.double().numpy()
        ms = [float(v) for v in self.max_size]
        for col, bounds in ((1, (120, -10)), (2, (ms[0], 0)), (3, (ms[1], 0)), (4, (ms[2], 0)), (6, (150, -150)), (0, tuple(x_bounds))):
            for bound in bounds:
                margins.see("removal", np.abs(b[:, col] - bound).min() / max(1.0, abs(bound)))
    in_phase("increment_fslds", "fsld")
    in_phase("remove_overlaps", "over")
    in_phase("remove_anomalies", "anom", before=anomaly_margins)

    def match_hungarian(self, first, second):
        out = T.match_hungarian(self, first, second)
        cur["match"] = np.asarray(out, dtype=np.int64).reshape(-1, 2)
        if len(first) and len(second):
            iou = trc._cross_iou(tb.footprints(first.numpy()[:, :6]), tb.footprints(second.numpy()[:, :6]))
            rows, cols = tc.lsap_restated(1.0 - iou)
            margins.see("match_iou", np.abs(iou[rows, cols] - self.phi_match).min())
            kept = [(r, c) for r, c in zip(rows, cols) if not (1.0 - iou[r, c]) > 1 - self.phi_match]
            assert np.array_equal(np.array(kept, np.int64).reshape(-1, 2), cur["match"])
            if len(kept):                                              # a per-object dt is predicted next (:1122-1126)
                assert len(self.filter.X) != 6, "see tests/track_cases.py: sequence (Q broadcast at 6 rows)"
        return out
    StandIn.match_hungarian = match_hungarian

    def manage_tracks(self, detections, matchings, pre_ids, *a, **k):
        cur["pre_ids"] = [int(i) for i in pre_ids]
        return T.manage_tracks(self, detections, matchings, pre_ids, *a, **k)
    StandIn.manage_tracks = manage_tracks

    def parse_detections(self, scores, *a, **k):
        margins.see("score_sigma_d", (scores - self.sigma_d).abs().min())
        return T.parse_detections(self, scores, *a, **k)
    StandIn.parse_detections = parse_detections

    view = me.filter.view

    def logged_view(dt=None, with_direction=False):
        ids, out = view(dt=dt, with_direction=with_direction)
        if isinstance(dt, float) and dt == 1 / 30.0 and len(ids):       # the crop frame's first view (:1150)
            assert len(ids) != 6, "see tests/track_cases.py: sequence (Q broadcast at 6 rows)"
            c = me.centers.double()
            d = ((c[None, :, 0] - out[:, None, 0].double()) ** 2 + (c[None, :, 1] - out[:, None, 1].double()) ** 2).sort(dim=1).values
            margins.see("camera", ((d[:, 1] - d[:, 0]) / d[:, 0].clamp(min=1.0)).min())
            cur["crop_view"] = True
        return ids, out
    me.filter.view = logged_view

    state_to_im = me.hg.state_to_im

    def logged_state_to_im(points, name=None):
        if isinstance(name, list) and cur["crop_view"] and not cur["crop_seen"]:               # the crop frame's priors (:1174)
            cur["crop_seen"] = True
            cur["crop_cams"] = np.array([me.cameras.index(n) for n in name], np.int64)
        return state_to_im(points, name=name)
    me.hg.state_to_im = logged_state_to_im
    cur["crop_seen"] = cur["crop_view"] = False

    def select_best_box(self, a_priori, preds, confs, classes, n_objs):
        out = T.select_best_box(self, a_priori, preds, confs, classes, n_objs)
        cur["pre_ids"] = [int(i) for i in self.filter.view()[0]]
        foot = otp.space_boxes(preds).reshape(n_objs, -1, 4)
        prior = otp.space_boxes(a_priori[:, :6])[:, None, :].repeat(1, foot.shape[1], 1)
        s = ((1 - self.W) * otp.md_iou(foot.double(), prior.double()) + self.W * confs).sort(dim=1, descending=True).values
        margins.see("best_box", (s[:, 0] - s[:, 1]).min())
        margins.see("conf_sigma_c", (out[2] - self.sigma_c).abs().min())
        assert np.array_equal(self.crop_detector.cams, cur["crop_cams"]), "the stand-in crop detector used other cameras"
        return out
    StandIn.select_best_box = select_best_box

    def nms(boxes, scores, thr):
        b = boxes.double()
        if len(b) > 1:
            iou = trc._cross_iou(b.numpy(), b.numpy())
            iou = iou[np.triu_indices(len(b), 1)]
            if np.isfinite(iou).any():
                margins.see("nms", np.abs(iou[np.isfinite(iou)] - thr).min())
        return oboxes.greedy_nms(boxes, scores, thr)

    def nxt(self):
        if cur.get("started"):                                        # a frame has just been stored (:1266-1282)
            rows = self.all_tracks[cur["stored_from"]:]
            rec = dict(frame_num=self.frame_num, timestamps=list(self.timestamps), match=cur["match"], pre_ids=cur["pre_ids"],
                       crop_cams=cur["crop_cams"], rm_fsld=cur["rm"].get("fsld", []), rm_over=cur["rm"].get("over", []),
                       rm_anom=cur["rm"].get("anom", []),
                       stored=np.stack([r[2].numpy() for r in rows]).astype(np.float32) if rows else np.zeros((0, 7), np.float32))
            assert [r[0] for r in rows] == list(self.filter.view()[0] if len(rows) else [])
            rec.update(trc.snapshot(self))
            frames.append(rec)
        cur.update(started=True, match=np.zeros((0, 2), np.int64), pre_ids=[], crop_cams=np.zeros(0, np.int64), rm={},
                   stored_from=len(self.all_tracks), crop_seen=False, crop_view=False)
        return T.__next__(self)
    StandIn.__next__ = nxt
    return me, nms


@contextlib.contextmanager
def shims(trk_mod, nms):
    def roi_align(frames, rois, output_size):
        return torch.from_numpy(ocr.roi_align(frames.numpy(), rois.numpy(), output_size))
    keep = (trk_mod.nms, trk_mod.roi_align, torch.cuda.synchronize, torch.cuda.empty_cache)
    trk_mod.nms, trk_mod.roi_align = nms, roi_align
    trk_mod.cv2.destroyAllWindows = lambda: None
    torch.cuda.synchronize = torch.cuda.empty_cache = lambda *a, **k: None
    try:
        yield
    finally:
        trk_mod.nms, trk_mod.roi_align, torch.cuda.synchronize, torch.cuda.empty_cache = keep
        del trk_mod.cv2.destroyAllWindows


def run_reference(trk_mod, hgmod, kfmod, margins, early_cutoff=1000, write_csv=False):
    frames = []
    me, nms = build_stand_in(trk_mod, hgmod, kfmod, margins, frames, early_cutoff)
    rows = None
    with shims(trk_mod, nms), contextlib.redirect_stdout(io.StringIO()):
        me.track()
        if write_csv:
            with tempfile.TemporaryDirectory() as tmp:
                me.output_file = os.path.join(tmp, "results.csv")
                me.write_results_csv()
                with open(me.output_file, newline="") as f:
                    rows = list(csv.reader(f))[1:]
    return me, frames, rows


def main(out_dir):
    if not os.path.isfile(os.path.join(mg.REF, "MC3D_crop_tracker.py")):
        raise SystemExit("the reference checkout (%s) is needed to write this fixture" % mg.REF)
    mg.install_shims()
    mg.tracker_import_shims()
    trk_mod, hgmod = mg.import_reference_tracker()
    kfmod = mg.ref_module_from_file("_reference_util_track_kf", "util_track/kf.py")
    margins = Margins()
    me, frames, rows = run_reference(trk_mod, hgmod, kfmod, margins, write_csv=True)
    out = {}
    for f, rec in enumerate(frames):
        for k in trc.FRAME_KEYS:
            v = rec[k]
            out["f%d_%s" % (f, k)] = np.asarray(v, dtype=np.int64) if k in ("pre_ids", "rm_fsld", "rm_over", "rm_anom", "frame_num",
                                                                              "next_obj_id") else np.asarray(v)
    out["n_frames"] = np.array(len(frames), np.int64)
    out["all_times"] = np.array(me.all_times, np.float64)
    out["csv_id"] = np.array([int(r[2]) for r in rows], np.int64)
    out["csv_time"] = np.array([float(r[1]) for r in rows], np.float64)
    out["csv_class"] = np.array([r[3] for r in rows])
    out["csv_state"] = np.array([[float(r[k]) for k in (39, 40, 43, 42, 44, 35, 38)] for r in rows], np.float32)   # x y l w h dir v
    # the scene does what it was written for
    rm = {ph: sum((list(rec["rm_" + ph]) for rec in frames), []) for ph in ("fsld", "over", "anom")}
    assert len(frames) == 14 and [rec["frame_num"] for rec in frames] == list(range(14)), [rec["frame_num"] for rec in frames]
    assert len(rm["fsld"]) >= 1 and len(rm["over"]) >= 1 and len(rm["anom"]) >= 2, rm
    assert any(len(set(rec["crop_cams"].tolist())) == 3 for rec in frames)
    assert sum(len(rec["match"]) for rec in frames) >= 40 and frames[-1]["next_obj_id"] >= 13
    moved = sum(not np.array_equal(a["ts_bias"], b["ts_bias"]) for a, b in zip(frames, frames[1:]))
    assert moved >= 5, moved
    assert len(rows) == sum(len(rec["stored"]) for rec in frames)
    for kind in ("camera", "match_iou", "conf_sigma_c", "score_sigma_d", "best_box", "nms", "removal"):
        out["margin_" + kind] = np.array(margins[kind], np.float64)
        print("margin %-14s %.4g" % (kind, margins[kind]))
    low = {k: v for k, v in margins.items() if not v >= trc.MARGIN}
    if low:
        raise SystemExit("decisions closer than %g to their runner-up: %s -- change the scene" % (trc.MARGIN, low))
    # the early cutoff: the reference's own rule, a prefix of the full run
    _, short, _ = run_reference(trk_mod, hgmod, kfmod, Margins(), early_cutoff=trc.EARLY_CUTOFF)
    out["cutoff_frames"] = np.array(len(short), np.int64)
    for a, b in zip(short, frames):
        for k in trc.FRAME_KEYS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, "tracker_run.npz"), **out)
    print("wrote", os.path.join(out_dir, "tracker_run.npz"), "-", len(frames), "frames,", len(rows), "rows,", out["cutoff_frames"],
          "frames to the cutoff")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)

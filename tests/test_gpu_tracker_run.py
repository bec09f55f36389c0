"""GPU: ``mc3d_tracker.MC_Crop_Tracker.track()`` on the scene of tests/tracker_cases.py with the stand-in detectors, frame by
frame against the reference's own ``track()`` run (tests/golden/tracker_run.npz); the result file; the early cutoff; the
``Frames4K`` loader; the device track log across chunk boundaries."""
import csv

import numpy as np
import pytest
import torch

import frames4k_cases as fc
import golden_cases as gc
import track_cases as tc
import tracker_cases as trc
import ts_bias_cases as tb

pytestmark = pytest.mark.gpu

X_BOUND = trc.STATE_TOL       # relative to max(1, |want|.max()), tests/test_gpu_track_assoc.py:174-180
T_BOUND = 1e-9


def _hg(dev):
    import homography as hgm
    names, _, _, (P, H), (P2, H2) = gc.homography_inputs()

    def make_hg(Pm, Hm):
        hg = hgm.Homography(device=dev)
        hg.correspondence = {n: {"P": Pm[i], "H": Hm[i], "H_inv": np.linalg.inv(Hm[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    return hgm.Homography_Wrapper(hg1=make_hg(P, H), hg2=make_hg(P2, H2))


def _tracker(dev, read_every_frame=False, **kw):
    """The tracker with thin recording overrides: every override calls straight through."""
    from mc3d_tracker import MC_Crop_Tracker

    class Recorded(MC_Crop_Tracker):
        def __next__(self):
            if getattr(self, "_started", False):
                rec = dict(frame_num=self.frame_num, timestamps=list(self.timestamps), **self._cur)
                for ph in ("fsld", "over", "anom"):
                    rec["rm_" + ph] = self._rm.get(ph, [])
                rec.update(trc.snapshot(self))
                rec["allowed_bias"] = self.allowed_bias
                self.records.append(rec)
                if read_every_frame:
                    self.reads.append([(i, t, s.clone()) for i, t, s in self.all_tracks])
            self._started = True
            self._cur = dict(pre_ids=[], match=np.zeros((0, 2), np.int64), crop_cams=np.zeros(0, np.int64))
            self._rm = {}
            return super().__next__()

        def associate(self, *a):
            pre_ids, matchings = super().associate(*a)
            m = matchings.cpu().numpy() if isinstance(matchings, torch.Tensor) else np.asarray(matchings)
            self._cur.update(pre_ids=[int(i) for i in pre_ids], match=m.reshape(-1, 2).astype(np.int64))
            return pre_ids, matchings

        def _crop_frame(self):
            super()._crop_frame()
            ids = self.filter.view()[0]
            if len(ids):
                self._cur.update(pre_ids=[int(i) for i in ids], crop_cams=np.asarray(self.crop_cameras, np.int64))

        def _phase(self, ph, fn, *a, **k):
            self._ph = ph
            try:
                return fn(*a, **k)
            finally:
                self._ph = "none"

        def increment_fslds(self, *a):
            return self._phase("fsld", super().increment_fslds, *a)

        def remove_overlaps(self):
            return self._phase("over", super().remove_overlaps)

        def remove_anomalies(self, **k):
            return self._phase("anom", super().remove_anomalies, **k)

        def estimate_ts_bias(self, boxes, cams):
            view = self.filter.view(with_direction=True)[1]
            if len(view) and len(cams):                   # the summation order of the two mean speeds is free: carried forward
                self.allowed_bias += tb.ulp_bound(boxes.cpu().numpy()[:, :6], cams.cpu().numpy(), view.cpu().numpy(), self.timestamps,
                                                  [float(b) for b in self.ts_bias], self.phi_nms_space, self.ts_alpha, float(self.filter.mu_v))
            return super().estimate_ts_bias(boxes, cams)

    det, cd = trc.StandInDetector(), trc.StandInCropDetector()
    params = dict(trc.PARAMS, cam_centers=dict(trc.CAM_CENTERS), ts=trc.ts_table(), GPU=dev.index or 0)
    params.update(kw.pop("params", {}))
    trk = Recorded([trc.ScriptedLoader(c, device=dev) for c in range(3)], det, tc.kf_init(), _hg(dev), tc.class_dict(), params=params,
                   cd=cd, PLOT=False, **kw)
    trk.records, trk.reads, trk.allowed_bias, trk._ph = [], [], 0.0, "none"
    remove = trk.filter.remove

    def logged_remove(ids):
        trk._rm[trk._ph] = sorted(int(i) for i in ids)
        remove(ids)
    trk.filter.remove = logged_remove
    return trc.attach(trk, det, cd)


@pytest.fixture(scope="module")
def full_run(dev):
    trk = _tracker(dev)
    trk.track()
    return trk


def _rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


def test_every_frame_against_the_reference_run(full_run, golden):
    g = golden("tracker_run")
    trk = full_run
    assert len(trk.records) == int(g["n_frames"])
    rows = trk.all_tracks
    assert trk.track_log.copies == 1                                   # one device -> host copy for the whole log
    worst = dict(X=0.0, P=0.0, stored=0.0, T=0.0, ts_bias=0.0)
    r0 = 0
    for f, rec in enumerate(trk.records):
        for k in trc.DISCRETE_KEYS:
            assert np.array_equal(np.asarray(rec[k]), g["f%d_%s" % (f, k)]), (f, k, rec[k], g["f%d_%s" % (f, k)])
        n = len(rec["ids"])
        assert [r[0] for r in rows[r0:r0 + n]] == rec["ids"].tolist() and all(r[1] == trk.all_times[f] for r in rows[r0:r0 + n])
        stored = torch.stack([r[2] for r in rows[r0:r0 + n]]).numpy() if n else np.zeros((0, 7), np.float32)
        r0 += n
        e = dict(X=_rel(rec["X"], g["f%d_X" % f]), P=_rel(rec["P"], g["f%d_P" % f]), stored=_rel(stored, g["f%d_stored" % f]),
                 T=float(np.abs(rec["T"] - g["f%d_T" % f]).max()) if n else 0.0,
                 ts_bias=float(np.abs(rec["ts_bias"] - g["f%d_ts_bias" % f]).max()))
        print("frame %2d: X %.2e P %.2e stored %.2e T %.2e ts_bias %.2e (allowed %.2e)"
              % (f, e["X"], e["P"], e["stored"], e["T"], e["ts_bias"], rec["allowed_bias"]))
        for k in worst:
            worst[k] = max(worst[k], e[k])
        assert e["X"] <= X_BOUND and e["P"] <= X_BOUND and e["stored"] <= X_BOUND, (f, e)
        assert e["T"] <= T_BOUND + rec["allowed_bias"], (f, e)
        assert e["ts_bias"] <= rec["allowed_bias"], (f, e)
    assert r0 == len(rows) == len(trk.all_ts_bias)
    print("worst:", worst)
    assert trk.all_times == g["all_times"].tolist()


def test_result_file(full_run, golden, tmp_path):
    g = golden("tracker_run")
    trk = full_run
    trk.output_file = str(tmp_path / "results.csv")
    trk.write_results_csv()
    with open(trk.output_file, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0][-1] == "ts_bias for cameras {}".format(trc.CAMERAS) and len(rows[0]) == 46
    rows = rows[1:]
    assert [int(r[2]) for r in rows] == g["csv_id"].tolist()
    assert [float(r[1]) for r in rows] == g["csv_time"].tolist()
    assert [r[3] for r in rows] == g["csv_class"].tolist()
    state = np.array([[float(r[k]) for k in (39, 40, 43, 42, 44, 35, 38)] for r in rows], np.float32)
    e = _rel(state, g["csv_state"])
    print("state columns of the result file: %.2e" % e)
    assert e <= X_BOUND


def test_early_cutoff_stops_where_the_reference_stops(dev, full_run, golden):
    g = golden("tracker_run")
    trk = _tracker(dev, early_cutoff=trc.EARLY_CUTOFF)
    trk.track()
    assert len(trk.records) == int(g["cutoff_frames"]) and trk.frame_num == trc.EARLY_CUTOFF + 1
    for a, b in zip(trk.records, full_run.records):
        for k in trc.FRAME_KEYS:
            if k != "stored":
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    short, full = trk.all_tracks, full_run.all_tracks
    assert len(short) == sum(len(r["ids"]) for r in trk.records)
    for a, b in zip(short, full):
        assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])


def test_track_log_across_chunks(dev, full_run):
    """A first chunk of 16 rows: the log grows several times during the run.  Reading all_tracks after every frame and
    reading it once at the end give the same list as the run with the default chunk."""
    every = _tracker(dev, read_every_frame=True, params=dict(log_rows=16))
    every.track()
    once = _tracker(dev, params=dict(log_rows=16))
    once.track()
    assert len(once.track_log.chunks) >= 3 and [len(c) for c in once.track_log.chunks][:3] == [16, 32, 64]
    assert len(full_run.track_log.chunks) == 1
    want = full_run.all_tracks
    final = once.all_tracks
    assert once.track_log.copies == 1 and every.track_log.copies == len(every.records)
    assert once.all_tracks is final                                    # cached until the next frame is stored
    for got in (final, every.all_tracks, every.reads[-1]):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a[0] == b[0] and a[1] == b[1] and not a[2].is_cuda and torch.equal(a[2], b[2])
    n = 0
    for rec, read in zip(every.records, every.reads):                  # what was read during the run is a prefix
        n += len(rec["ids"])
        assert len(read) == n and all(torch.equal(a[2], b[2]) for a, b in zip(read, want))


def test_crop_frame_without_a_crop_detector(dev):
    trk = _tracker(dev)
    trk.crop_detector = None
    with pytest.raises(RuntimeError, match="cd"):
        trk.track()
    assert trk.frame_num == 1


def test_frames4k_loader(dev):
    import timestamp_utilities as tsu
    from mc3d_tracker import Frames4K
    from retinanet_mi355x import ops
    geom = fc.geometry(4, 7, 13, x0=5, y0=1)
    tab = fc.table(geom)
    digits = fc.random_digits(2, 12, seed=43)
    frames = np.stack([fc.render(fc.stamp_text(d, 13), geom, 8, 64) for d in digits])
    frames[1, 1:8, 5 + 12:5 + 16] = 255                                # camera 2's stamp is unreadable
    loaders = [Frames4K("/data/p1c%d_0.mp4" % (c + 1), [torch.from_numpy(frames[c])], tsu.TimestampReader([(geom, tab)], 1, device=dev))
               for c in range(2)]
    for c, loader in enumerate(loaders):
        assert len(loader) == 1 and loader.sequence.endswith("p1c%d_0.mp4" % (c + 1))
        frame_num, frame, original, stamp = next(loader)
        want, t, s = ops.load_frames_4k(torch.from_numpy(frames[c:c + 1]).to(dev), tsu.TimestampReader([(geom, tab)], 1, device=dev))
        assert frame_num == 0 and original is None
        assert frame.is_cuda and frame.dtype == torch.float32 and tuple(frame.shape) == (3, 4, 32) and torch.equal(frame, want[0])
        if c == 0:
            assert int(s[0]) == fc.READ and stamp == float(t[0]) == float(fc.stamp_text(digits[0], 13))
        else:
            assert int(s[0]) != fc.READ and stamp is None
        assert next(loader) == (-1, None, None, None)

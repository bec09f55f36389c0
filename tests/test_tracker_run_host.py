"""CPU: the tracker's frame loop restated in tests/tracker_cases.py against the reference's own ``track()`` run
(tests/golden/tracker_run.npz, tools/make_golden_tracker.py); the argmin rule of ops.track_crop_prior; and what
``mc3d_tracker.MC_Crop_Tracker`` refuses at construction, before any GPU work."""
import numpy as np
import pytest
import torch

import track_cases as tc
import tracker_cases as trc


@pytest.fixture(scope="module")
def host_run():
    return trc.run_host()


def test_fixture_keeps_its_margins(golden):
    """The golden tool refuses to write a fixture with a decision closer than MARGIN to its runner-up; the margins it
    measured travel with the file."""
    g = golden("tracker_run")
    kinds = [k for k in g.files if k.startswith("margin_")]
    assert len(kinds) == 7
    for k in kinds:
        assert float(g[k]) >= trc.MARGIN, (k, float(g[k]))
    assert int(g["n_frames"]) == 14 and int(g["cutoff_frames"]) == trc.EARLY_CUTOFF + 1


def test_restatement_reproduces_the_reference_run(golden, host_run):
    g = golden("tracker_run")
    trk, recs = host_run
    assert len(recs) == int(g["n_frames"])
    worst = {"X": 0.0, "P": 0.0, "stored": 0.0, "ts_bias": 0.0, "T": 0.0}
    for f, rec in enumerate(recs):
        for k in trc.DISCRETE_KEYS:
            assert np.array_equal(np.asarray(rec[k]), g["f%d_%s" % (f, k)]), (f, k)
        for k in ("X", "P", "stored"):                            # fp32 round-off: the restatement and the reference run the
            want = g["f%d_%s" % (f, k)]                          # same torch algebra up to the order of a few sums
            assert rec[k].shape == want.shape, (f, k)
            if want.size:
                e = float(np.abs(rec[k] - want).max() / max(1.0, np.abs(want).max()))
                worst[k] = max(worst[k], e)
                assert e <= 1e-5, (f, k, e)
        if len(rec["T"]):
            worst["T"] = max(worst["T"], float(np.abs(rec["T"] - g["f%d_T" % f]).max()))
        worst["ts_bias"] = max(worst["ts_bias"], float(np.abs(rec["ts_bias"] - g["f%d_ts_bias" % f]).max()))
    print("worst differences:", worst)
    assert worst["T"] <= 1e-9 and worst["ts_bias"] <= 1e-7
    assert trk.all_times == g["all_times"].tolist()
    assert [t[0] for t in trk.all_tracks] == g["csv_id"].tolist() and [t[1] for t in trk.all_tracks] == g["csv_time"].tolist()


def test_early_cutoff_is_a_prefix(golden, host_run):
    g = golden("tracker_run")
    _, full = host_run
    _, short = trc.run_host(early_cutoff=trc.EARLY_CUTOFF)
    assert len(short) == int(g["cutoff_frames"])
    for a, b in zip(short, full):
        for k in trc.FRAME_KEYS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_scene_exercises_the_time_sync(host_run):
    """Camera 2 skips a frame of its loader, camera 1 has one unreadable stamp: after the sync the cameras are within 20 ms."""
    _, recs = host_run
    st = trc.stamps()
    assert st[1][7] is None and st[2][trc.LAG_FRAME] - st[0][trc.LAG_FRAME] < -0.02
    for rec in recs:
        assert max(rec["timestamps"]) - min(rec["timestamps"]) < 0.02
    assert recs[trc.LAG_FRAME]["timestamps"][2] == st[2][trc.LAG_FRAME + 1]
    assert recs[7]["timestamps"][1] == recs[6]["timestamps"][1] + 1 / 30.0


def test_argmin_rule_on_hand_made_rows():
    """ops.track_crop_prior's camera pick is torch.argmin's rule on the CPU: an exact tie goes to the lower index, the
    first NaN wins.  Both restatements agree on rows made by hand."""
    nan, inf = float("nan"), float("inf")
    rows = [[3.0, 1.0, 1.0, 5.0], [2.0, 2.0], [nan, 1.0], [2.0, nan, nan, 0.0], [inf, inf, 7.0], [0.0, -0.0], [5.0, 4.0, nan]]
    want = [1, 0, 0, 1, 2, 0, 2]
    for row, w in zip(rows, want):
        assert trc.first_min_nan_wins(row) == w, row
        assert int(torch.argmin(torch.tensor(row))) == w, row
    # through the restatement of the crop frame: track 0 half way between two centres, track 1 with a NaN position
    centers = torch.tensor([[100, 50], [300, 50], [200, 950]])
    pre = torch.tensor([[200.0, 50.0], [nan, 10.0], [290.0, 60.0]])
    cam, dt = trc.crop_prior_restated(pre, centers, [10.0, 20.0, 30.0], [0.5, 0.25, 0.125], torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64))
    assert cam.tolist() == [0, 0, 1] and dt.tolist() == [9.5, 8.5, 17.25]


def _args():
    det, cd = trc.StandInDetector(), trc.StandInCropDetector()
    loaders = [trc.ScriptedLoader(c) for c in range(3)]

    class HG:
        correspondence = {c: {} for c in trc.CAMERAS}
    params = dict(trc.PARAMS, cam_centers=dict(trc.CAM_CENTERS), ts=trc.ts_table())
    return loaders, det, tc.kf_init(), HG(), tc.class_dict(), params, cd


def test_constructor_refusals():
    """All of these raise before any GPU work: the module imports and refuses on a machine without a GPU."""
    from mc3d_tracker import MC_Crop_Tracker
    loaders, det, kf, hg, cd_, params, cd = _args()
    with pytest.raises(NotImplementedError, match="PLOT=False"):
        MC_Crop_Tracker(loaders, det, kf, hg, cd_, params=params, cd=cd)                     # PLOT defaults to True
    with pytest.raises(NotImplementedError, match="PLOT=False"):
        MC_Crop_Tracker(loaders, det, kf, hg, cd_, params=params, cd=cd, PLOT=False, OUT="/tmp/frames")
    with pytest.raises(NotImplementedError, match="loader"):
        MC_Crop_Tracker(["/data/p1c1_0.mp4"], det, kf, hg, cd_, params=params, cd=cd, PLOT=False)
    no_centres = {k: v for k, v in params.items() if k != "cam_centers"}
    with pytest.raises(ValueError, match="cam_centers"):
        MC_Crop_Tracker(loaders, det, kf, hg, cd_, params=no_centres, cd=cd, PLOT=False)
    hg.correspondence = {c: {} for c in trc.CAMERAS[:2]}
    with pytest.raises(KeyError, match=trc.CAMERAS[2]):
        MC_Crop_Tracker(loaders, det, kf, hg, cd_, params=params, cd=cd, PLOT=False)


def test_new_entry_point_is_bound_and_registered():
    from retinanet_mi355x import _hip, ops, torch_ops
    assert "rn_track_crop_prior" in _hip.SIGNATURES and len(_hip.SIGNATURES["rn_track_crop_prior"][1]) == 13
    assert "track_crop_prior" in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, "track_crop_prior")
    case = trc.crop_prior_case(4, 2, seed=1)
    cpu = [torch.from_numpy(case[k]) for k in ("X", "D", "T")] + [torch.eye(6)] + \
          [torch.from_numpy(case[k]) for k in ("centers", "stamps", "bias")]
    with pytest.raises(RuntimeError):
        ops.track_crop_prior(*cpu)
    lib = _hip.load()                                            # host-side argument checks of the C entry point
    assert lib.rn_track_crop_prior(None, None, None, None, None, None, None, 3, None, None, None, 0, None) == 0
    assert lib.rn_track_crop_prior(None, None, None, None, None, None, None, 0, None, None, None, 5, None) == 1   # hipErrorInvalidValue

"""CPU: the numpy restatement of estimate_ts_bias (tests/ts_bias_cases.py, the GPU tests' fuzz oracle) against the
reference's own outputs in tests/golden/ts_bias.npz, the C ABI's argument lists, and the refusal of CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ts_bias_cases as tb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(r, g, key, ts_start):
    assert np.array_equal(r["entries"], g[key + "entries"]), key
    assert r["time_error"].dtype == np.float32 and np.array_equal(r["time_error"], g[key + "time_error"]), key
    assert np.array_equal(np.array(r["ts_bias"], np.float64), g[key + "ts_bias"]), (key, r["ts_bias"], g[key + "ts_bias"])
    if len(r["entries"]) == 0:
        assert r["ts_bias"] == [float(b) for b in ts_start], key


def test_restatement_reproduces_every_golden_case(golden):
    """Entry lists equal; time_error and ts_bias bit for bit.  The mean speeds are re-derived where they are free of the
    summation order (every scripted case: <= 2 tracks per direction or the fallback) and must equal the golden's."""
    g = golden("ts_bias")
    for name, c in tb.cases().items():
        r = tb.restated(c["boxes"], c["cams"], c["objs"], c["timestamps"], c["ts_bias"], c["phi"])
        if r["vel"] is not None:
            assert np.array_equal(np.array(r["vel"], np.float32), g[name + "_vel"]), name
        _same(r, g, name + "_", c["ts_bias"])
    assert len(g["overlap3_entries"]) >= 12 and len(g["same_camera_entries"]) == 0
    assert len(g["threshold_entries"]) == 2 and len(g["threshold_equal_entries"]) == 0


def test_restatement_reproduces_the_sequence(golden):
    """The filter holds more than two tracks of a direction: the two mean speeds come from the golden, everything else
    is re-derived, the biases carried from frame to frame."""
    g = golden("ts_bias")
    bias = list(tb.SEQ_TS_BIAS)
    moved = 0
    for f, fr in enumerate(tb.sequence()):
        key = "seq%d_" % f
        objs = np.zeros((1, 7), np.float32) if f else np.zeros((0, 7), np.float32)     # only "any track at all" matters here
        r = tb.restated(fr["detections"], fr["cameras"], objs, fr["timestamps"], bias, tb.PHI, vel=tuple(g[key + "vel"]))
        _same(r, g, key, bias)
        moved += r["ts_bias"] != bias
        bias = r["ts_bias"]
    assert moved >= 6


def test_restatement_on_the_parser_states(golden):
    """parse_est_ts: the golden holds the parser's outputs after the space NMS, not the states estimate_ts_bias saw, so
    the restatement runs on the CPU oracle's states (equal to the reference's to 1e-5 / 1e-4): the entries must be the
    reference's exactly, every time_error and every camera's bias within what that state tolerance allows
    (ts_bias_cases.parse_bias_bound: per entry and per camera, two orders below the change of the biases)."""
    import golden_cases as gc
    from oracle import tracker_post as otp
    g = golden("ts_bias")
    scores, labels, boxes, cams, names, (P, H), (P2, H2) = gc.tracker_post_inputs()
    st, _, _, cm = otp.parse_detections(scores, labels, boxes, cams, H, H2, P, P2, perform_nms=False, refine_height=True)
    keep = scores > 0.1
    idx = otp.im_nms(boxes[keep].reshape(-1, 10, 2)[:, :8, :], scores[keep], threshold=0.3, groups=cams[keep])
    st, cm = st[idx].numpy(), cm[idx].numpy()
    objs, ts, bias = tb.parse_scene()
    r = tb.restated(st, cm, objs, ts, bias, tb.PHI)
    assert np.array_equal(r["entries"], g["parse_est_ts_entries"])
    assert np.array_equal(np.array(r["vel"], np.float32), g["parse_est_ts_vel"])
    bound, te_bound = tb.parse_bias_bound(st, r, len(bias))
    assert (np.abs(r["time_error"].astype(np.float64) - g["parse_est_ts_time_error"]) <= te_bound).all()
    diff = np.abs(np.array(r["ts_bias"]) - g["parse_est_ts_ts_bias"])
    assert (diff <= bound).all(), (diff, bound)
    moved = np.abs(g["parse_est_ts_ts_bias"] - np.array(bias))
    assert bound.max() <= 0.02 * moved.max() and (moved > 10 * bound).sum() >= 10      # the bound is far below the effect


def _header_args(name):
    src = open(os.path.join(REPO, "include", "retinanet_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    out = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        if "*" in a:
            out.append(ctypes.c_void_p)
        else:
            out.append({"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double,
                        "float": ctypes.c_float}[a.rsplit(" ", 1)[0].replace("const ", "")])
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[m.group(1)], out


def test_signatures_name_the_new_entry_points():
    from retinanet_mi355x import _hip
    for name in ("rn_ts_bias_workspace_bytes", "rn_estimate_ts_bias"):
        assert name in _hip.SIGNATURES
        res, args = _hip.SIGNATURES[name]
        assert (res, list(args)) == _header_args(name), name
    lib = _hip.load()
    assert lib.rn_ts_bias_workspace_bytes(0, 16) == 0
    assert lib.rn_ts_bias_workspace_bytes(100, 256) >= 100 * 24 + 256 * 16


def test_new_op_refuses_cpu_tensors_and_is_registered():
    from retinanet_mi355x import ops, torch_ops
    c = tb.cases()["cam0_only"]
    args = (torch.from_numpy(c["boxes"]), torch.from_numpy(c["cams"]), torch.from_numpy(c["objs"]),
            torch.tensor(c["timestamps"], dtype=torch.float64), torch.tensor(c["ts_bias"], dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.estimate_ts_bias(*args, tb.PHI, tb.ALPHA, tb.MU_V)
    assert "estimate_ts_bias" in torch_ops.OPERATORS
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.retinanet_mi355x.estimate_ts_bias(*args, tb.PHI, tb.ALPHA, tb.MU_V, 64)
    import mc3d_track
    assert mc3d_track.TrackManager.estimate_ts_bias is mc3d_track.estimate_ts_bias


def test_scripted_cases_have_their_properties():
    """What each case is named after, read off the restatement (the generator checks the same on the reference)."""
    cs = tb.cases()
    r = {n: tb.restated(c["boxes"], c["cams"], c["objs"], c["timestamps"], c["ts_bias"], c["phi"]) for n, c in cs.items()}
    e = r["overlap3"]["entries"]
    written, dependent = set(), False
    for c1, c2, _, _ in e:
        dependent |= c1 != 0 and c2 in written
        written |= {int(c1)} - {0}
    assert len(e) >= 12 and dependent
    assert all(0 in (c1, c2) for c1, c2, _, _ in r["cam0_only"]["entries"])
    assert r["one_direction"]["vel"][1] == -tb.MU_V
    assert len(r["same_camera"]["entries"]) == 0 and len(tb.pair_list(cs["same_camera"]["boxes"], np.arange(10), tb.PHI)) >= 5
    iou = tb.iou_matrix(tb.footprints(cs["threshold"]["boxes"]))
    assert iou[0, 1] > tb.PHI > iou[2, 3] and iou[0, 1] - iou[2, 3] < 1e-5
    n_fuzz = sum(len(tb.restated(**tb.fuzz_scene(t))["entries"]) > 0 for t in range(40))
    assert n_fuzz >= 20

"""CPU: the numpy restatement of the filter fit (tests/fit_filter_cases.py) against tests/golden/fit_filter.npz, which
tools/make_golden.py makes by running fit_filter_3D.py's cells around the reference's own Homography_Wrapper and Torch_KF.

Chosen rows are exact; states, predictions, targets, per-iteration errors, residuals and speeds come from the same fp32
(or fp64-then-rounded) operations and are bit-equal.  Means and covariances: the script sums serially in fp32, the
restatement (as the kernel) in fp64 with one rounding.  Largest deviation measured here, as |difference| / the array's
largest magnitude: 2.5e-7 (Q, 100 rows; class covariances 1.9e-7; class sizes 1.4e-7; var_v 7.9e-8; R 7.2e-8; mu_R
6.3e-8; mu_Q and mu_v equal).  fit_filter_cases.MOMENT_BOUND is 4x that largest value; the GPU tests use the same bound.

The header also declares the two new C-ABI entries and the binding knows them (the library itself is checked by
tests/test_cabi_exports.py, which compares every declared symbol)."""
import os
import re

import numpy as np

import fit_filter_cases as fc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_fit_entries():
    src = open(os.path.join(REPO, "include", "retinanet_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(rn_[a-z0-9_]+)\s*\(", src))
    from retinanet_mi355x import _hip
    for n in ("rn_fit_nearest", "rn_residual_moments"):
        assert n in names and n in _hip.SIGNATURES, n
    assert len(_hip.SIGNATURES["rn_fit_nearest"][1]) == 9 and len(_hip.SIGNATURES["rn_residual_moments"][1]) == 9
    import ctypes
    if os.path.exists(_hip.LIB_PATH):
        lib = ctypes.CDLL(_hip.LIB_PATH)
        assert hasattr(lib, "rn_fit_nearest") and hasattr(lib, "rn_residual_moments")


def test_states_and_q_rows_are_bit_equal(golden):
    z = golden("fit_filter")
    tr, cls, cam = fc.tracklets()
    n = len(tr)
    st = fc.gt_states(tr.reshape(-1, 8, 2), np.repeat(cls, 3), np.repeat(cam, 3)).reshape(n, 3, 6)
    assert np.array_equal(st, z["q_states"])
    err, pred, tgt = fc.q_errors(st)
    assert np.array_equal(pred, z["q_pred"]) and np.array_equal(tgt, z["q_target"]) and np.array_equal(err, z["q_errors"])
    assert np.array_equal(fc.speeds(st[:, 0], st[:, 2], 3)[:, None], z["speeds"])


def test_r_rows_and_residuals_are_exact(golden):
    z = golden("fit_filter")
    gt_im, gt_cls, cam, scores, labels, boxes20, off = fc.detector_frames()
    gs = fc.gt_states(gt_im[:, 0], gt_cls, cam)
    ds = fc.gt_states(boxes20[:, :16].reshape(-1, 8, 2), labels, np.repeat(cam, fc.FRAME_D))
    assert np.array_equal(gs, z["r_gt_states"]) and np.array_equal(ds, z["r_det_states"])
    rows, resid, counts = fc.nearest(gs, ds, off)
    assert np.array_equal(rows, z["r_rows"]) and np.array_equal(resid, z["r_errors"])
    assert counts == (len(z["r_errors"]), fc.FRAME_D.count(0), 0)


def test_nearest_cases(golden):
    z = golden("fit_filter")
    for name, (gt, det, off) in fc.nearest_cases().items():
        rows, resid, counts = fc.nearest(gt, det, off)
        assert np.array_equal(rows, z["nearest_%s_rows" % name]), name
        assert np.array_equal(resid, z["nearest_%s_resid" % name]), name
    assert fc.nearest(*fc.nearest_cases()["nan"])[2] == (2, 1, 1)


def test_moments_of_the_golden(golden):
    z = golden("fit_filter")
    _, cls, _ = fc.tracklets()
    devs = {}
    for tag, rows, mean, cov in (("Q", z["q_errors"], z["mu_Q"], z["Q"]), ("R", z["r_errors"], z["mu_R"], z["R"]),
                                 ("v", z["speeds"], z["mu_v"], z["var_v"])):
        m, c, n = fc.moments(rows)
        assert n[0] == len(rows)
        devs["mu_" + tag], devs["cov_" + tag] = fc.moment_dev(m, mean), fc.moment_dev(c, cov)
    m, c, n = fc.moments(z["q_states"].reshape(-1, 6)[:, 2:5], np.repeat(cls, 3), 8)
    devs["class_size"] = max(fc.moment_dev(m[g], z["class_size"][g]) for g in range(8))
    devs["class_cov"] = max(fc.moment_dev(c[g], z["class_covariance"][g]) for g in range(8))
    print("fp64-accumulated restatement against the reference's serial fp32 sums:", devs)
    assert max(devs.values()) <= fc.MOMENT_BOUND, devs
    P = np.zeros((6, 6), np.float32)
    P[:5, :5] = z["R"]
    P[5, 5] = z["var_v"][0, 0]
    assert np.array_equal(P, z["P"])


def test_moments_restatement_edges():
    m, c, n = fc.moments(np.array([[3.0, -2.0]], np.float32))
    assert n[0] == 1 and np.array_equal(m, [3.0, -2.0]) and not c.any()
    E, grp, G = fc.moments_cases()["groups"]
    m, c, n = fc.moments(E, grp, G)
    assert n[2] == 0 and n[5] == 0 and n[3] == 1 and not c[3].any() and not m[2].any() and n.sum() == len(E)

"""GPU: fitting the Kalman filter's covariances (csrc/fit_filter.hip, fit_filter.py) against tests/golden/fit_filter.npz
(fit_filter_3D.py's cells run around the reference's own Homography_Wrapper and Torch_KF) and the numpy restatement of
tests/fit_filter_cases.py.

residual_moments: equal to the fp64 restatement rounded to fp32 within 1 fp32 ulp (the kernel's and numpy's fp64 sums
run in different orders: ~1e-16 relative, which can move the one rounding to fp32 by a unit), bit-identical between runs.
fit_nearest: rows, residuals and counts exact.  The drop-in functions on the golden's inputs: states, predictions and
targets to the homography / filter tolerances of test_gpu_ops.py and test_gpu_kf.py (rtol 1e-6, atol 1e-5), moments to
fit_filter_cases.MOMENT_BOUND (measured on the CPU, see tests/test_fit_filter.py)."""
import pickle

import numpy as np
import pytest
import torch

import fit_filter_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from retinanet_mi355x import ops, torch_ops       # noqa: F401  (registers torch.ops.retinanet_mi355x.*)
    return ops


@pytest.fixture(scope="module")
def hg():
    import homography
    names, (Ps, Hs), (Ps2, Hs2) = fc.cameras()

    def make(P, H):
        h = homography.Homography()
        h.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        h.default_correspondence = names[0]
        return h
    return homography.Homography_Wrapper(hg1=make(Ps, Hs), hg2=make(Ps2, Hs2)), names


def n(t):
    return t.detach().cpu().numpy()


def ulps32(a, b):
    """Largest distance in units of the last place between two fp32 arrays of finite values."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


CASES = fc.moments_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_residual_moments(ops, dev, name):
    E, grp, G = CASES[name]
    e = torch.from_numpy(E).to(dev)
    g = None if grp is None else torch.from_numpy(grp).to(dev)
    got = ops.residual_moments(e, g, G if grp is not None else None)
    want = fc.moments(E, grp, G)
    assert np.array_equal(n(got[2]), want[2])
    assert ulps32(n(got[0]), want[0]) <= 1 and ulps32(n(got[1]), want[1]) <= 1, (ulps32(n(got[0]), want[0]), ulps32(n(got[1]), want[1]))
    again = ops.residual_moments(e, g, G if grp is not None else None)
    for a, b in zip(got, again):
        assert np.array_equal(n(a).view(np.int32), n(b).view(np.int32))
    cov = n(got[1])
    assert np.array_equal(cov, np.swapaxes(cov, -1, -2))
    if len(E) == 1:
        assert not cov.any() and np.array_equal(n(got[0]), E[0])
    if name == "offset":                                           # uncentred sums would lose the variance below 1e4^2
        assert np.all(np.abs(np.diag(cov) - 1.0) < 0.3)
    if name == "groups":
        cnt = n(got[2])
        assert cnt[2] == 0 and cnt[5] == 0 and cnt[3] == 1 and not n(got[0])[2].any() and not cov[2].any() and not cov[3].any()


def test_residual_moments_operator_and_empty(ops, dev):
    E, grp, G = CASES["groups"]
    e, g = torch.from_numpy(E).to(dev), torch.from_numpy(grp).to(dev)
    m, c, k = torch.ops.retinanet_mi355x.residual_moments(e, g, G)
    want = ops.residual_moments(e, g, G)
    assert all(np.array_equal(n(a), n(b)) for a, b in zip((m, c, k), want))
    m1, c1, k1 = torch.ops.retinanet_mi355x.residual_moments(e, None, 1)
    assert tuple(m1.shape) == (1, 3) and tuple(c1.shape) == (1, 3, 3) and int(k1[0]) == len(E)
    m0, c0, k0 = ops.residual_moments(e[:0])
    assert int(k0[0]) == 0 and not n(m0).any() and not n(c0).any()
    with pytest.raises(RuntimeError):
        ops.residual_moments(torch.zeros(4, 9, device=dev))
    with pytest.raises(RuntimeError):
        ops.residual_moments(torch.zeros(4, 3))


def naive_argmin(dists):
    """What a reduction without the script's rules does: a later equal distance replaces the earlier one, and a NaN
    is never rejected (``not (d > best)`` is true for it)."""
    r = 0
    for j in range(len(dists)):
        if not (dists[j] > dists[r]):
            r = j
    return r


@pytest.mark.parametrize("name", ["sizes", "ties", "nan"])
def test_fit_nearest(ops, dev, golden, name):
    z = golden("fit_filter")
    gt, det, off = fc.nearest_cases()[name]
    rows, resid, info = ops.fit_nearest(torch.from_numpy(gt).to(dev), torch.from_numpy(det).to(dev), torch.from_numpy(off).to(dev))
    w_rows, w_resid, w_counts = fc.nearest(gt, det, off)
    assert np.array_equal(w_rows, z["nearest_%s_rows" % name]) and np.array_equal(w_resid, z["nearest_%s_resid" % name])
    assert np.array_equal(n(rows), w_rows), (n(rows), w_rows)
    assert tuple(n(info)) == w_counts
    k = int(info[0])
    assert np.array_equal(n(resid)[:k].view(np.int32), w_resid.view(np.int32)) and not n(resid)[k:].any()
    if name in ("ties", "nan"):                                    # the cases catch a reduction without the two rules
        assert not np.array_equal(fc.nearest(gt, det, off, pick=naive_argmin)[0], w_rows)
    if name == "nan":
        assert list(n(rows)) == [1, -1, 4, -1] and tuple(n(info)) == (2, 1, 1)
    if name == "ties":
        assert list(n(rows)) == [0, 73, 141]


@pytest.mark.parametrize("last", [2, 0])
def test_fit_nearest_compaction_carries_across_a_chunk_of_frames(ops, dev, last):
    """fit_compact_kernel takes the frames 1024 at a time: 1025 frames of 0 .. 2 detections.  Frames without a match (empty,
    or NaN distances only) lie all over the first chunk, frame 1023 among them; frame 1024, alone in the second chunk, has a
    match (its residual's row is the carry) or is empty (the carry is the count)."""
    from retinanet_mi355x import synth
    B = 1025
    d_per = (np.arange(B) * 5 + 1) % 3
    d_per[[0, 1022, 1023, 1024]] = (1, 2, 0, last)
    off = np.concatenate(([0], np.cumsum(d_per))).astype(np.int64)
    gt = synth.vehicle_states(B, seed=541).numpy()
    gt[[6, 1020], 3] = 0                                           # zero area: NaN distances, no match
    frame = np.repeat(np.arange(B), d_per)
    det = gt[frame].copy()
    det[:, 0] += synth.uniform((len(det),), 542, -20, 20)
    det[:, 1] += synth.uniform((len(det),), 543, -3, 3)
    assert d_per[6] and d_per[1020]
    w_rows, w_resid, w_counts = fc.nearest(gt, det, off)
    assert w_counts[1] == int((d_per == 0).sum()) > 300 and w_counts[2] == 2 and (w_rows[1024] >= 0) == (last > 0)
    rows, resid, info = ops.fit_nearest(torch.from_numpy(gt).to(dev), torch.from_numpy(det).to(dev), torch.from_numpy(off).to(dev))
    assert np.array_equal(n(rows), w_rows) and tuple(n(info)) == w_counts
    k = int(info[0])
    assert np.array_equal(n(resid)[:k].view(np.int32), w_resid.view(np.int32)) and not n(resid)[k:].any()


def test_fit_nearest_operator_and_edges(ops, dev):
    gt, det, off = fc.nearest_cases()["sizes"]
    g, d, o = torch.from_numpy(gt).to(dev), torch.from_numpy(det).to(dev), torch.from_numpy(off).to(dev)
    rows, resid, info = torch.ops.retinanet_mi355x.fit_nearest(g, d, o)
    want = ops.fit_nearest(g, d, o)
    assert all(np.array_equal(n(a), n(b)) for a, b in zip((rows, resid, info), want))
    rows, resid, info = ops.fit_nearest(g[:2], d[:0], torch.zeros(3, dtype=torch.int64, device=dev))   # no detection at all
    assert list(n(rows)) == [-1, -1] and tuple(n(info)) == (0, 2, 0)
    bad = torch.tensor([0, 5, 10 ** 6], device=dev)                # offsets beyond det are clamped, nothing outside is read
    rows, resid, info = ops.fit_nearest(g[:2], d[:7], bad)
    assert int(rows.max()) < 7 and int(info.sum()) == 2
    with pytest.raises(RuntimeError):
        ops.fit_nearest(g, d, o[:-1])


def close(a, b, rtol=1e-6, atol=1e-5):
    a = n(a) if isinstance(a, torch.Tensor) else a
    assert a.shape == b.shape and np.allclose(a, b, rtol=rtol, atol=atol), float(np.abs(a - b).max())


def close_fitted(a, b, rtol):
    """For the state of a filter built from fitted parameters: they may differ from the golden's by MOMENT_BOUND of
    their array's largest entry, and X / P carry them (P0 is the fitted P itself), so that much of the expected array's
    largest entry is allowed on top of the filter tests' tolerance."""
    close(a, b, rtol, 1e-5 + 2 * fc.MOMENT_BOUND * float(np.abs(b).max()))


def test_gt_states_and_fit_Q(dev, golden, hg):
    import fit_filter
    z = golden("fit_filter")
    wr, names = hg
    tr, cls, cam = fc.tracklets()
    cams = [names[c] for c in cam]
    st = fit_filter.gt_states(wr, torch.from_numpy(tr[:, 0]).to(dev), [fc.CLASS_NAMES[c] for c in cls], cams)
    close(st, z["q_states"][:, 0])
    st3 = fit_filter.tracklet_states(wr, torch.from_numpy(tr).to(dev), torch.from_numpy(cls), (names, torch.from_numpy(cam)))
    close(st3, z["q_states"])
    err, pred, tgt = fit_filter.q_errors(wr, fc.kf_params(), torch.from_numpy(tr).to(dev), cls, cams)
    close(pred, z["q_pred"]), close(tgt, z["q_target"])
    close(err, z["q_errors"], atol=2e-5 + 2e-6 * float(np.abs(z["q_pred"]).max()))      # a difference of two such rows
    mu_Q, Q = fit_filter.fit_Q(wr, fc.kf_params(), torch.from_numpy(tr).to(dev), cls, cams)
    assert mu_Q.is_cuda and tuple(mu_Q.shape) == (6,) and tuple(Q.shape) == (6, 6) and Q.dtype == torch.float32
    dm, dq = fc.moment_dev(n(mu_Q), z["mu_Q"]), fc.moment_dev(n(Q), z["Q"])
    print("mu_Q dev %.3e  Q dev %.3e  rows equal: %s" % (dm, dq, np.array_equal(n(err), z["q_errors"])))
    assert dm <= fc.MOMENT_BOUND and dq <= fc.MOMENT_BOUND, (dm, dq)


def _detections(dev):
    gt_im, gt_cls, cam, scores, labels, boxes20, off = fc.detector_frames()
    det = tuple(torch.from_numpy(a).to(dev) for a in (scores, labels, boxes20)) + (torch.from_numpy(off),)
    return torch.from_numpy(gt_im).to(dev), gt_cls, cam, det


def test_fit_R_precomputed(dev, golden, hg):
    import fit_filter
    z = golden("fit_filter")
    wr, names = hg
    gt_im, gt_cls, cam, det = _detections(dev)
    cams = [names[c] for c in cam]
    resid, rows, info, gs, ds = fit_filter.r_errors(wr, None, None, gt_im, gt_cls, cams, detections=det)
    close(gs, z["r_gt_states"]), close(ds, z["r_det_states"])
    assert np.array_equal(n(rows), z["r_rows"])
    assert tuple(n(info)) == (len(z["r_errors"]), fc.FRAME_D.count(0), 0)
    close(resid[:int(info[0])], z["r_errors"], atol=2e-5 + 2e-6 * float(np.abs(z["r_gt_states"]).max()))
    mu_R, R, empty, bad = fit_filter.fit_R(wr, None, None, gt_im, gt_cls, cams, detections=det)
    assert (empty, bad) == (fc.FRAME_D.count(0), 0) and tuple(mu_R.shape) == (5,) and tuple(R.shape) == (5, 5)
    dm, dr = fc.moment_dev(n(mu_R), z["mu_R"]), fc.moment_dev(n(R), z["R"])
    print("mu_R dev %.3e  R dev %.3e  rows equal: %s" % (dm, dr, np.array_equal(n(resid)[:int(info[0])], z["r_errors"])))
    assert dm <= fc.MOMENT_BOUND and dr <= fc.MOMENT_BOUND, (dm, dr)


def test_fit_R_runs_the_detector_per_frame(dev, golden, hg):
    """The detector path: a stand-in module that returns each frame's precomputed detections, called in eval mode."""
    import fit_filter
    z = golden("fit_filter")
    wr, names = hg
    gt_im, gt_cls, cam, (scores, labels, boxes20, off) = _detections(dev)

    class Stub(torch.nn.Module):
        calls = 0

        def forward(self, frame):
            assert not self.training and not torch.is_grad_enabled()
            b = int(frame[0])
            Stub.calls += 1
            lo, hi = int(off[b]), int(off[b + 1])
            return scores[lo:hi], labels[lo:hi], boxes20[lo:hi]
    frames = torch.arange(len(gt_im), device=dev).reshape(-1, 1)
    mu_R, R, empty, bad = fit_filter.fit_R(wr, Stub().train(), frames, gt_im, gt_cls, [names[c] for c in cam])
    assert Stub.calls == len(gt_im) and (empty, bad) == (fc.FRAME_D.count(0), 0)
    assert fc.moment_dev(n(mu_R), z["mu_R"]) <= fc.MOMENT_BOUND and fc.moment_dev(n(R), z["R"]) <= fc.MOMENT_BOUND


def test_fit_class_sizes_and_speed(dev, golden):
    import fit_filter
    z = golden("fit_filter")
    _, cls, _ = fc.tracklets()
    st = torch.from_numpy(z["q_states"]).to(dev)
    sizes, covs = fit_filter.fit_class_sizes(st.reshape(-1, 6), torch.from_numpy(np.repeat(cls, 3)))
    assert sorted(sizes) == sorted(fc.CLASS_NAMES)
    for g, name in enumerate(fc.CLASS_NAMES):
        assert tuple(sizes[name].shape) == (3,) and tuple(covs[name].shape) == (3, 3)
        assert fc.moment_dev(n(sizes[name]), z["class_size"][g]) <= fc.MOMENT_BOUND
        assert fc.moment_dev(n(covs[name]), z["class_covariance"][g]) <= fc.MOMENT_BOUND
    sizes, _ = fit_filter.fit_class_sizes(st[:4, 0], torch.tensor([1, 1, 4, 1]))       # only the classes that occur
    assert sorted(sizes) == ["midsize", "semi"]
    mu_v, var_v = fit_filter.fit_speed(st[:, 0], st[:, 2], 3)
    assert tuple(mu_v.shape) == (1,) and tuple(var_v.shape) == (1, 1)
    assert fc.moment_dev(n(mu_v), z["mu_v"]) <= fc.MOMENT_BOUND and fc.moment_dev(n(var_v), z["var_v"]) <= fc.MOMENT_BOUND


def test_fit_gives_a_dict_the_filter_takes(dev, golden, hg):
    import fit_filter
    from util_track.kf import Torch_KF
    z = golden("fit_filter")
    wr, names = hg
    tr, cls, cam = fc.tracklets()
    gt_im, gt_cls, fcam, det = _detections(dev)
    params, empty, bad = fit_filter.fit(wr, fc.kf_params(), torch.from_numpy(tr).to(dev), cls, [names[c] for c in cam], None, None,
                                        gt_im, gt_cls, [names[c] for c in fcam], detections=det)
    assert (empty, bad) == (fc.FRAME_D.count(0), 0)
    for key, shape in (("mu_Q", (6,)), ("Q", (6, 6)), ("mu_R", (5,)), ("R", (5, 5)), ("P", (6, 6)), ("mu_v", (1,)),
                       ("F", (6, 6)), ("H", (5, 6))):
        assert tuple(params[key].shape) == shape and params[key].dtype == torch.float32 and not params[key].is_cuda, key
    for key in ("mu_Q", "Q", "mu_R", "R", "mu_v", "P"):
        assert fc.moment_dev(n(params[key]), z[key]) <= fc.MOMENT_BOUND, key
    P = n(params["P"])
    assert np.array_equal(P[:5, :5], n(params["R"])) and not P[5, :5].any() and not P[:5, 5].any()
    assert fc.moment_dev(P[5:, 5:], z["var_v"]) <= fc.MOMENT_BOUND
    for g, name in enumerate(fc.CLASS_NAMES):
        assert fc.moment_dev(n(params["class_size"][name]), z["class_size"][g]) <= fc.MOMENT_BOUND
        assert fc.moment_dev(n(params["class_covariance"][name]), z["class_covariance"][g]) <= fc.MOMENT_BOUND
    params = pickle.loads(pickle.dumps(params))
    st, classes, meas = fc.filter_probe()
    kf = Torch_KF(dev, INIT=params)
    s = torch.from_numpy(st)
    kf.add(s[:, :5].clone(), list(range(len(s))), s[:, 5].clone(), torch.zeros(len(s), dtype=torch.float64), init_speed=True,
           classes=classes)
    close_fitted(kf.X, z["probe_X0"], 1e-6), close_fitted(kf.P, z["probe_P0"], 1e-6)
    kf.predict()
    close_fitted(kf.X, z["probe_X1"], 1e-6), close_fitted(kf.P, z["probe_P1"], 1e-5)
    kf.update(torch.from_numpy(meas), list(range(len(s))))
    close(kf.X, z["probe_X2"], 1e-4, 1e-4), close(kf.P, z["probe_P2"], 1e-4, 1e-4)

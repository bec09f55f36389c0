"""GPU: the calibration kernels (csrc/calibrate.hip) against their numpy restatement (tests/calib_cases.py) bit for bit,
against what the reference produced (tests/golden/calibration.npz), and the set-up interface of the drop-in end to end."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import calib_cases as cc
from test_calibration_host import ERR_DEV

pytestmark = pytest.mark.gpu

# Largest |H - H_true| / max |H_true| (both with H[2,2] = 1) of the numpy restatement on fit_case(n, H, 500 + n) for
# n = 4, 5, 12, 65, image -> road and road -> image, measured on the CPU: between 4.6e-17 and 9.52e-15 (n = 12, road ->
# image).  The kernel is held to 8 x the largest.  This says how well exact data is recovered, not how close to OpenCV.
FIT_DEV_MEASURED = 9.6e-15
FIT_FACTOR = 8


@pytest.fixture(scope="module")
def cal(golden):
    return golden("calibration")


@pytest.fixture(scope="module")
def vp_cases():
    """name -> (lines, restated result), computed once."""
    return {name: (cc.vp_lines(name), cc.vanishing_point(cc.vp_lines(name))) for name in cc.VP_ALL}


def _launch_vp(sets, dev):
    from retinanet_mi355x import ops
    offsets = np.cumsum([0] + [len(s) for s in sets]).astype(np.int64)
    out, trace, status = ops.vanishing_points(torch.from_numpy(np.concatenate(sets)).to(dev), torch.from_numpy(offsets).to(dev))
    return out.cpu().numpy(), trace.cpu().numpy(), status.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_vanishing_points_of_unequal_sets_in_one_launch(cal, vp_cases, dev):
    names = list(cc.VP_ALL)                                            # 2, 3, 8, 2 (31-point axis), 2 (empty), 3 (NaN), 65 lines
    out, trace, status = _launch_vp([vp_cases[n][0] for n in names], dev)
    for i, n in enumerate(names):
        want = vp_cases[n][1]
        assert status[i] == want["status"] == 0, n
        assert _same_bits(out[i, :2], want["point"]) and _same_bits(out[i, 2], want["best"]), n
        assert _same_bits(trace[i], want["trace"]), n
        if n in cc.VP_GOLDEN:
            assert _same_bits(out[i, :2], cal["vp_%s_point" % n]), n   # what the reference returned
    assert vp_cases["axis31"][1]["bounds"][0, 0, 2] == 31
    assert out[names.index("empty"), 2] == np.inf and np.isfinite(out[names.index("nan"), 2])
    again = _launch_vp([vp_cases[n][0] for n in names], dev)
    assert all(_same_bits(a, b) for a, b in zip((out, trace), again[:2]))


@pytest.mark.parametrize("name", ["n2", "n3", "n8", "n65", "axis31"])
def test_vanishing_point_of_one_set(vp_cases, dev, name):
    lines, want = vp_cases[name]
    out, trace, status = _launch_vp([lines], dev)
    assert status[0] == 0 and _same_bits(out[0, :2], want["point"]) and _same_bits(out[0, 2], want["best"])
    assert _same_bits(trace[0], want["trace"])


def test_find_vanishing_point_interface(cal, dev):
    import homography as hgmod
    vp = hgmod.find_vanishing_point([row for row in cal["vp_n3_lines"]], device=dev)
    assert isinstance(vp, list) and _same_bits(np.array(vp), cal["vp_n3_point"])
    five = np.concatenate((cal["vp_n8_lines"], np.full((8, 1), 2.0)), 1)     # rows of an axes file carry a fifth column
    vps = hgmod.find_vanishing_points([cal["vp_n2_lines"], five], device=dev)
    assert _same_bits(np.array(vps), np.stack((cal["vp_n2_point"], cal["vp_n8_point"])))
    with pytest.raises(ValueError):
        hgmod.find_vanishing_point([[0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 2.0, 2.0]], device=dev)   # x1 = 0: the start is not finite


def test_row_ranges_outside_the_inputs_are_refused_not_read(vp_cases, cal, dev):
    from retinanet_mi355x import ops
    lines = torch.from_numpy(vp_cases["n3"][0]).to(dev)
    for bad in ([0, 4], [-1, 2], [2, 1], [1 << 40, (1 << 40) + 2]):
        out, _, status = ops.vanishing_points(lines, torch.tensor(bad, dtype=torch.int64, device=dev))
        assert status.cpu().tolist() == [ops.VP_BAD_OFFSETS] and bool(torch.isnan(out[0, :2]).all())
    src = torch.zeros(4, 2, dtype=torch.float64, device=dev)
    for bad in ([0, 5], [-4, 0], [3, 1]):
        H, status = ops.fit_homography(src, src, torch.tensor(bad, dtype=torch.int64, device=dev))
        assert status.cpu().tolist() == [ops.FIT_BAD_OFFSETS] and bool(torch.isnan(H).all())


# ------------------------------------------------------------------------------------------------ reprojection error, scale_Z
@pytest.fixture(scope="module")
def sz_cases(cal):
    out = {}
    for d in cc.SZ_D:
        tag = "sz_d%d_" % d
        boxes, heights, H, P0 = (cal[tag + k] for k in ("boxes", "heights", "H", "P0"))
        out[d] = (boxes, heights, H, P0, cc.scale_z(boxes, heights, H, P0))
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("d", cc.SZ_D)
def test_reprojection_errors_and_scale_z_search(cal, sz_cases, dev, d):
    from retinanet_mi355x import ops
    boxes, heights, H, P0, want = sz_cases[d]
    tb, th, tH, tP = _t(boxes, dev), _t(heights, dev), _t(H, dev), _t(P0, dev)
    Cs = np.concatenate((want["trace"][0, :, 0], want["trace"][-1, :, 0], [1.0]))
    got = ops.hg_reproj_error(tb, th, tH, tP, _t(Cs, dev)).cpu().numpy()
    assert _same_bits(got, cc.reproj_errors(boxes, heights, H, P0, Cs))
    trace, out, info = ops.hg_scale_z(tb, th, tH, tP)
    trace, out, (iters, status) = trace.cpu().numpy(), out.cpu().numpy(), info.cpu().tolist()
    assert status == 0 and iters == want["iters"] == len(cal["sz_d%d_grids" % d]) - 1
    assert _same_bits(trace[:iters], want["trace"]) and not trace[iters:].any()
    assert _same_bits(out, [want["last_C"], want["best_C"], want["best_error"]])
    assert _same_bits(cc.scaled_P(P0, out[0]), cal["sz_d%d_P_final" % d])


def _hg(cal, d, dev):
    from homography import Homography
    hg = Homography(device=dev)
    H = cal["sz_d%d_H" % d]
    hg.correspondence = {"cam": {"H": H, "H_inv": np.linalg.inv(H), "P": cal["sz_d%d_P0" % d].copy()}}
    hg.default_correspondence = "cam"
    return hg


def _numbers(text):
    pat = r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?"
    return re.sub(pat, "#", text), [float(x) for x in re.findall(pat, text)]


def _same_text(got, want, tol):
    (gs, gn), (ws, wn) = _numbers(got), _numbers(want)
    assert gs == ws, (got, want)
    for a, b in zip(gn, wn):
        assert abs(a - b) <= tol * abs(b), (got, want)


@pytest.mark.parametrize("d", (3, 300))
def test_scale_Z_leaves_P_at_the_last_candidate_and_prints_like_the_reference(cal, sz_cases, dev, d):
    hg = _hg(cal, d, dev)
    boxes, heights = torch.from_numpy(cal["sz_d%d_boxes" % d]), torch.from_numpy(cal["sz_d%d_heights" % d])
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        err = hg.test_transformation(boxes, heights=heights)
    assert err.dtype == torch.float64 and err.dim() == 0 and not err.is_cuda
    _same_text(text.getvalue(), bytes(cal["sz_d%d_tt_text" % d]).decode(), ERR_DEV)
    assert abs(float(err) - float(cal["sz_d%d_tt_error" % d])) <= ERR_DEV * float(cal["sz_d%d_tt_error" % d])
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        assert hg.scale_Z(boxes, heights) is None
    want = sz_cases[d][4]
    _same_text(text.getvalue(), bytes(cal["sz_d%d_sz_text" % d]).decode(), ERR_DEV * want["trace"][:, :, 1].min() / want["best_error"])
    P = hg.correspondence["cam"]["P"]
    assert _same_bits(P, cal["sz_d%d_P_final" % d])
    assert _same_bits(P, cc.scaled_P(cal["sz_d%d_P0" % d], want["last_C"]))
    assert not _same_bits(P, cc.scaled_P(cal["sz_d%d_P0" % d], want["best_C"]))       # the last candidate, not the best
    with pytest.raises(ValueError):
        hg.scale_Z(boxes, heights, granularity=2.0, max_scale=10)     # first step (10 - 2) / 9 is not above 2
    assert _same_bits(hg.correspondence["cam"]["P"], P)


# ------------------------------------------------------------------------------------------------ homography fit
def _fit(pairs, dev, refine=True):
    from retinanet_mi355x import ops
    src = np.concatenate([p[0] for p in pairs])
    dst = np.concatenate([p[1] for p in pairs])
    offsets = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    H, status = ops.fit_homography(_t(src, dev), _t(dst, dev), _t(offsets, dev), refine)
    return H.cpu().numpy(), status.cpu().numpy()


def test_fit_recovers_a_known_camera_from_exact_points(cal, dev):
    H = cal["sz_d17_H"]
    Hi = np.linalg.inv(H)
    pairs, truth = [], []
    for n in cc.FIT_N:
        im, sp = cc.fit_case(n, H, 500 + n)
        pairs += [(im, sp), (sp, im)]
        truth += [H / H[2, 2], Hi / Hi[2, 2]]
    got, status = _fit(pairs, dev)                                     # unequal sizes, both directions, one launch
    assert not status.any()
    for k, (g, t) in enumerate(zip(got, truth)):
        dev_k = np.abs(g - t).max() / np.abs(t).max()
        print("n = %d %s: %.2e" % (len(pairs[k][0]), "road->image" if k & 1 else "image->road", dev_k))
        assert g[2, 2] == 1.0 and dev_k <= FIT_FACTOR * FIT_DEV_MEASURED


def test_fit_refinement_does_not_raise_the_transfer_error_of_noisy_points(cal, dev):
    H = cal["sz_d17_H"]
    pairs = []
    for n in (5, 12, 65):
        im, sp = cc.fit_case(n, H, 600 + n, noise=0.5)
        pairs += [(im, sp), (sp, im)]
    refined, s1 = _fit(pairs, dev)
    plain, s2 = _fit(pairs, dev, refine=False)
    assert not s1.any() and not s2.any()
    for (src, dst), Hr, Hp in zip(pairs, refined, plain):
        r, p = cc.transfer_rms(Hr, src, dst), cc.transfer_rms(Hp, src, dst)
        w = cc.transfer_rms(cc.fit_homography(src, dst)[0], src, dst)
        print("n = %d: refined %.6f DLT %.6f restated %.6f" % (len(src), r, p, w))
        assert r <= p and r <= FIT_FACTOR * w


def test_fit_reports_degenerate_input(cal, dev):
    from homography import Homography
    H = cal["sz_d17_H"]
    line = np.stack((np.arange(6.0) * 100, np.arange(6.0) * 50 + 3), 1)
    good = cc.fit_case(5, H, 505)
    got, status = _fit([(line, line * 2), (line[:3], line[:3] + 1), good], dev)
    assert list(status) == [cc.FIT_DEGENERATE, cc.FIT_FEW_POINTS, 0]
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and np.isfinite(got[2]).all()
    hg = Homography(device=dev)
    for pts in (line, line[:3]):
        with pytest.raises(ValueError):
            hg.add_correspondence(list(pts), list(pts * 2), [[0, 0], [0, 0], [1.0, 2.0]], name="x")
    assert hg.correspondence == {}


# ------------------------------------------------------------------------------------------------ end to end
def test_add_i24_camera_then_scale_Z_reproduces_the_boxes(cal, dev, tmp_path):
    """Two files in the reference's formats -> add_i24_camera -> scale_Z -> the transforms the tracker calls."""
    from homography import Homography
    H, P_true = cal["sz_d17_H"], None
    Hi = np.linalg.inv(H)
    # the true camera: the fixture's H and a vertical vanishing point; boxes are made with the P it implies at C_TRUE
    vp_z, C_TRUE = np.array([960.0, -3360.0]), 0.14
    P_true = np.zeros((3, 4))
    P_true[:, [0, 1, 3]] = Hi / Hi[2, 2]
    P_true[:, 2] = np.array([vp_z[0], vp_z[1], 1.0]) * 0.01 * C_TRUE
    road = np.array([[x, y] for x in (300.0, 500.0, 700.0) for y in (0.0, 30.0, 60.0)])
    p = np.concatenate((road, np.ones((len(road), 1))), 1) @ (Hi / Hi[2, 2]).T
    image = p[:, :2] / p[:, 2:3]
    point_file, axes_file = tmp_path / "cam_EB_im_lmcs_transform_points.csv", tmp_path / "cam_axes.csv"
    rows = ["im x,im y,road x,road y"] + [",".join(repr(float(v)) for v in (a, b, c, d)) for (a, b), (c, d) in zip(image, road)] + ["tail"] * 4
    point_file.write_text("\n".join(rows) + "\n")
    vps_true = [P_true[:2, 0] / P_true[2, 0], P_true[:2, 1] / P_true[2, 1], vp_z]
    with open(axes_file, "w") as f:
        for axis, vp in enumerate(vps_true):
            for ln in cc.converging_lines(4, vp, 700 + axis, noise=0.0):
                f.write(",".join(repr(float(v)) for v in ln) + ",%d\n" % axis)
    hg = Homography(device=dev)
    hg.add_i24_camera(str(point_file), str(axes_file), "cam")
    cor = hg.correspondence["cam"]
    assert hg.default_correspondence == "cam" and cor["corr_pts"].shape == (9, 2)
    assert np.abs(cor["H_inv"] - Hi / Hi[2, 2]).max() <= 1e-9 * np.abs(Hi / Hi[2, 2]).max()
    assert np.array_equal(cor["P"][:, [0, 1, 3]], cor["H_inv"]) and cor["P"][2, 2] == 0.01
    # the three vanishing points are the restated search's, bit for bit (how near they land to the true ones is the
    # reference's own business: its best distance is carried across levels and a finer grid need not contain the winner)
    axes = np.loadtxt(str(axes_file), delimiter=",")
    for axis in range(3):
        want = cc.vanishing_point(axes[axes[:, 4] == axis][:, :4])
        assert _same_bits(np.array(cor["vps"][axis]), want["point"])
    assert _same_bits(cor["P"][:, 2], np.array([cor["vps"][2][0], cor["vps"][2][1], 1]) * 0.01)
    from retinanet_mi355x import synth
    states = synth.vehicle_states(12, seed=77)
    states[:, 1] = torch.where(states[:, 1] > 60, states[:, 1] - 60, states[:, 1])
    true = Homography(device=dev)
    true.correspondence = {"cam": {"H": H / H[2, 2], "H_inv": Hi / Hi[2, 2], "P": P_true}}
    true.default_correspondence = "cam"
    boxes = true.state_to_im(states)
    heights = states[:, 4].clone()
    P0 = cor["P"].copy()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        before = hg.test_transformation(boxes, heights=heights, verbose=False)
        hg.scale_Z(boxes, heights, name="cam")
        measured = hg.test_transformation(boxes, heights=heights, verbose=False)
    assert text.getvalue().startswith("Best Error: ")
    want = cc.scale_z(boxes.numpy(), heights.numpy(), cor["H"], P0)
    P = hg.correspondence["cam"]["P"]
    assert _same_bits(P, cc.scaled_P(P0, want["last_C"]))
    top, bot = cc.reproj_error(boxes.numpy(), heights.numpy(), cor["H"], P)
    assert float(measured) == top + bot
    # the result feeds the transforms the tracker calls: they reproduce the boxes to the error test_transformation measured
    back = hg.state_to_im(hg.im_to_state(boxes, heights=heights))
    e = torch.sqrt(((boxes - back) ** 2).sum(2))
    again = float(e[:, 4:].mean() + e[:, :4].mean())
    print("reprojection error: %.4f px before scale_Z, %.4f px after, %.4f px through the transforms; C = %.6f (true %.2f)"
          % (float(before), float(measured), again, P[2, 2] / 0.01, C_TRUE))
    assert abs(again - float(measured)) <= 1e-9 * float(measured)
    # the search minimises this very error over scales that bracket the true one; the scale it started from is 7 x off
    assert float(measured) < float(before)
    # the same through the reference's driver: built from the files, Z fitted on the first frame of a label file with
    # guessed heights, pickled, and unpickled by the next call
    import homography as hgmod
    classes = ["sedan", "semi", "nonsense"] * 4
    with open(tmp_path / "rectified_cam_0_track_outputs_3D.csv", "w") as f:
        f.write("a header line\nFrame #,Timestamp\n")
        for b, c in zip(boxes.numpy(), classes):
            f.write(",".join(["0", "", "", c] + [""] * 7 + [repr(float(v)) for v in b.reshape(-1)]) + "\n")
        f.write(",".join(["0", "", "", "van"] + [""] * 24) + "\n")              # a row without a 3D box is skipped
    save = str(tmp_path / "hg.cpkl")
    with contextlib.redirect_stdout(io.StringIO()):
        built = hgmod.get_homographies(save_file=save, directory=str(tmp_path), direction="EB", data_dir=str(tmp_path),
                                       vp_dir=str(tmp_path), cameras=["cam"])
        by_hand = Homography(device=dev)
        by_hand.add_i24_camera(str(point_file), str(axes_file), "cam")
        by_hand.scale_Z(boxes, by_hand.guess_heights(classes), name="cam")
        loaded = hgmod.get_homographies(save_file=save)
    assert built.correspondence["cam"]["P"][2, 2] != 0.01 and sorted(loaded.correspondence) == ["cam"]
    for k in ("H", "H_inv", "P"):
        assert _same_bits(built.correspondence["cam"][k], by_hand.correspondence["cam"][k])
        assert _same_bits(loaded.correspondence["cam"][k], built.correspondence["cam"][k])

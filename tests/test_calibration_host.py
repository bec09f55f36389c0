"""CPU: camera calibration (homography.py:12-154, 239-271, 336-385, 554-666).  The numpy restatement of the four kernels
(tests/calib_cases.py) against what the reference itself produced (tests/golden/calibration.npz, written by
tools/make_golden.py's gen_calibration), and the host side of the drop-in's set-up interface."""
import contextlib
import io
import pickle

import numpy as np
import pytest
import torch

import calib_cases as cc

# Largest |restated error - reference's error| over all 100 evaluations of a scale_Z search, relative to that search's
# smallest error, measured on the committed fixture: d = 1: 6.7e-13, d = 3: 4.9e-13, d = 17: 3.3e-11, d = 65: 1.04e-9,
# d = 300: 8.1e-11 (the reference sums with torch's vectorised CPU reduction, the restatement in the kernels' fixed order;
# the coarse candidates have errors of 1e4 .. 1e5 pixels, the best a few pixels).  The constant is 4 x the largest: the
# margin is for torch builds whose CPU reduction takes another order.
ERR_DEV_MEASURED = 1.05e-9
ERR_DEV = 4 * ERR_DEV_MEASURED


@pytest.fixture(scope="module")
def cal(golden):
    return golden("calibration")


def test_arange_and_linspace_formulas_are_numpys():
    for p in (0.0, 123.456, -7e16, 3.3e17, cc.VP31_START, 1e40, -2392.25):
        g = 1e16
        while g > 1:
            got, (start, stop) = cc.arange_axis(p, g)
            want = np.arange(p - g * (31 // 2), p + g * (31 // 2), g)
            assert np.array_equal(got, want), (p, g)
            g = g / 10.0
        assert g == 1.0
    for lo, hi in ((1e-06, 10), (0.3 - 1.1111, 0.3 + 1.1111), (-0.5, 0.25), (2.0, 2.0), (1.2345678 - 3e-6, 1.2345678 + 3e-6)):
        assert np.array_equal(cc.linspace10(lo, hi), np.linspace(lo, hi, num=10)), (lo, hi)


def test_case_table_has_the_axis_lengths_it_claims():
    assert len(np.arange(cc.VP31_START - 1e16 * 15, cc.VP31_START + 1e16 * 15, 1e16)) == 31
    r = cc.vanishing_point(cc.vp_lines("axis31"))
    assert cc.vp_start(cc.vp_lines("axis31")) == (cc.VP31_START, 0.0)
    assert r["bounds"][0, 0, 2] == 31 and r["bounds"][0, 1, 2] == 30 and r["status"] == 0
    r = cc.vanishing_point(cc.vp_lines("empty"))
    assert (r["bounds"][:, 0, 2] == 0).all() and r["best"] == np.inf and tuple(r["point"]) == (1e40, 0.0)
    r = cc.vanishing_point(cc.vp_lines("nan"))
    assert np.isfinite(r["best"])                                      # the NaN cells lost, finite ones won
    with pytest.raises(IndexError):
        cc.vanishing_point(cc.vp_lines("n2")[:1])
    assert cc.vanishing_point([[0, 0, 0, 1], [1, 1, 2, 2]])["status"] == cc.VP_BAD_START      # division by x1 = 0


@pytest.mark.parametrize("name", cc.VP_GOLDEN)
def test_restated_vanishing_point_is_the_references(cal, name):
    lines = cal["vp_%s_lines" % name]
    assert np.array_equal(lines, cc.vp_lines(name))                   # the case table regenerates the fixture's inputs
    r = cc.vanishing_point(lines)
    assert np.array_equal(r["point"], cal["vp_%s_point" % name])
    rec = cal["vp_%s_arange" % name]                                   # [16, 2, (start, stop, step, length, first, last)]
    assert np.array_equal(r["bounds"][:, :, 0], rec[:, :, 0]) and np.array_equal(r["bounds"][:, :, 1], rec[:, :, 1])
    assert np.array_equal(r["bounds"][:, :, 2], rec[:, :, 3])
    assert np.array_equal(rec[:, 0, 2], [10.0 ** k for k in range(16, 0, -1)])
    assert np.array_equal(r["trace"][:, 0] - rec[:, 0, 2] * 15.0, rec[:, 0, 0])   # the grid is fixed by the level's start


@pytest.mark.parametrize("d", cc.SZ_D)
def test_restated_scale_z_is_the_references(cal, d):
    """Grids, winners and the final P bit for bit; the errors to ERR_DEV of the search's smallest.  Measured on the
    committed fixture (printed below): d = 1: 6.7e-13, 3: 4.9e-13, 17: 3.3e-11, 65: 1.04e-9, 300: 8.1e-11; ERR_DEV is 4 x
    the largest."""
    tag = "sz_d%d_" % d
    boxes, heights, H, P0 = (cal[tag + k] for k in ("boxes", "heights", "H", "P0"))
    r = cc.scale_z(boxes, heights, H, P0)
    grids, evals = cal[tag + "grids"], cal[tag + "evals"]
    assert r["status"] == 0 and r["iters"] == len(grids) - 1 == len(evals) // 10
    assert np.array_equal(r["trace"][:, :, 0], grids[:-1])
    want = evals[:, 3].reshape(-1, 10)
    got = r["trace"][:, :, 1]
    assert np.array_equal(got.argmin(1), want.argmin(1))              # the same winner at every iteration
    dev = np.abs(got - want).max() / want.min()
    print("d = %d: error deviation %.3e of the smallest error" % (d, dev))
    assert dev <= ERR_DEV
    P = cc.scaled_P(P0, r["last_C"])
    assert np.array_equal(P, cal[tag + "P_final"])                    # bit for bit ...
    assert r["last_C"] == grids[-2, 9] and r["last_C"] != r["best_C"]  # ... and it is the LAST candidate, not the best
    assert np.array_equal(np.stack([cc.scaled_P(P0, C)[:, 2] for C in grids[:-1].reshape(-1)]), evals[:, :3])
    text = bytes(cal[tag + "sz_text"]).decode()
    assert abs(float(text.split("Best Error: ")[1]) - r["best_error"]) <= ERR_DEV * want.min()
    top, bot = cc.reproj_error(boxes, heights, H, P0)
    assert abs((top + bot) - float(cal[tag + "tt_error"])) <= ERR_DEV * float(cal[tag + "tt_error"])


# ------------------------------------------------------------------------------------------------ the drop-in's host side
def _hg():
    from homography import Homography
    return Homography()


def _camera(cal):
    H = cal["sz_d17_H"]
    return H, np.linalg.inv(H)


def test_add_correspondence_with_given_matrices_builds_P_exactly(cal):
    hg = _hg()
    H, H_inv = _camera(cal)
    corr = [[10.0, 20.0], [300.0, 40.0], [500.0, 700.0], [30.0, 600.0]]
    space = [[0.0, 0.0], [100.0, 0.0], [100.0, 50.0], [0.0, 50.0]]
    vps = [[1.0, 2.0], [3.0, 4.0], [960.0, -4509.0021]]
    hg.add_correspondence(corr, space, vps, name="p1c1", H=H, H_inv=H_inv)
    cor = hg.correspondence["p1c1"]
    assert cor["H"] is H and cor["H_inv"] is H_inv                    # stored as they are
    P = np.zeros([3, 4])
    P[:, 0], P[:, 1], P[:, 3] = H_inv[:, 0], H_inv[:, 1], H_inv[:, 2]
    P[:, 2] = np.array([960.0, -4509.0021, 1]) * 0.01
    assert np.array_equal(cor["P"], P) and cor["P"].dtype == np.float64
    assert np.array_equal(cor["corr_pts"], np.array(corr)) and np.array_equal(cor["space_pts"], np.array(space))
    assert cor["vps"] is vps and hg.default_correspondence == "p1c1"
    hg.add_correspondence(corr, space, vps, name="p1c2", H=H, H_inv=H_inv)
    assert hg.default_correspondence == "p1c1" and sorted(hg.correspondence) == ["p1c1", "p1c2"]


def test_remove_correspondence_and_pickle_round_trip(cal):
    hg = _hg()
    H, H_inv = _camera(cal)
    for n in ("a", "b"):
        hg.add_correspondence([[0.0, 0.0]] * 4, [[1.0, 1.0]] * 4, [[0, 0], [0, 0], [5.0, 6.0]], name=n, H=H, H_inv=H_inv)
    back = pickle.loads(pickle.dumps(hg))
    assert sorted(back.correspondence) == ["a", "b"] and back.default_correspondence == "a"
    for k in ("H", "H_inv", "P", "corr_pts", "space_pts"):
        assert np.array_equal(back.correspondence["b"][k], hg.correspondence["b"][k])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        hg.remove_correspondence("b")
        hg.remove_correspondence("b")
    assert out.getvalue() == "Deleted correspondence for b\nTried to delete correspondence b, but this does not exist\n"
    assert sorted(hg.correspondence) == ["a"]


def test_error_cases_that_need_no_device(cal, tmp_path):
    import homography as hgmod
    hg = _hg()
    H, H_inv = _camera(cal)
    hg.add_correspondence([[0.0, 0.0]] * 4, [[1.0, 1.0]] * 4, [[0, 0], [0, 0], [5.0, 6.0]], name="a", H=H, H_inv=H_inv)
    with pytest.raises(IndexError):
        hgmod.find_vanishing_point([[0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(IndexError):
        hgmod.find_vanishing_points([[[0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 3.0]], []])
    with pytest.raises(ValueError):
        hg.scale_Z(torch.zeros(0, 8, 2, dtype=torch.float64), torch.zeros(0))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert hg.test_transformation(torch.zeros(2, 8, 2, dtype=torch.float64)) is None
    assert out.getvalue() == "Must either specify heights or classes for boxes\n"
    with pytest.raises(NotImplementedError):
        hg.test_transformation(torch.zeros(2, 8, 2, dtype=torch.float64), heights=torch.ones(2), im=np.zeros((4, 4, 3)))
    assert hgmod.line_to_point((0.0, 0.0, 4.0, 0.0), (1.0, 3.0)) == 12.0 / (4.0 + 1e-08)
    # get_homographies returns the pickled object when the file exists (homography.py:21-23)
    path = str(tmp_path / "hg.cpkl")
    with open(path, "wb") as f:
        pickle.dump(hg, f)
    back = hgmod.get_homographies(save_file=path, directory=str(tmp_path))
    assert np.array_equal(back.correspondence["a"]["P"], hg.correspondence["a"]["P"])


def test_calibration_ops_are_bound_and_refuse_cpu_tensors():
    from retinanet_mi355x import ops, torch_ops
    for name in ("vanishing_points", "hg_reproj_error", "hg_scale_z", "fit_homography"):
        assert name in torch_ops.OPERATORS
    f64 = torch.float64
    with pytest.raises(RuntimeError):
        ops.vanishing_points(torch.zeros(2, 4, dtype=f64), torch.tensor([0, 2]))
    with pytest.raises(RuntimeError):
        ops.hg_reproj_error(torch.zeros(1, 8, 2, dtype=f64), torch.ones(1), torch.eye(3, dtype=f64), torch.zeros(3, 4, dtype=f64),
                            torch.ones(1, dtype=f64))
    with pytest.raises(RuntimeError):
        ops.hg_scale_z(torch.zeros(1, 8, 2, dtype=f64), torch.ones(1), torch.eye(3, dtype=f64), torch.zeros(3, 4, dtype=f64))
    with pytest.raises(RuntimeError):
        ops.fit_homography(torch.zeros(4, 2, dtype=f64), torch.zeros(4, 2, dtype=f64), torch.tensor([0, 4]))


def test_restated_fit_recovers_a_known_camera_and_reports_degenerate_input(cal):
    H = cal["sz_d17_H"]
    for n in cc.FIT_N:
        im, sp = cc.fit_case(n, H, 500 + n)
        got, status = cc.fit_homography(im, sp)
        assert status == 0 and np.abs(got - H / H[2, 2]).max() <= 1e-12 * np.abs(H / H[2, 2]).max()
    line = np.stack((np.arange(6.0) * 100, np.arange(6.0) * 50 + 3), 1)
    assert cc.fit_homography(line, line * 2)[1] == cc.FIT_DEGENERATE
    assert cc.fit_homography(line[:3], line[:3])[1] == cc.FIT_FEW_POINTS

"""GPU: the crop frame's front end (csrc/track_step.hip, ops.track_crop_prior) -- the filter viewed 1/30 s ahead, the
nearest camera centre per track and the per-track dt -- bit for bit against ``Torch_KF.view`` on the same filter and
against the torch-CPU restatement of MC3D_crop_tracker.py:1156-1171 in tests/tracker_cases.py."""
import numpy as np
import pytest
import torch

import tracker_cases as trc

pytestmark = pytest.mark.gpu

T_OFFSET = 1.0e9          # seconds: an epoch-sized time stamp, so a float32 dt would lose the whole difference


def _filter(dev, X, D, T):
    """A Torch_KF holding exactly these tensors (ids 0 .. n-1)."""
    import track_cases as tc
    from util_track.kf import Torch_KF
    kf = Torch_KF(dev, INIT=tc.kf_init())
    if len(X):
        kf.X, kf.D, kf.T = X.clone(), D.clone(), T.clone()
        kf.P = kf.P0.repeat(len(X), 1, 1)
        kf.obj_idxs = {i: i for i in range(len(X))}
    return kf


def _check(dev, case, op=None):
    from retinanet_mi355x import ops
    X, D, T, centers, stamps, bias = (torch.from_numpy(case[k]).to(dev) for k in ("X", "D", "T", "centers", "stamps", "bias"))
    kf = _filter(dev, X, D, T)
    pre_loc, cam, dt = (op or ops.track_crop_prior)(X, D, T, kf.F, centers, stamps, bias)
    n = len(X)
    assert pre_loc.dtype == torch.float32 and tuple(pre_loc.shape) == (n, 7) and pre_loc.is_cuda
    assert cam.dtype == torch.int32 and tuple(cam.shape) == (n,) and dt.dtype == torch.float64 and tuple(dt.shape) == (n,)
    if n == 0:
        return None
    ids, want = kf.view(with_direction=True, dt=1 / 30.0)
    assert ids == list(range(n))
    got = pre_loc.cpu()
    assert np.array_equal(got.numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))        # bit for bit, NaN included
    want_cam, want_dt = trc.crop_prior_restated(got, torch.from_numpy(case["centers"]), case["stamps"].tolist(),
                                                case["bias"].tolist(), torch.from_numpy(case["T"]))
    assert np.array_equal(cam.cpu().numpy(), want_cam.numpy().astype(np.int32))
    assert np.array_equal(dt.cpu().numpy().view(np.uint64), want_dt.numpy().view(np.uint64))
    return cam.cpu().numpy(), dt.cpu().numpy()


@pytest.mark.parametrize("c", [1, 2, 18])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_crop_prior_is_bit_identical(dev, n, c):
    case = trc.crop_prior_case(n, c, seed=700 + 31 * n + c, t_offset=T_OFFSET)
    out = _check(dev, case)
    if n == 0:
        return
    cam, dt = out
    assert set(np.unique(case["D"])) <= {-1.0, 1.0} and (n < 2 or len(np.unique(case["D"])) == 2)   # both directions
    assert np.array_equal(case["centers"], np.round(case["centers"]))                               # integer-valued centres
    if c > 1:
        for r, k in case["ties"]:                       # rows built to tie between cameras k and k + 1: the lower index
            assert cam[r] == k, (r, k, cam[r])
        assert len(np.unique(cam)) > 1 or n < 3
    for r in case["nan_rows"]:                          # a NaN position: every distance is NaN, the first one wins
        assert cam[r] == 0 and np.isnan(dt[r]) == np.isnan(case["T"][r])
    # the fp64 dt matters: rounded through float32 it would be a multiple of 64 s at this offset
    finite = np.isfinite(dt)
    assert finite.all() and np.abs(dt).max() < 1.0 and np.abs(dt).max() > 0.0


def test_first_nan_distance_wins(dev):
    case = trc.crop_prior_case(65, 6, seed=910, t_offset=T_OFFSET)
    case["centers"] = case["centers"].copy()
    case["centers"][2, 0] = np.nan                      # camera 2's distance is NaN for every track, camera 4's too
    case["centers"][4, 1] = np.nan
    cam, _ = _check(dev, case)
    want = np.full(65, 2)
    want[case["nan_rows"]] = 0                          # a NaN position: camera 0's distance is NaN already
    assert np.array_equal(cam, want)


def test_custom_op_gives_the_same(dev):
    from retinanet_mi355x import ops, torch_ops
    case = trc.crop_prior_case(65, 18, seed=920, t_offset=T_OFFSET)
    a = _check(dev, case)
    b = _check(dev, case, op=torch.ops.retinanet_mi355x.track_crop_prior)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    X, D, T, centers, stamps, bias = (torch.from_numpy(case[k]).to(dev) for k in ("X", "D", "T", "centers", "stamps", "bias"))
    torch.library.opcheck(torch_ops.track_crop_prior, (X, D, T, torch.eye(6, device=dev), centers, stamps, bias),
                          test_utils=("test_schema", "test_autograd_registration"))
    assert ops.track_crop_prior is not None


def test_refusals(dev):
    from retinanet_mi355x import ops
    case = trc.crop_prior_case(5, 3, seed=930, t_offset=0.0)
    cpu = [torch.from_numpy(case[k]) for k in ("X", "D", "T")] + [torch.eye(6)] + \
          [torch.from_numpy(case[k]) for k in ("centers", "stamps", "bias")]
    with pytest.raises(RuntimeError):
        ops.track_crop_prior(*cpu)                                        # CPU tensors
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.retinanet_mi355x.track_crop_prior(*cpu)
    g = [t.to(dev) for t in cpu]
    for i, bad in ((0, g[0].double()), (0, g[0][:, :5]), (1, g[1][:-1]), (2, g[2].float()), (3, g[3][:5]),
                   (4, g[4][:0]), (4, g[4].double()), (5, g[5][:-1]), (6, g[6].float())):
        args = list(g)
        args[i] = bad
        with pytest.raises(RuntimeError):
            ops.track_crop_prior(*args)

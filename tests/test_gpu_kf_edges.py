"""The Kalman filter kernels (rn_kf_view / rn_kf_predict / rn_kf_update of csrc/kf.hip) past their first block, through
every row swap of the 5x5 inverse, with every form of dt and every measurement model, against the float64 reference of
tests/kf_cases.py: through the C ABI between guard bands and through util_track.kf.Torch_KF.
tests/test_kf_cases_host.py proves the cases, the reference and that the comparisons used here reject wrong filters.
view / predict are held to the dot-product bounds, update to UPDATE_M times the float32 oracle's own error; the known
answer case, untouched rows, guard bands, T and view(dt=None) are exact."""
import numpy as np
import pytest
import torch

import kf_cases as kc

pytestmark = pytest.mark.gpu

GUARD = 64                                           # elements of sentinel before and after every buffer
SENTINEL = {torch.float32: -777.25, torch.float64: -777.25, torch.int32: 0x5A5A5A5}


@pytest.fixture(scope="module")
def lib(dev):
    from retinanet_mi355x import _hip
    lib = _hip.load()
    assert lib.rn_check_device() == 0
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded(object):
    """A flat device copy of ``a`` inside a larger buffer full of a sentinel."""

    def __init__(self, a, dev):
        t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
        self.n, self.fill = t.numel(), SENTINEL[t.dtype]
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=t.dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + self.n]
        self.t.copy_(t)
        self.shape = np.shape(a)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def get(self):
        return self.t.cpu().numpy().reshape(self.shape)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _dt_buffer(dt, dev):
    """-> (Guarded float64 buffer, is_tensor flag) the way Torch_KF._dt hands dt to the kernels."""
    if isinstance(dt, np.ndarray):
        return Guarded(dt.astype(np.float64), dev), 1
    return Guarded(np.array([dt], dtype=np.float64), dev), 0


def _assert_within(got, ref, bound, what):
    ok, worst = kc.within(got, ref, bound)
    print("%s: worst err / bound %.3f" % (what, worst))
    assert ok, (what, worst)


def check_update(what, got, start, ref, orc, rows):
    """The figures first, then the assertion: updated rows within UPDATE_M of the oracle's own error, the rest untouched."""
    rx, rp = kc.update_ratios(got, ref, orc, rows)
    print("%s: err / max(err_oracle32, 4u max|ref|), worst object: X %.3f P %.3f (median object: X %.3f P %.3f)"
          % (what, rx.max(), rp.max(), np.median(rx), np.median(rp)))
    assert kc.update_within(got, start, ref, orc, rows, kc.UPDATE_M), (what, float(rx.max()), float(rp.max()))


# ------------------------------------------------------------------------------------------------ C ABI, block edges
@pytest.mark.parametrize("c", kc.block_edge_cases()["predict"], ids=lambda c: c.name)
def test_view_block_edges(lib, dev, c):
    X, D, F = Guarded(c.X, dev), Guarded(c.D.astype(np.float32), dev), Guarded(c.F, dev)
    for wd in (0, 1):
        for dt in (None, c.dt, c.dt0):
            out = Guarded(np.full((c.n, 6 + wd), 5.5, dtype=np.float32), dev)
            dtb, flag = (None, 0) if dt is None else _dt_buffer(dt, dev)
            rc = lib.rn_kf_view(X.ptr(), D.ptr(), F.ptr(), None if dtb is None else dtb.ptr(), flag, wd, out.ptr(), c.n, _stream())
            assert rc == 0
            torch.cuda.synchronize()
            ref = kc.ref_view(c.X, c.D, c.F, dt, bool(wd))
            if dt is None:
                assert np.array_equal(_bits(out.get()), _bits(ref.astype(np.float32)))
            else:
                b = kc.view_bound(c.X, c.D, c.F, dt)
                _assert_within(out.get(), ref, kc.with_dir(b, 0 * c.D) if wd else b, "view %s wd=%d" % (c.name, wd))
            assert out.intact() and (dtb is None or dtb.intact())
    for g, a in ((X, c.X), (D, c.D.astype(np.float32)), (F, c.F)):
        assert g.intact() and np.array_equal(_bits(g.get()), _bits(a))


@pytest.mark.parametrize("c", kc.block_edge_cases()["predict"], ids=lambda c: c.name)
def test_predict_block_edges(lib, dev, c):
    for dt in (c.dt, c.dt0):
        X, P, D, T = Guarded(c.X, dev), Guarded(c.P, dev), Guarded(c.D.astype(np.float32), dev), Guarded(c.T, dev)
        F, Q = Guarded(c.F, dev), Guarded(c.Q, dev)
        dtb, flag = _dt_buffer(dt, dev)
        rc = lib.rn_kf_predict(X.ptr(), P.ptr(), D.ptr(), T.ptr(), F.ptr(), Q.ptr(), dtb.ptr(), flag, kc.DT_DEFAULT, c.n, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        ref = kc.ref_predict(c.X, c.P, c.D, c.T, c.F, c.Q, dt)
        bx, bp = kc.predict_bound(c.X, c.P, c.D, c.F, c.Q, dt)
        what = "predict %s %s" % (c.name, "tensor dt" if flag else "scalar dt")
        _assert_within(X.get(), ref[0], bx, what + " X")
        _assert_within(P.get(), ref[1], bp, what + " P")
        assert np.array_equal(_bits(T.get()), _bits(ref[2]))                       # T + dt, bit for bit
        assert all(g.intact() for g in (X, P, D, T, F, Q, dtb))
        assert np.array_equal(D.get(), c.D) and np.array_equal(F.get(), c.F) and np.array_equal(Q.get(), c.Q)


@pytest.mark.parametrize("c", kc.block_edge_cases()["update"], ids=lambda c: c.name)
def test_update_block_edges(lib, dev, c):
    assert int(c.rows.max()) < c.n and int(c.rows.min()) >= 0 and c.z.shape == (len(c.rows), 5)   # bounds, before any launch
    X, P, rows, z = Guarded(c.X, dev), Guarded(c.P, dev), Guarded(c.rows, dev), Guarded(c.z, dev)
    H, R, mu = Guarded(c.H, dev), Guarded(c.R, dev), Guarded(c.mu_R, dev)
    rc = lib.rn_kf_update(X.ptr(), P.ptr(), rows.ptr(), z.ptr(), H.ptr(), R.ptr(), mu.ptr(), len(c.rows), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    a = (c.X, c.P, c.rows, c.z, c.H, c.R, c.mu_R)
    check_update("update " + c.name, (X.get(), P.get()), (c.X, c.P), kc.ref_update(*a), kc.oracle_update(*a), c.rows)
    assert all(g.intact() for g in (X, P, rows, z, H, R, mu))
    assert np.array_equal(rows.get(), c.rows) and np.array_equal(z.get(), c.z)


# ------------------------------------------------------------------------------------------------ Torch_KF
def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def make_kf(c, dev):
    """A Torch_KF with the case's matrices and objects (ids 100, 101, ...) and its P in place of P0."""
    from util_track.kf import Torch_KF
    INIT = {"P": torch.eye(6), "F": _t(c.F), "H": _t(c.H), "Q": _t(c.Q), "R": _t(c.R), "mu_Q": torch.zeros(6),
            "mu_R": _t(c.mu_R)}
    for k in ("H2", "R2", "mu_R2", "H3", "R3", "mu_R3"):
        if hasattr(c, k):
            INIT[k] = _t(getattr(c, k))
    kf = Torch_KF(dev, INIT=INIT, ADD_MEAN_R=True)
    ids = list(range(100, 100 + c.n))
    kf.add(_t(c.X), ids, _t(c.D), _t(c.T, torch.float64))
    kf.P = _t(c.P).to(dev)
    return kf, ids


def _state(kf):
    return kf.X.cpu().numpy(), kf.P.cpu().numpy()


def _kf_update_check(c, dev, idx, what):
    kf, ids = make_kf(c, dev)
    H, R, mu = kc.measurement_model(c, idx)
    kf.update(_t(c.z, torch.float64), [ids[r] for r in c.rows], measurement_idx=idx)
    a = (c.X, c.P, c.rows, c.z, H, R, mu)
    check_update(what, _state(kf), (c.X, c.P), kc.ref_update(*a), kc.oracle_update(*a), c.rows)


def test_update_takes_every_row_swap(dev):
    _kf_update_check(kc.pivot_cases(), dev, 1, "pivot")


def test_update_exact_known_answer(dev):
    c = kc.exact_pivot_case()
    kf, ids = make_kf(c, dev)
    kf.update(_t(c.z, torch.float64).to(dev), [ids[r] for r in c.rows])
    X, P = _state(kf)
    assert np.array_equal(X, c.want_X)
    assert not P[:, :5].any() and np.array_equal(P[:, 5], c.P[:, 5]) and np.array_equal(P, c.want_P)


@pytest.mark.parametrize("idx", [1, 2, 3])
def test_update_measurement_models(dev, idx):
    _kf_update_check(kc.alt_measurement_case(), dev, idx, "alt-measurement %d" % idx)


def test_update_default_constructor_style(dev):
    """P = P0 = 1e4 I straight after add, numpy measurements as the tracker passes them."""
    from util_track.kf import Torch_KF
    c = kc.default_case()
    kf = Torch_KF(dev)
    ids = list(range(100, 100 + c.n))
    kf.add(_t(c.X[:, :5]), ids, _t(c.D), _t(c.T, torch.float64))
    assert np.array_equal(kf.X.cpu().numpy(), c.X) and np.array_equal(kf.P.cpu().numpy(), c.P)
    kf.update(c.z.astype(np.float32), [ids[r] for r in c.rows])
    a = (c.X, c.P, c.rows, c.z, c.H, c.R, c.mu_R)
    check_update("P0 = 1e4 I", _state(kf), (c.X, c.P), kc.ref_update(*a), kc.oracle_update(*a), c.rows)


@pytest.mark.parametrize("c", kc.dt_cases(), ids=lambda c: c.name)
def test_dt_forms(dev, c):
    kf, ids = make_kf(c, dev)
    if c.form == "float":
        dt = c.dt
    elif c.form == "f64":
        dt = _t(c.dt, torch.float64).to(dev)
    elif c.form == "get_dt":
        dt = kf.get_dt(list(c.targets), idxs=list(c.idxs))                         # as mc3d_track.py does before predict
        assert dt.dtype == torch.float32 and np.array_equal(_bits(dt.cpu().numpy()), _bits(c.dt))
    else:
        dt = kf.get_dt(float(c.target))
        assert dt.dtype == torch.float64 and np.array_equal(_bits(dt.cpu().numpy()), _bits(c.dt)) and bool((dt < 0).any())
    bx, bp = kc.predict_bound(c.X, c.P, c.D, c.F, c.Q, c.dt)
    for wd in (False, True):
        idl, v = kf.view(dt=dt.clone() if isinstance(dt, torch.Tensor) else dt, with_direction=wd)
        assert idl == ids
        _assert_within(v.cpu().numpy(), kc.ref_view(c.X, c.D, c.F, c.dt, wd), kc.with_dir(bx, 0 * c.D) if wd else bx,
                       "view %s wd=%d" % (c.name, wd))
    assert np.array_equal(_bits(kf.X.cpu().numpy()), _bits(c.X))                   # view changes nothing
    kf.predict(dt=dt)
    ref = kc.ref_predict(c.X, c.P, c.D, c.T, c.F, c.Q, c.dt)
    _assert_within(kf.X.cpu().numpy(), ref[0], bx, "predict %s X" % c.name)
    _assert_within(kf.P.cpu().numpy(), ref[1], bp, "predict %s P" % c.name)
    assert np.array_equal(_bits(kf.T.cpu().numpy()), _bits(ref[2]))


def test_long_run(dev):
    c = kc.long_run_case()
    kf, ids = make_kf(c, dev)
    everyone = np.arange(c.n)
    for s in range(kc.LONG_STEPS):
        kf.predict(dt=_t(c.dts[s], torch.float64).to(dev))
        kf.update(_t(c.zs[s], torch.float64), [ids[r] for r in c.rows[s]])
        if s + 1 in kc.LONG_CHECK:
            ref, orc = c.ref[s + 1], c.orc[s + 1]
            rx, rp = kc.update_ratios(_state(kf), ref[:2], orc[:2], everyone)
            print("long run, step %d: err / max(err_oracle32, 4u max|ref|), worst object: X %.3f P %.3f" % (s + 1, rx.max(), rp.max()))
            assert rx.max() <= kc.UPDATE_M and rp.max() <= kc.UPDATE_M, (s + 1, float(rx.max()), float(rp.max()))
            assert np.array_equal(_bits(kf.T.cpu().numpy()), _bits(ref[2]))


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_remove_everything_then_add(dev):
    c = kc.block_edge_cases()["predict"][1]
    kf, ids = make_kf(c, dev)
    kf.remove(list(ids))
    assert len(kf.X) == 0 and kf.obj_idxs == {}
    assert kf.predict() is None and kf.view() == ([], []) and kf.view(dt=0.1, with_direction=True) == ([], [])
    assert kf.get_dt(10.5) is None
    assert len(kf.X) == 0 and len(kf.P) == 0 and len(kf.T) == 0
    kf.add(_t(c.X), ids, _t(c.D), _t(c.T, torch.float64))
    kf.P = _t(c.P).to(dev)
    fresh, _ = make_kf(c, dev)
    dt = _t(c.dt, torch.float64).to(dev)
    kf.predict(dt=dt.clone()), fresh.predict(dt=dt.clone())
    assert kf.obj_idxs == fresh.obj_idxs and kf.view()[0] == ids
    for a, b in ((kf.X, fresh.X), (kf.P, fresh.P), (kf.T, fresh.T), (kf.view(dt=dt)[1], fresh.view(dt=dt)[1])):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    bx, bp = kc.predict_bound(c.X, c.P, c.D, c.F, c.Q, c.dt)
    assert kc.within(kf.P.cpu().numpy(), kc.ref_predict(c.X, c.P, c.D, c.T, c.F, c.Q, c.dt)[1], bp)[0]


def test_add_remove_in_the_middle_then_update(dev):
    """Objects 0..79 plus 80..129 added later, 31 of them removed from the middle: ids keep their objects, rows close
    up, and an update by id moves exactly the rows the reference moves."""
    c = kc.pivot_cases()
    from util_track.kf import Torch_KF
    kf, _ = make_kf(c, dev)
    ids = list(range(100, 100 + c.n))
    first = 80
    kf.remove(ids[first:])
    kf.add(_t(c.X[first:]), ids[first:], _t(c.D[first:]), _t(c.T[first:], torch.float64))
    kf.P[first:] = _t(c.P[first:]).to(dev)
    gone = list(range(40, 71))
    kf.remove([ids[i] for i in gone])
    left = np.array([i for i in range(c.n) if i not in gone])
    assert [kf.obj_idxs[ids[i]] for i in left] == list(range(len(left))) and len(kf.X) == len(left)
    X0, P0 = c.X[left], c.P[left]
    assert np.array_equal(_bits(kf.X.cpu().numpy()), _bits(X0)) and np.array_equal(_bits(kf.P.cpu().numpy()), _bits(P0))
    sel = [k for k, r in enumerate(c.rows) if r not in gone]                      # the case's permuted order, minus the gone
    rows = np.array([int(np.flatnonzero(left == c.rows[k])[0]) for k in sel], dtype=np.int32)
    z = c.z[sel]
    assert len(rows) >= 65 and not np.array_equal(rows, np.sort(rows))
    kf.update(_t(z, torch.float64), [ids[c.rows[k]] for k in sel])
    a = (X0, P0, rows, z, c.H, c.R, c.mu_R)
    check_update("after add / remove", _state(kf), (X0, P0), kc.ref_update(*a), kc.oracle_update(*a), rows)


# ------------------------------------------------------------------------------------------------ refused on the host
def test_shape_mistakes_raise_before_any_launch(dev):
    from util_track.kf import Torch_KF
    c = kc.alt_measurement_case()
    kf, ids = make_kf(c, dev)
    X0, P0 = _state(kf)
    z = _t(c.z[:3], torch.float64)
    with pytest.raises(RuntimeError, match="detections"):
        kf.update(z, ids[:4])                                                     # 3 measurements for 4 objects
    with pytest.raises(RuntimeError, match="detections"):
        kf.update(z[:, :4], ids[:3])                                              # 4 columns
    with pytest.raises(RuntimeError, match="detections"):
        kf.update(z.reshape(-1), ids[:3])
    with pytest.raises(RuntimeError, match="detections"):
        kf.update(np.zeros((3, 6), dtype=np.float32), ids[:3])
    with pytest.raises(RuntimeError, match="dt has"):
        kf.predict(dt=torch.zeros(c.n - 1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="dt has"):
        kf.view(dt=torch.zeros(c.n + 1))
    for name, bad in (("H2", torch.zeros(5, 5, device=dev)), ("H3", torch.zeros(6, 6, device=dev)),
                      ("R2", torch.zeros(5, 5, device=dev)), ("R3", torch.zeros(1, 5, 5)),
                      ("mu_R2", torch.zeros(5, device=dev)), ("mu_R3", torch.zeros(1, 5, dtype=torch.float64, device=dev)),
                      ("H", torch.zeros(6, 5, device=dev)), ("R", torch.zeros(1, 4, 4, device=dev)),
                      ("mu_R", torch.zeros(1, 5))):
        good = getattr(kf, name)
        setattr(kf, name, bad)
        with pytest.raises(RuntimeError, match=name + " must be"):
            kf.update(z, ids[:3], measurement_idx=int(name[-1]) if name[-1] in "23" else 1)
        setattr(kf, name, good)
    with pytest.raises(ValueError):
        kf.update(z, ids[:3], measurement_idx=4)
    assert np.array_equal(_bits(kf.X.cpu().numpy()), _bits(X0)) and np.array_equal(_bits(kf.P.cpu().numpy()), _bits(P0))
    kf.update(z, ids[:3], measurement_idx=2)                                      # and the filter still works
    assert not np.array_equal(kf.X.cpu().numpy()[:3], X0[:3]) and np.array_equal(kf.X.cpu().numpy()[3:], X0[3:])
    d = Torch_KF(dev)                                                             # R2 on the CPU, no H2 / mu_R2 at all
    d.add(_t(c.X[:4, :5]), [0, 1, 2, 3], _t(c.D[:4]), _t(c.T[:4], torch.float64))
    with pytest.raises(RuntimeError, match="must be"):
        d.update(_t(c.z[:2], torch.float64), [0, 1], measurement_idx=2)
    with pytest.raises(RuntimeError, match="must be"):
        d.update(_t(c.z[:2], torch.float64), [0, 1], measurement_idx=3)

"""CPU: the restatement of fixed-interval smoothing (tests/smooth_cases.py) on its scenes, its mathematics against an exact
rational solve of the model's quadratic, and the host half of track_smooth.py (parameters, the model block, packing, copying
``data``).  No device code runs here."""
from fractions import Fraction

import numpy as np
import pytest

import smooth_cases as sc


def test_exact_scene_is_returned_bit_for_bit():
    offsets, cols, direction = sc.exact_scene()
    assert len(cols) == 17 and len(set(np.diff(cols[:, 0]).tolist())) > 1            # uneven steps
    res = sc.smooth(offsets, cols, direction, sc.full_model())
    assert res["status"] == 0 and not res["flag"].any() and (res["nis"] == 0.0).all()
    assert res["out"][:, :6].tobytes() == cols[:, 1:7].tobytes()
    assert res["filt"][:, :6].tobytes() == cols[:, 1:7].tobytes()
    assert (res["out"][:, 5] == 96.0).all() and (res["out"][:, 6:] > 0).all()


@pytest.fixture(scope="module")
def noisy():
    offsets, cols, direction, truth = sc.noisy_scene()
    return offsets, cols, direction, truth, sc.smooth(offsets, cols, direction, sc.NOISY_MODEL)


def test_noisy_scene_flags_the_displaced_rows_and_beats_the_filter(noisy):
    offsets, cols, direction, truth, res = noisy
    assert len(offsets) == 21 and (np.diff(offsets) == 150).all() and sorted(set(direction.tolist())) == [-1, 1]
    sc.check_noisy(offsets, cols, truth, res)
    speed = [np.sqrt(((res["out"][lo:hi, 5] - truth[lo:hi, 6]) ** 2).mean()) for lo, hi in zip(offsets[:-1], offsets[1:])]
    print("smoothed speed RMSE per tracklet: max %.3f" % max(speed))                # a figure, not a bound: the inequalities are above
    M = sc.full(res["filt"][:, 6:])
    assert np.array_equal(M, np.swapaxes(M, 1, 2))                                  # symmetric by construction


def test_edge_scenes(noisy):
    scenes = sc.edge_scenes()
    res = {k: sc.smooth(o, c, d, sc.NOISY_MODEL, gate=g) for k, (o, c, d, g) in scenes.items()}
    assert all(r["status"] == 0 and np.isfinite(r["out"]).all() for r in res.values())
    o, c, d, _ = scenes["short"]
    r = res["short"]
    assert np.diff(o).tolist() == [1, 2, 3]
    assert r["out"][0, :6].tobytes() == c[0, 1:7].tobytes()                         # one row: no step at all, the row and P0
    assert r["out"][0, 6:].tolist() == [4, 4, 4, 4, 4, 100] and r["filt"][0, 6:].tobytes() == sc.NOISY_MODEL[61:].reshape(6, 6)[np.triu_indices(6)].tobytes()
    assert (r["out"][[1, 3], 6:] < r["filt"][[1, 3]][:, [6 + sc.tri(a, a) for a in range(6)]]).all()   # a first row gains from the later ones
    o, c, d, _ = scenes["mixed65"]
    assert len(o) == 66 and sorted(set(np.diff(o).tolist())) == [1, 2, 7, 130]
    order = sc.sorted_order(o)
    assert np.diff(o)[order].tolist() == sorted(np.diff(o).tolist(), reverse=True) and np.diff(o)[order[63]] != np.diff(o)[order[0]]
    r = res["flag_ends"]
    assert r["flag"].nonzero()[0].tolist() == [1, 17]
    assert r["filt"][17, 1:6].tobytes() == r["filt"][16, 1:6].tobytes()             # flagged: s = s-, only x moves in a prediction
    assert r["out"][17].tobytes() == np.concatenate((r["filt"][17, :6], r["filt"][17, [6 + sc.tri(a, a) for a in range(6)]])).tobytes()
    o, c, d, _ = scenes["all_flagged"]
    r = res["all_flagged"]
    first = np.zeros(len(c), bool)
    first[o[:-1]] = True
    assert np.array_equal(r["flag"].astype(bool), ~first)
    assert (r["out"][:, 5] == 95.0).all() and (r["out"][:, 2:5] == c[o[:-1].repeat(np.diff(o)), 3:6]).all()   # nothing but row 0 is used
    o, c, d, _ = scenes["gate_off"]
    assert not res["gate_off"]["flag"].any() and res["gate_off"]["nis"].max() > sc.GATE
    assert sc.smooth(o, c, d, sc.NOISY_MODEL)["flag"].nonzero()[0].tolist() == [5]
    o, c, d, _ = scenes["direction_zero"]
    assert d.sum() == 0
    plus = sc.smooth(o, c, np.ones_like(d), sc.NOISY_MODEL)
    assert plus["out"].tobytes() == res["direction_zero"]["out"].tobytes()
    assert sc.smooth(o, c, -np.ones_like(d), sc.NOISY_MODEL)["out"].tobytes() != plus["out"].tobytes()


def test_refusals_set_their_bit():
    for name, (o, c, d, model, bit) in sc.refusal_scenes().items():
        assert sc.smooth(o, c, d, model)["status"] == bit, name


# ------------------------------------------------------------------------------------------------ the mathematics, exactly
def _inv(M):
    """Gauss-Jordan over the rationals."""
    n = len(M)
    A = [list(row) + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(M)]
    for c in range(n):
        p = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[p] = A[p], A[c]
        piv = A[c][c]
        A[c] = [v / piv for v in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                m = A[r][c]
                A[r] = [v - m * w for v, w in zip(A[r], A[c])]
    return [row[n:] for row in A]


def _mm(A, B):
    return [[sum((A[i][k] * B[k][j] for k in range(len(B))), Fraction(0)) for j in range(len(B[0]))] for i in range(len(A))]


def _tr(A):
    return [list(r) for r in zip(*A)]


def _add(A, B, sign=1):
    return [[a + sign * b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def exact_minimiser(cols, d, model, dt_default):
    """The minimiser over (s_0 .. s_(n-1)) of (s_0 - m_0)' P0^-1 (s_0 - m_0) + sum_k (z_k - H s_k)' R^-1 (z_k - H s_k) + sum_k (s_k - F_k
    s_(k-1))' Qk^-1 (s_k - F_k s_(k-1)), k = 1 .. n-1, by block elimination of its block-tridiagonal normal equations in
    rationals.  dt, f and Qk are the doubles the model defines (one rounding each), taken as exact from there on."""
    Fr = lambda v: Fraction(float(v))
    n = len(cols)
    P0i = _inv([[Fr(model[61 + a * 6 + b]) for b in range(6)] for a in range(6)])
    Ri = _inv([[Fr(model[36 + a * 5 + b]) for b in range(5)] for a in range(5)])
    HRH = [[Ri[a][b] if a < 5 and b < 5 else Fraction(0) for b in range(6)] for a in range(6)]
    diag = [P0i] + [HRH for _ in range(1, n)]
    rhs = [_mm(P0i, [[Fr(v)] for v in cols[0, 1:7]])] + [_mm(HRH, [[Fr(v)] for v in cols[k, 1:6]] + [[Fraction(0)]]) for k in range(1, n)]
    low = [None] * n                                                               # block (k, k-1)
    for k in range(1, n):
        dt = float(cols[k, 0]) - float(cols[k - 1, 0])
        f = float(d) * dt
        Qi = _inv([[Fr((float(model[min(a, b) * 6 + max(a, b)]) * dt) / dt_default) for b in range(6)] for a in range(6)])
        F = [[Fraction(int(a == b)) for b in range(6)] for a in range(6)]
        F[0][5] = Fr(f)
        QF = _mm(Qi, F)
        diag[k] = _add(diag[k], Qi)
        diag[k - 1] = _add(diag[k - 1], _mm(_tr(F), QF))
        low[k] = [[-v for v in row] for row in QF]
    for k in range(1, n):                                                          # forward elimination
        W = _mm(low[k], _inv(diag[k - 1]))
        diag[k] = _add(diag[k], _mm(W, _tr(low[k])), -1)
        rhs[k] = _add(rhs[k], _mm(W, rhs[k - 1]), -1)
    x = [None] * n
    x[n - 1] = _mm(_inv(diag[n - 1]), rhs[n - 1])
    for k in range(n - 2, -1, -1):
        x[k] = _mm(_inv(diag[k]), _add(rhs[k], _mm(_tr(low[k + 1]), x[k + 1]), -1))
    return np.array([[float(v[0]) for v in xk] for xk in x])


MEASURED_REL = 1.851e-15    # the figure in the docstring of the test below and in DESIGN.md


def test_smoothed_means_minimise_the_model_s_quadratic():
    """With gating off the smoothed means are the minimiser of the model's quadratic.  On the seeded tracklets below (2, 3, 5, 8 and
    12 rows, both directions, the noisy scene's model and the full one) the largest relative difference between the restatement
    and the exact rational minimiser, max |got - exact| / |exact| over all means, was measured as 1.851e-15 (at 5 rows; it is
    printed per case); the assertion allows four times that."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for n, d, model in ((2, 1, sc.NOISY_MODEL), (3, -1, sc.NOISY_MODEL), (5, 1, sc.full_model()), (8, -1, sc.full_model()), (12, 1, sc.NOISY_MODEL)):
        o, c, dd = sc.pack([sc._walk(rng, n, d)], [d])
        res = sc.smooth(o, c, dd, model, gate=0.0)
        assert res["status"] == 0
        exact = exact_minimiser(c, d, model, sc.DT_DEFAULT)
        rel = float((np.abs(res["out"][:, :6] - exact) / np.abs(exact)).max())
        print("n = %d: largest relative difference %.3e" % (n, rel))
        worst = max(worst, rel)
    print("largest relative difference %.3e" % worst)
    assert worst <= 4 * MEASURED_REL


# ------------------------------------------------------------------------------------------------ the host half
def test_params_are_validated():
    import track_smooth
    assert track_smooth.DEFAULTS == {"gate": 20.515, "q_scale": 1.0, "r_scale": 1.0, "dt_default": 1 / 30}
    assert track_smooth.resolve_params() == track_smooth.DEFAULTS and track_smooth.resolve_params({"gate": 0})["gate"] == 0.0
    for bad in ({"gates": 1.0}, {"gate": -1.0}, {"gate": float("inf")}, {"q_scale": 0.0}, {"r_scale": float("nan")}, {"dt_default": 0.0}):
        with pytest.raises(ValueError):
            track_smooth.resolve_params(bad)


def _kf(Q=sc.NOISY_Q, R=sc.NOISY_R, P=sc.NOISY_P0):
    import torch
    return {"Q": torch.from_numpy(np.array(Q)), "R": torch.from_numpy(np.array(R)), "P": torch.from_numpy(np.array(P)),
            "H": torch.zeros(3, 3), "mu_Q": torch.ones(6), "mu_R": torch.ones(5)}


def test_model_block_and_its_refusals():
    from retinanet_mi355x import ops
    block = ops.smooth_model(_kf())
    assert block.dtype == np.float64 and block.shape == (ops.SMOOTH_MODEL,) and block.tobytes() == sc.NOISY_MODEL.tobytes()
    assert block[5] == float(np.float32(.05))                                       # widened exactly, not re-parsed
    scaled = ops.smooth_model(_kf(), 2.0, 0.5)
    assert scaled.tobytes() == sc.model_block(sc.NOISY_Q, sc.NOISY_R, sc.NOISY_P0, 2.0, 0.5).tobytes()
    assert (ops.SMOOTH_NONFINITE, ops.SMOOTH_BAD_OFFSETS, ops.SMOOTH_BAD_DT, ops.SMOOTH_PIVOT, ops.SMOOTH_BAD_ORDER) == \
        (sc.NONFINITE, sc.BAD_OFFSETS, sc.BAD_DT, sc.PIVOT, sc.BAD_ORDER)
    asym = sc.NOISY_Q.copy()
    asym[0, 5] = .06
    nan = sc.NOISY_R.copy()
    nan[1, 1] = np.nan
    for bad in (dict(Q=sc.NOISY_Q[:5, :5]), dict(R=sc.NOISY_Q), dict(P=sc.NOISY_P0[:, :5]), dict(Q=asym), dict(R=nan)):
        with pytest.raises(ValueError):
            ops.smooth_model(_kf(**bad))
    for scales in ((0.0, 1.0), (1.0, -1.0), (float("inf"), 1.0)):
        with pytest.raises(ValueError):
            ops.smooth_model(_kf(), *scales)
    with pytest.raises(ValueError):
        ops.smooth_model({"Q": sc.NOISY_Q, "R": sc.NOISY_R})
    ops.smooth_check(0)
    with pytest.raises(RuntimeError, match="time stamp"):
        ops.smooth_check(sc.BAD_DT)


def test_packing_order_and_copying_on_the_host(monkeypatch):
    """smooth_tracks with a stand-in for the device half: one pass through pack_tracklets, the packed row of every datum found
    again, the six fields replaced by Python floats, everything else and the input untouched."""
    import track_smooth
    o, c, d = sc.pack([sc._walk(np.random.default_rng(1), n, 1) for n in (3, 1, 4)], [1, -1, 1])
    c[:, 0] = np.round(np.concatenate((np.arange(3), [1], np.arange(4) + 1)) / 30.0, 4)   # frames shared between the tracks
    data = sc.as_data(o, c, d, ids=[30, 10, 20])
    before = [{k: dict(v) for k, v in f.items()} for f in data]
    assert track_smooth.lane_order(o).tolist() == [2, 0, 1] and track_smooth.lane_order(o).dtype == np.int32
    seen = {}

    def stand_in(offsets, cols, direction, model, params, device=None):
        seen.update(offsets=offsets, cols=cols, model=model, params=params)
        R = len(cols)
        out = np.concatenate((cols[:, 1:7] + 1000.0, np.ones((R, 6))), axis=1)
        return dict(status=np.zeros(1, np.int32), filt=np.zeros((R, 27)), nis=np.zeros(R), flag=np.zeros(R, np.uint8), out=out)
    monkeypatch.setattr(track_smooth, "smooth_packed", stand_in)
    new, report = track_smooth.smooth_tracks(data, _kf(), {"gate": 3})
    assert seen["offsets"].tolist() == [0, 1, 5, 8] and seen["params"]["gate"] == 3.0 and seen["model"].tobytes() == sc.NOISY_MODEL.tobytes()
    assert report["ids"].tolist() == [10, 20, 30] and report["direction"].tolist() == [-1, 1, 1] and report["status"] == 0
    assert report["var"].shape == (8, 6) and report["filtered"].shape == (8, 27) and report["offsets"].tolist() == [0, 1, 5, 8]
    assert data == before and [list(f) for f in new] == [list(f) for f in data]
    for f_new, f_old in zip(new, data):
        for key in f_old:
            a, b = f_new[key], f_old[key]
            assert a is not b and all(type(a[k]) is float and a[k] == b[k] + 1000.0 for k in ("x", "y", "l", "w", "h", "v"))
            assert all(a[k] == b[k] for k in b if k not in ("x", "y", "l", "w", "h", "v"))
    with pytest.raises(ValueError):
        track_smooth.smooth_tracks(data, _kf(), {"gait": 3})


def test_the_operators_are_registered():
    import torch
    from retinanet_mi355x import ops, torch_ops
    for name in ("smooth_filter", "smooth_rts"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    o, c, d = sc.exact_scene()
    t = [torch.from_numpy(a) for a in (o, sc.sorted_order(o), c, d, sc.NOISY_MODEL)]
    with pytest.raises(RuntimeError):
        ops.smooth_filter(*t, sc.GATE, sc.DT_DEFAULT)                               # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.smooth_rts(*t, sc.DT_DEFAULT, torch.zeros(len(c), 27, dtype=torch.float64))

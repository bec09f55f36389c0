"""The cases of tests/kf_cases.py are what they claim, its float64 reference agrees with oracle/kf.py inside the derived
bounds, and its comparisons reject wrong filters (no GPU).  oracle/kf.py itself stays pinned by tests/golden/kf.npz in
test_oracle_golden.py.  The wrong filters are float32 CPU emulations of the kernels with one mistake each; they stand in
for mutating the kernels, which nobody should do on a GPU."""
import numpy as np
import pytest

import kf_cases as kc

U = kc.U


def _update_args(c, idx=1):
    H, R, mu = kc.measurement_model(c, idx)
    return c.X, c.P, c.rows, c.z, H, R, mu


def _update_refs(c, idx=1):
    a = _update_args(c, idx)
    return kc.ref_update(*a), kc.oracle_update(*a)


UPDATE_CASES = ([(c.name, c, 1) for c in kc.block_edge_cases()["update"]]
                + [("pivot", kc.pivot_cases(), 1), ("default", kc.default_case(), 1)]
                + [("alt%d" % i, kc.alt_measurement_case(), i) for i in (1, 2, 3)])


# ------------------------------------------------------------------------------------------------ reference vs oracle
@pytest.mark.parametrize("c", kc.block_edge_cases()["predict"] + kc.dt_cases(), ids=lambda c: c.name)
def test_reference_predict_and_view_equal_oracle(c):
    dts = [c.dt] if hasattr(c, "form") else [c.dt, c.dt0]
    for dt in dts:
        ref = kc.ref_predict(c.X, c.P, c.D, c.T, c.F, c.Q, dt)
        bx, bp = kc.predict_bound(c.X, c.P, c.D, c.F, c.Q, dt)
        emu = kc.emu_predict(c.X, c.P, c.D, c.T, c.F, c.Q, dt, isinstance(dt, np.ndarray))
        assert kc.predict_within(emu, ref, (bx, bp))
        for wd in (False, True):
            rv = kc.ref_view(c.X, c.D, c.F, dt, wd)
            assert np.array_equal(rv, kc.with_dir(ref[0], c.D) if wd else ref[0])
        if getattr(c, "oracle", True):
            assert kc.predict_within(kc.oracle_predict(c, dt), ref, (bx, bp)), c.name
            for wd in (False, True):
                b = kc.with_dir(bx, 0 * c.D) if wd else bx
                assert kc.within(kc.oracle_view(c, dt, wd), kc.ref_view(c.X, c.D, c.F, dt, wd), b)[0]
    assert np.array_equal(kc.ref_view(c.X, c.D, c.F, None, True), kc.with_dir(c.X.astype(np.float64), c.D))


def test_n6_tensor_dt_is_where_the_oracle_departs():
    """At n == 6 ``step4 * dt`` broadcasts along the last axis and raises nothing, so the oracle (as the reference) scales
    column b of every object's Q by dt[b]: outside the bound of the per-object semantics the kernel implements."""
    c = [c for c in kc.dt_cases() if c.name == "f64_n6"][0]
    ref = kc.ref_predict(c.X, c.P, c.D, c.T, c.F, c.Q, c.dt)
    bounds = kc.predict_bound(c.X, c.P, c.D, c.F, c.Q, c.dt)
    assert c.n == 6 and not kc.predict_within(kc.oracle_predict(c, c.dt), ref, bounds)
    assert kc.predict_within(kc.emu_predict(c.X, c.P, c.D, c.T, c.F, c.Q, c.dt, True), ref, bounds)
    assert all(c.n != 6 for c in kc.dt_cases() if c.oracle and kc.dt_is_tensor(c))


def test_dt_cases_cover_zero_negative_and_tiny():
    cases = {c.name: c for c in kc.dt_cases()}
    assert {c.form for c in cases.values()} == {"float", "f64", "get_dt", "get_dt_float"}
    assert sorted(c.dt for c in cases.values() if c.form == "float") == [-0.02, 0.0, 1e-4, 0.05]
    for name in ("f64", "get_dt"):
        dt = cases[name].dt
        assert (dt == 0).any() and (dt < 0).any() and (np.abs(dt - 1e-4) < 1e-6).any() and (dt > 0.01).any()
    g = cases["get_dt"]
    assert g.dt.dtype == np.float32 and np.sum(g.dt == np.float32(kc.DT_DEFAULT)) == g.n - len(g.idxs)
    assert cases["f64"].dt.dtype == np.float64 and (cases["get_dt_float"].dt < 0).any() and (cases["get_dt_float"].dt > 0).any()
    F = cases["f64"].F
    assert np.abs(F - np.eye(6)).min() > 0 and np.abs(F - np.eye(6)).max() < 0.03


@pytest.mark.parametrize("name,c,idx", UPDATE_CASES, ids=[u[0] for u in UPDATE_CASES])
def test_reference_update_equals_oracle(name, c, idx):
    """M = 1 against the oracle is a tautology for the ratio, so the oracle's own error is held to what a backward stable
    float32 inverse owes: 8 cond(S) u of the largest entry that takes part (in or out) per object; and the float32
    emulation of the kernel, a third algorithm on another machine's arithmetic, passes the comparison at 2 UPDATE_M."""
    ref, orc = _update_refs(c, idx)
    H, R, mu = kc.measurement_model(c, idx)
    cond = np.linalg.cond(kc.innovation_cov(c.P, c.rows, H, R))
    rest = np.setdiff1d(np.arange(c.n), c.rows)
    for r, o, start in zip(ref, orc, (c.X, c.P)):
        assert np.array_equal(r[rest], start[rest].astype(np.float64)) and np.array_equal(o[rest], start[rest])
        ax = tuple(range(1, r.ndim))
        scale = np.maximum(np.abs(r[c.rows]).max(axis=ax), np.abs(start[c.rows].astype(np.float64)).max(axis=ax))
        scale = np.maximum(scale, np.abs(c.z).max(axis=1))
        err = np.abs(o[c.rows] - r[c.rows]).max(axis=ax)
        assert np.all(err <= 8 * cond * U * scale), float((err / (cond * U * scale)).max())
    emu = kc.emu_update(*_update_args(c, idx))[:2]
    rx, rp = kc.update_ratios(emu, ref, orc, c.rows)
    print("%s: float32 emulation / oracle error ratio X %.2f P %.2f, cond(S) <= %.3g" % (name, rx.max(), rp.max(), cond.max()))
    assert kc.update_within(emu, (c.X, c.P), ref, orc, c.rows, 2 * kc.UPDATE_M)


# ------------------------------------------------------------------------------------------------ case conditions
def test_block_edge_cases():
    cases = kc.block_edge_cases()
    assert tuple(c.n for c in cases["predict"]) == (1, 127, 128, 129, 257)
    assert sorted(len(c.rows) for c in cases["update"]) == [1, 1, 63, 64, 65, 129]
    for c in cases["update"]:
        r, n = c.rows, c.n
        assert n == 300 and r.dtype == np.int32 and len(set(r.tolist())) == len(r) and r.min() >= 0 and r.max() < n
        assert c.z.shape == (len(r), 5)
        if len(r) > 1:
            assert 0 in r and n - 1 in r
            assert not np.array_equal(r, np.sort(r)) and not np.array_equal(r, np.sort(r)[::-1])
            assert np.abs(np.diff(np.sort(r))).max() > 1
    singles = sorted(int(c.rows[0]) for c in cases["update"] if len(c.rows) == 1)
    assert singles == [0, 299]


def test_pivot_cases_take_every_row_swap():
    c = kc.pivot_cases()
    assert len(c.rows) >= 65 and c.n == 130
    S = kc.innovation_cov(c.P, c.rows, c.H, c.R)
    assert np.linalg.cond(S).max() <= 1e4 and np.linalg.eigvalsh(c.P.astype(np.float64)).min() > 0
    assert np.linalg.eigvalsh(c.R.astype(np.float64)).min() > 0
    piv = kc.emu_update(*_update_args(c))[2]
    assert kc.pivot_pairs_taken(piv) == set(kc.PIVOT_PAIRS) and len(kc.PIVOT_PAIRS) == 10
    for half in (piv[:64], piv[64:]):                        # both update blocks swap rows
        assert (half != np.arange(5)).any()
    # the golden of test_gpu_kf.py never does, which is why these cases exist
    INIT, det, _, _, _, upd, z, _ = __import__("golden_cases").kf_inputs()
    P = np.repeat(INIT["P"].numpy()[None], len(det), axis=0)
    assert not kc.pivot_pairs_taken(kc.gauss_jordan_f32(kc.innovation_cov(P, upd, INIT["H"].numpy(), INIT["R"].numpy()))[1])


def test_other_cases_are_well_conditioned():
    c = kc.alt_measurement_case()
    for idx in (1, 2, 3):
        H, R, mu = kc.measurement_model(c, idx)
        assert H.shape == (5, 6) and R.shape == (5, 5) and mu.shape == (5,)
        assert np.linalg.cond(kc.innovation_cov(c.P, c.rows, H, R)).max() <= 1e4
    mats = [kc.measurement_model(c, i) for i in (1, 2, 3)]
    for k in range(3):
        assert not np.array_equal(mats[0][k], mats[1][k]) and not np.array_equal(mats[0][k], mats[2][k])
        assert not np.array_equal(mats[1][k], mats[2][k])
    assert not c.H3[4].any() and c.R3[4, 4] == 1000 and len(c.rows) >= 65
    d = kc.default_case()
    assert 1e4 <= np.linalg.cond(kc.innovation_cov(d.P, d.rows, d.H, d.R)).max() <= 1.01e4


def test_gauss_jordan_emulation_inverts():
    c = kc.pivot_cases()
    S = kc.innovation_cov(c.P, c.rows, c.H, c.R)
    inv, _ = kc.gauss_jordan_f32(S)
    cond = np.linalg.cond(S)
    err = np.abs(inv.astype(np.float64) @ S - np.eye(5)).max(axis=(1, 2))
    assert np.all(err <= 8 * cond * U), float((err / (cond * U)).max())


def test_exact_pivot_case_is_exact():
    c = kc.exact_pivot_case()
    assert c.n == 120 and len(set(c.rows.tolist())) == 120 and len(c.rows) > 64
    S = kc.innovation_cov(c.P, np.arange(c.n), c.H, c.R)
    assert np.array_equal(S, c.P[:, :5, :5]) and len({s.tobytes() for s in (S != 0)}) == 120
    assert np.all((S != 0).sum(axis=1) == 1) and np.all((S != 0).sum(axis=2) == 1)
    m = np.frexp(S[S != 0])[0]
    assert np.all(m == 0.5) and len(np.unique(S[S != 0])) > 8           # powers of two, several of them
    assert not np.array_equal(c.P, c.P.transpose(0, 2, 1))
    for a in (c.X, c.z, c.mu_R):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 512
    assert np.all(c.X[:, 5] != 0)
    X, P, piv = kc.emu_update(*_update_args(c))
    assert kc.pivot_pairs_taken(piv) == set(kc.PIVOT_PAIRS)
    assert np.array_equal(X, c.want_X) and np.array_equal(P, c.want_P)
    assert not P[:, :5].any() and np.array_equal(P[:, 5], c.P[:, 5])
    assert np.array_equal(X[c.rows, :5], (c.z + c.mu_R).astype(np.float32)) and np.array_equal(X[:, 5], c.X[:, 5])
    ref = kc.ref_update(*_update_args(c))                                # and the float64 equations say the same
    assert np.array_equal(ref[0], c.want_X) and np.array_equal(ref[1], c.want_P)
    bad = kc.emu_update(*_update_args(c), wrong="inv_not_swapped")
    assert not np.array_equal(bad[0], c.want_X)


def test_long_run_case():
    c = kc.long_run_case()
    assert sorted(c.ref) == [1, 10, 100, 300] and c.dts.shape == (300, 40)
    assert all(set(range(40)) - set(r.tolist()) == {i for i in range(40) if (i + s) % 3 == 1} for s, r in enumerate(c.rows))
    for step in kc.LONG_CHECK:
        (rx, rp, rt), (ox, op, ot) = c.ref[step], c.orc[step]
        assert np.array_equal(rt, ot)
        # the float32 oracle alone stays near the float64 run: the filter contracts
        assert np.abs(ox - rx).max() <= 64 * U * np.abs(rx).max() and np.abs(op - rp).max() <= 64 * U * np.abs(rp).max()
    assert np.abs(c.ref[300][1]).max() < np.abs(c.P).max()


# ------------------------------------------------------------------------------------------------ wrong filters
def _predict_rejected(wrong):
    """-> names of the dt cases on which the wrong predict falls outside predict_bound."""
    out = []
    for c in kc.dt_cases() + kc.block_edge_cases()["predict"]:
        ref = kc.ref_predict(c.X, c.P, c.D, c.T, c.F, c.Q, c.dt)
        bounds = kc.predict_bound(c.X, c.P, c.D, c.F, c.Q, c.dt)
        tensor = isinstance(c.dt, np.ndarray)
        assert kc.predict_within(kc.emu_predict(c.X, c.P, c.D, c.T, c.F, c.Q, c.dt, tensor), ref, bounds)
        if not kc.predict_within(kc.emu_predict(c.X, c.P, c.D, c.T, c.F, c.Q, c.dt, tensor, wrong=wrong), ref, bounds):
            out.append(c.name)
    return out


def _update_rejected(wrong, M=2 * kc.UPDATE_M):
    out = []
    for name, c, idx in UPDATE_CASES + [("exact", kc.exact_pivot_case(), 1)]:
        ref, orc = _update_refs(c, idx)
        got = kc.emu_update(*_update_args(c, idx), wrong=wrong)[:2]
        if not kc.update_within(got, (c.X, c.P), ref, orc, c.rows, M):
            out.append(name)
    return out


def test_wrong_filters_are_rejected():
    """Each mistake is caught on the cases built to catch it, at twice the M the GPU tests use."""
    got = _update_rejected("inv_not_swapped")
    assert "pivot" in got and "exact" in got and "default" not in got          # only where rows are swapped
    got = _update_rejected("row_k")
    assert {"m63", "m64", "m65", "m129", "pivot", "alt1", "alt2", "alt3", "default", "exact"} <= set(got)
    assert "m1_row0" not in got                                                # k == rows[k] there: nothing is wrong
    got = _predict_rejected("noise_dt0")
    assert {"f64", "get_dt", "get_dt_float", "n127", "n257"} <= set(got) and not any(n.startswith("float_") for n in got)
    got = _predict_rejected("no_sign")
    assert {"float_-0.02", "float_0.0001", "float_0.05", "f64", "get_dt", "get_dt_float", "n128"} <= set(got)
    assert "float_0" not in got                                                # dt = 0: the sign has nothing to act on
    got = _predict_rejected("noise_unscaled")
    assert {"f64", "f64_n6", "get_dt", "get_dt_float", "n1", "n129"} <= set(got)


def test_update_m_is_recorded():
    assert kc.UPDATE_M == 16

"""Edge cases, a plain float64 reference and derived error bounds for the tracker's Kalman filter kernels (rn_kf_view /
rn_kf_predict / rn_kf_update of csrc/kf.hip, reached through util_track/kf.py:Torch_KF).  tests/test_kf_cases_host.py
proves that the cases are what they claim, that the reference agrees with oracle/kf.py and that the comparisons reject
wrong filters; tests/test_gpu_kf_edges.py runs the kernels on them.

Reference (float64 numpy, per object, from the filter equations; state x = (x, y, l, w, h, v), direction D, time T)
  ref_view      x' = F_i x with F_i = F except F_i[0,5] = D_i dt_i; with_direction puts D between h and v
  ref_predict   x' = F_i x,  P' = F_i P F_i^T + Q dt_i / dt_default,  T' = T + dt_i
  ref_update    y = z + mu_R - H x,  S = H P H^T + R,  K = P H^T S^-1,  x' = x + K y,  P' = (I - K H) P  (rows given)
A scalar dt is the same dt for every object.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u), absolute values taken in float64)
  view / predict do the reference's operations in float32; only summation order and fma contraction are free:
      |err_X| <= (gamma_7 + 2u)  |F_i| |x|
      |err_P| <= (gamma_14 + 2u) (|F_i| |P| |F_i^T| + |Q dt_i / dt_default|)
  gamma_7: a 6-term dot product plus the rounding of F_i[0,5] = D dt;  gamma_14: two of them in a row;  2u = one float32
  ulp: dt (a float64) rounded to float32 where the kernel or the oracle does so, and the result rounded on its way out.
  update depends on cond(S) and on the inverse algorithm (Gauss-Jordan in the kernel, LAPACK in the oracle), so the
  kernel is held to the float32 oracle's own error against the same float64 reference, per object:
      err_obj <= M max(err_oracle32_obj, 4u max|ref_obj|)            (update_ratios gives err_obj over that maximum)
  for X and for P apiece, with UPDATE_M below.

Emulations (float32 numpy): gauss_jordan_f32 is the kernel's elimination order with partial pivoting and returns the
pivot row of each column, which is how the cases prove that they pivot; emu_predict / emu_update follow the kernels'
dtype choices and take ``wrong=`` to produce the deliberately wrong filters that the comparisons must reject.

Everything is deterministic (retinanet_mi355x.synth, numpy.random.default_rng(seed)); nothing here touches a GPU.
"""
import functools
import itertools
import types

import numpy as np
import torch

import golden_cases as gc
from oracle import kf as okf
from retinanet_mi355x import synth

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
DT_DEFAULT = 1 / 30.0

# err_kernel / max(err_oracle32, 4u max|ref|), worst object over X and P, measured on an MI355X (gfx950) per family:
#   pivot 6.04 (P; X 1.08) | alt-measurement 1.04 | long run 1.43 (step 100) | P0 = 1e4 I 0.16 | block edges 1.18
# UPDATE_M = smallest power of two >= 2 * worst ratio = 2 * 6.04.  The pivot family's figure is the tail of a quotient of
# two round-off errors of the same order, not a weaker inverse: over its 100 objects the median quotient is 0.91 in P
# and 0.16 in X.  P' = (I - K H) P cancels there from max|P| of several hundred to a few tens, which leaves either
# algorithm with a few u max|P|, and the quotient is large where the oracle happens to keep about one.
UPDATE_M = 16


def gamma(k):
    return k * U / (1 - k * U)


def _sq(a, k):
    return np.asarray(a, dtype=F64).reshape(k)


# ------------------------------------------------------------------------------------------------ float64 reference
def _F_rep(F, D, dt):
    D = np.asarray(D, dtype=F64)
    Fr = np.repeat(_sq(F, (1, 6, 6)), len(D), axis=0)
    Fr[:, 0, 5] = D * np.asarray(dt, dtype=F64)
    return Fr


def with_dir(x, D):
    """[n,6] -> [n,7]: the direction between h and v."""
    return np.concatenate((x[:, :5], np.asarray(D, dtype=x.dtype)[:, None], x[:, 5:]), axis=1)


def ref_view(X, D, F, dt=None, with_direction=False):
    x = np.asarray(X, dtype=F64)
    if dt is not None:
        x = np.einsum("nab,nb->na", _F_rep(F, D, dt), x)
    return with_dir(x, D) if with_direction else x


def ref_predict(X, P, D, T, F, Q, dt, dt_default=DT_DEFAULT):
    """-> (X, P, T) in float64; dt a number or [n]."""
    Fr = _F_rep(F, D, dt)
    dtv = np.broadcast_to(np.asarray(dt, dtype=F64), (len(Fr),))
    Xn = np.einsum("nab,nb->na", Fr, np.asarray(X, dtype=F64))
    Pn = Fr @ np.asarray(P, dtype=F64) @ Fr.transpose(0, 2, 1) + _sq(Q, (1, 6, 6)) * dtv[:, None, None] / dt_default
    return Xn, Pn, np.asarray(T, dtype=F64) + dtv


def innovation_cov(P, rows, H, R):
    """S = H P H^T + R of the updated objects, float64 [m,5,5]."""
    H = _sq(H, (5, 6))
    return H @ np.asarray(P, dtype=F64)[rows] @ H.T + _sq(R, (5, 5))


def ref_update(X, P, rows, z, H, R, mu_R):
    """-> (X, P) in float64 with the objects in ``rows`` updated by z [m,5], every other row as it was."""
    Xo, Po = np.array(X, dtype=F64), np.array(P, dtype=F64)
    H, R, mu = _sq(H, (5, 6)), _sq(R, (5, 5)), _sq(mu_R, (5,))
    for k, r in enumerate(rows):
        x, p = Xo[r].copy(), Po[r].copy()
        y = np.asarray(z[k], dtype=F64) + mu - H @ x
        K = p @ H.T @ np.linalg.inv(H @ p @ H.T + R)
        Xo[r] = x + K @ y
        Po[r] = (np.eye(6) - K @ H) @ p
    return Xo, Po


# ------------------------------------------------------------------------------------------------ bounds, comparisons
def view_bound(X, D, F, dt):
    """[n,6] bound on |view - ref_view| (the direction column of with_direction is exact)."""
    return (gamma(7) + 2 * U) * np.einsum("nab,nb->na", np.abs(_F_rep(F, D, dt)), np.abs(np.asarray(X, dtype=F64)))


def predict_bound(X, P, D, F, Q, dt, dt_default=DT_DEFAULT):
    """-> ([n,6], [n,6,6]) bounds on |predict - ref_predict| in X and P."""
    Fa = np.abs(_F_rep(F, D, dt))
    dtv = np.broadcast_to(np.asarray(dt, dtype=F64), (len(Fa),))
    noise = np.abs(_sq(Q, (1, 6, 6)) * dtv[:, None, None] / dt_default)
    bP = (gamma(14) + 2 * U) * (Fa @ np.abs(np.asarray(P, dtype=F64)) @ Fa.transpose(0, 2, 1) + noise)
    return view_bound(X, D, F, dt), bP


def within(got, ref, bound):
    """-> (ok, worst err / bound); a zero bound asks for equality."""
    err = np.abs(np.asarray(got, dtype=F64) - ref)
    if not np.all(np.isfinite(err)):
        return False, np.inf
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    return bool(np.all(err <= bound)), worst


def predict_within(got, ref, bounds):
    """got, ref = (X, P, T): X and P inside their bounds, T bit for bit."""
    okx, _ = within(got[0], ref[0], bounds[0])
    okp, _ = within(got[1], ref[1], bounds[1])
    return okx and okp and np.array_equal(np.asarray(got[2], dtype=F64), ref[2])


def update_ratios(got, ref, orc, rows):
    """err_obj / max(err_oracle32_obj, 4u max|ref_obj|) of the updated objects -> ([m] for X, [m] for P); got, ref and
    orc are (X, P) of the kernel, the float64 reference and the float32 oracle."""
    out = []
    for g, r, o in zip(got, ref, orc):
        g, o = np.asarray(g, dtype=F64)[rows], np.asarray(o, dtype=F64)[rows]
        r = r[rows]
        ax = tuple(range(1, r.ndim))
        err, err_o = np.abs(g - r).max(axis=ax), np.abs(o - r).max(axis=ax)
        err = np.where(np.isfinite(err), err, np.inf)
        out.append(err / np.maximum(err_o, 4 * U * np.abs(r).max(axis=ax)))
    return out


def update_within(got, start, ref, orc, rows, M):
    """The updated rows inside M times the oracle's own error, every other row of (X, P) bit for bit as in ``start``."""
    rx, rp = update_ratios(got, ref, orc, rows)
    rest = np.setdiff1d(np.arange(len(start[0])), rows)
    same = all(np.array_equal(np.asarray(g)[rest].view(np.uint32), np.asarray(s)[rest].view(np.uint32))
               for g, s in zip(got, start))
    return bool(rx.max() <= M and rp.max() <= M and same)


# ------------------------------------------------------------------------------------------------ float32 emulations
def gauss_jordan_f32(S, swap_inv=True):
    """Gauss-Jordan inverse with partial pivoting in float32, the kernel's order of operations (first largest |entry| at
    or below the diagonal wins) -> (inv [m,5,5], pivot row taken in each column [m,5]).  ``swap_inv=False`` is the wrong
    filter that swaps the rows of S only."""
    S = np.array(S, dtype=F32)
    m, ar = len(S), np.arange(len(S))
    inv = np.repeat(np.eye(5, dtype=F32)[None], m, axis=0)
    piv = np.zeros((m, 5), dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(5):
            p = c + np.argmax(np.abs(S[:, c:, c]), axis=1)
            piv[:, c] = p
            for A in ((S, inv) if swap_inv else (S,)):
                top = A[ar, c].copy()
                A[ar, c] = A[ar, p]
                A[ar, p] = top
            d = F32(1) / S[:, c, c]
            S[:, c] *= d[:, None]
            inv[:, c] *= d[:, None]
            for a in range(5):
                if a != c:
                    f = S[:, a, c].copy()
                    S[:, a] -= f[:, None] * S[:, c]
                    inv[:, a] -= f[:, None] * inv[:, c]
    return inv, piv


def emu_predict(X, P, D, T, F, Q, dt, is_tensor, dt_default=DT_DEFAULT, wrong=None):
    """rn_kf_predict in float32 numpy -> (X, P, T).  wrong: "no_sign" (F[0,5] = dt), "noise_dt0" (every object's noise
    from dt[0]), "noise_unscaled" (tensor-dt noise = Q)."""
    X, P, D = np.asarray(X, dtype=F32), np.asarray(P, dtype=F32), np.asarray(D, dtype=F32)
    Q = np.asarray(Q, dtype=F32).reshape(1, 6, 6)
    n = len(X)
    dtv = np.broadcast_to(np.asarray(dt, dtype=F64), (n,))
    sign = np.ones_like(D) if wrong == "no_sign" else D
    Fr = np.repeat(np.asarray(F, dtype=F32).reshape(1, 6, 6), n, axis=0)
    Fr[:, 0, 5] = (sign.astype(F64) * dtv).astype(F32) if is_tensor else sign * dtv.astype(F32)
    Xn = np.einsum("nab,nb->na", Fr, X)
    s = Fr @ P @ Fr.transpose(0, 2, 1)
    dn = np.full(n, dtv[0]) if wrong == "noise_dt0" else dtv
    if is_tensor:
        noise = Q.astype(F64) * (1.0 if wrong == "noise_unscaled" else dn[:, None, None] / dt_default)
        Pn = (s.astype(F64) + noise).astype(F32)
    else:
        Pn = s + Q * dn.astype(F32)[:, None, None] / F32(dt_default)
    return Xn, Pn, np.asarray(T, dtype=F64) + dtv


def emu_update(X, P, rows, z, H, R, mu_R, wrong=None):
    """rn_kf_update in float32 numpy -> (X, P, pivot rows [m,5]).  wrong: "inv_not_swapped", "row_k" (object rows[k]
    is read and the result written to row k)."""
    Xo, Po = np.array(X, dtype=F32), np.array(P, dtype=F32)
    H, R = np.asarray(H, dtype=F32).reshape(5, 6), np.asarray(R, dtype=F32).reshape(5, 5)
    mu = np.asarray(mu_R, dtype=F32).reshape(5)
    rows = np.asarray(rows, dtype=np.int64)
    x, p = Xo[rows], Po[rows]
    y = ((np.asarray(z, dtype=F64) + mu.astype(F64)) - (x @ H.T).astype(F64)).astype(F32)
    S = H @ p @ H.T + R
    inv, piv = gauss_jordan_f32(S, swap_inv=wrong != "inv_not_swapped")
    with np.errstate(all="ignore"):
        K = p @ H.T @ inv
        dst = np.arange(len(rows)) if wrong == "row_k" else rows
        Xo[dst] = x + np.einsum("nab,nb->na", K, y)
        Po[dst] = (np.eye(6, dtype=F32) - K @ H) @ p
    return Xo, Po, piv


# ------------------------------------------------------------------------------------------------ oracle/kf.py, as numpy
def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def oracle_view(c, dt, with_direction=False):
    dt = _t(dt, torch.from_numpy(np.asarray(dt)).dtype) if isinstance(dt, np.ndarray) else dt
    return okf.view(_t(c.X), _t(c.D), _t(c.F), dt, with_direction).numpy()


def oracle_predict(c, dt):
    """dt: a Python float, or a float64 / float32 numpy array, each taking the path it takes in the tracker."""
    dt = _t(dt, torch.from_numpy(np.asarray(dt)).dtype) if isinstance(dt, np.ndarray) else dt
    X, P, T = okf.predict(_t(c.X), _t(c.P), _t(c.D), _t(c.T, torch.float64), _t(c.F), _t(c.Q).reshape(1, 6, 6), dt, DT_DEFAULT)
    return X.numpy(), P.numpy(), T.numpy()


def oracle_update(X, P, rows, z, H, R, mu_R):
    X, P = okf.update(_t(X), _t(P), [int(r) for r in rows], _t(z, torch.float64), _t(H), _t(R).reshape(1, 5, 5),
                      _t(mu_R).reshape(1, 5))
    return X.numpy(), P.numpy()


# ------------------------------------------------------------------------------------------------ building blocks
def model():
    """F (not the identity), H, Q, R, mu_R of the tracker's shapes: H / Q / R / mu_R as in golden_cases.kf_inputs."""
    INIT = gc.kf_inputs()[0]
    F = np.eye(6, dtype=F32) + (synth.uniform((6, 6), 707) - F32(0.5)) * F32(0.05)
    return types.SimpleNamespace(F=F, H=INIT["H"].numpy(), Q=INIT["Q"].numpy(), R=INIT["R"].numpy(), mu_R=INIT["mu_R"].numpy())


def objects(n, seed):
    """n tracked vehicles: X [n,6] (speed 60..120), an SPD P apiece, D in {+1,-1}, T around 10 s."""
    st = synth.vehicle_states(n, seed=seed).numpy()
    X = np.concatenate((st[:, :5], 60 + 60 * synth.uniform((n, 1), seed + 11)), axis=1).astype(F32)
    a = synth.uniform((n, 6, 6), seed + 12).astype(F64) - 0.5
    scale = 5.0 + 40.0 * synth.uniform((n, 1, 1), seed + 13).astype(F64)
    P = ((a @ a.transpose(0, 2, 1) + np.eye(6)) * scale).astype(F32)
    T = synth.uniform((n,), seed + 14).astype(F64) * 0.2 + 10.0
    return X, P, st[:, 5].copy(), T


def make_case(name, n, seed, **kw):
    X, P, D, T = objects(n, seed)
    c = model()
    c.__dict__.update(name=name, n=n, X=X, P=P, D=D, T=T)
    c.__dict__.update(kw)
    return c


def permuted_rows(n, m, seed):
    """m distinct rows of 0..n-1 in a seeded order that is neither sorted nor contiguous; rows 0 and n-1 are among them
    (m = 1 leaves room for one of the two: n-1)."""
    rng = np.random.default_rng(seed)
    if m == 1:
        return np.array([n - 1], dtype=np.int32)
    inner = rng.permutation(np.arange(1, n - 1))[:m - 2]
    return rng.permutation(np.concatenate(([0, n - 1], inner))).astype(np.int32)


def measurements(X, rows, seed, spread=3.0):
    return (np.asarray(X, dtype=F64)[rows, :5] + (synth.uniform((len(rows), 5), seed).astype(F64) - 0.5) * spread)


# ------------------------------------------------------------------------------------------------ block edges
BLOCK_N = (1, 127, 128, 129, 257)            # view / predict: 128 lanes per block
BLOCK_M = (1, 63, 64, 65, 129)               # update: 64 lanes per block
UPDATE_N = 300


@functools.lru_cache(maxsize=None)
def block_edge_cases():
    """-> {"predict": cases with a per-object dt [n] and a scalar dt0, "update": cases on a filter of 300 objects with
    rows / z}.  m = 1 comes twice, once with row 0 and once with row n-1, since one row cannot be both."""
    pred = [make_case("n%d" % n, n, 900 + n, dt=synth.uniform((n,), 950 + n).astype(F64) * 0.08 + 0.01, dt0=0.04)
            for n in BLOCK_N]
    upd = []
    for m in BLOCK_M:
        c = make_case("m%d" % m, UPDATE_N, 1200 + m, rows=permuted_rows(UPDATE_N, m, 1300 + m))
        c.z = measurements(c.X, c.rows, 1400 + m)
        upd.append(c)
    c = make_case("m1_row0", UPDATE_N, 1201, rows=np.array([0], dtype=np.int32))
    c.z = measurements(c.X, c.rows, 1401)
    upd.append(c)
    return {"predict": pred, "update": upd}


# ------------------------------------------------------------------------------------------------ pivots
PIVOT_N, PIVOT_M, PIVOT_SEED, PIVOT_RHO = 130, 100, 0, 0.9
PIVOT_PAIRS = [(c, a) for c in range(5) for a in range(c + 1, 5)]


def correlated_spd(k, sigma, rho, signs):
    """diag(sigma) C diag(sigma) with C = (1 - rho) I + rho e e^T, e = signs: every pair correlated +-rho."""
    C = (1 - rho) * np.eye(k) + rho * np.outer(signs, signs)
    return C * np.outer(sigma, sigma)


@functools.lru_cache(maxsize=None)
def pivot_cases():
    """A freshly added object next to long-tracked ones: SPD P_i and R with correlation 0.9 and per-coordinate standard
    deviations 10^U(-0.5, 1.5), so that |S[a][c]| > S[c][c] happens in every column.  130 objects, 100 of them updated in
    a permuted order (two update blocks)."""
    rng = np.random.default_rng(PIVOT_SEED)
    c = make_case("pivot", PIVOT_N, 1500, rows=permuted_rows(PIVOT_N, PIVOT_M, 1501))
    for i in range(PIVOT_N):
        c.P[i] = correlated_spd(6, 10 ** rng.uniform(-0.5, 1.5, 6), PIVOT_RHO, rng.choice([-1.0, 1.0], 6)).astype(F32)
    c.R = correlated_spd(5, 10 ** rng.uniform(-0.5, 1.5, 5), PIVOT_RHO, rng.choice([-1.0, 1.0], 5)).astype(F32)
    c.z = measurements(c.X, c.rows, 1502, spread=20.0)
    return c


def pivot_pairs_taken(piv):
    """{(column, pivot row)} with pivot row > column in an [m,5] pivot table."""
    return {(col, int(a)) for col in range(5) for a in np.unique(piv[:, col]) if a > col}


@functools.lru_cache(maxsize=None)
def exact_pivot_case():
    """Known answer, zero tolerance.  H = [I5 | 0], R = 0, P_i = blockdiag(Pi_i D_i, 1) with Pi_i each of the 120
    permutation matrices of size 5 and D_i a diagonal of powers of two (not symmetric: the kernel does not assume it).
    S_i = Pi_i D_i exactly, every elimination step is exact in float32 and K = [I5; 0], so with integer x, z, mu_R:
    X_new[:5] = z + mu_R, X_new[5] = x[5], rows 0-4 of P_new are +-0 and row 5 is unchanged, bit for bit."""
    rng = np.random.default_rng(77)
    perms = list(itertools.permutations(range(5)))
    n = len(perms)
    c = types.SimpleNamespace(name="exact_pivot", n=n, F=np.eye(6, dtype=F32), Q=np.eye(6, dtype=F32))
    c.H = np.eye(5, 6, dtype=F32)
    c.R = np.zeros((5, 5), dtype=F32)
    c.mu_R = np.array([3, -2, 1, 4, -5], dtype=F32)
    c.P = np.zeros((n, 6, 6), dtype=F32)
    for i, perm in enumerate(perms):
        d = 2.0 ** rng.integers(-6, 7, 5)
        for col, row in enumerate(perm):
            c.P[i, row, col] = d[col]
        c.P[i, 5, 5] = 1
    c.X = rng.integers(-200, 201, (n, 6)).astype(F32)
    c.X[:, 5] = rng.integers(1, 100, n)
    c.D = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(F32)
    c.T = np.full(n, 10.0)
    c.rows = rng.permutation(n).astype(np.int32)
    c.z = rng.integers(-300, 301, (n, 5)).astype(F64)
    c.want_X = c.X.copy()
    c.want_X[c.rows, :5] = (c.z + c.mu_R).astype(F32)
    c.want_P = np.zeros_like(c.P)
    c.want_P[:, 5] = c.P[:, 5]
    return c


# ------------------------------------------------------------------------------------------------ dt
def get_dt_f32(T, targets, idxs, dt_default=DT_DEFAULT):
    """Torch_KF.get_dt(list, idxs) as numpy: a float32 [n] of dt_default with target - T at idxs."""
    dt = np.zeros(len(T), dtype=F32) + F32(dt_default)
    idxs = np.asarray(idxs, dtype=np.int64)
    dt[idxs] = (np.asarray(targets, dtype=F64)[:len(idxs)] - np.asarray(T, dtype=F64)[idxs]).astype(F32)
    return dt


DT_N = 37


@functools.lru_cache(maxsize=None)
def dt_cases():
    """Predict / view with every form of dt the tracker hands over, zero, negative (a track ahead of the frame) and tiny
    values among them; D takes both signs, F is not the identity.  form: "float" (a Python float, the all-float32 path),
    "f64" (a float64 tensor [n]), "get_dt" (the float32 tensor of get_dt(targets, idxs), mc3d_track.py:229), "get_dt_float"
    (the float64 tensor of get_dt(float), here a time that lies before some tracks).  ``dt`` is what reaches predict:
    a float or a numpy array of the tensor's dtype.

    n stays away from 6 wherever a tensor dt meets oracle/kf.py: at n == 6 the reference's ``step4 * dt`` broadcasts
    [6,6,6] * [6] along the last axis instead of per object and never reaches its per-object fallback, and the oracle
    copies that.  "f64_n6" is therefore compared with ref_predict only (``oracle=False``)."""
    out = []
    for k, v in enumerate((0.0, -0.02, 1e-4, 0.05)):
        out.append(make_case("float_%g" % v, DT_N, 1600 + k, form="float", dt=v, oracle=True))
    c = make_case("f64", DT_N, 1610, form="f64", oracle=True)
    c.dt = synth.uniform((DT_N,), 1611).astype(F64) * 0.12 - 0.04
    c.dt[[0, 5, DT_N - 1]] = (0.0, 1e-4, -0.03)
    out.append(c)
    c = make_case("get_dt", DT_N, 1620, form="get_dt", oracle=True)
    c.idxs = [3, 7, 0, 36, 20, 11]
    c.targets = [float(c.T[3]), float(c.T[7]) - 0.05, float(c.T[0]) + 1e-4, float(c.T[36]) + 0.07, float(c.T[20]) - 0.2, 10.3]
    c.dt = get_dt_f32(c.T, c.targets, c.idxs)
    out.append(c)
    c = make_case("get_dt_float", DT_N, 1630, form="get_dt_float", oracle=True, target=10.1)
    c.dt = c.target - c.T
    out.append(c)
    c = make_case("f64_n6", 6, 1640, form="f64", oracle=False)
    c.dt = np.array([0.0, -0.02, 1e-4, 0.05, 0.03, -0.01])
    out.append(c)
    assert all(set(np.unique(c.D)) == {-1.0, 1.0} for c in out)
    return out


def dt_is_tensor(c):
    return c.form != "float"


# ------------------------------------------------------------------------------------------------ other measurements
@functools.lru_cache(maxsize=None)
def alt_measurement_case():
    """H2 / R2 / mu_R2 and H3 / R3 / mu_R3 next to H / R / mu_R, all different: H2 scales l and also sees the speed a
    little through x and y, H3 has a zero row (h is not measured) that a large R3 entry pads.  80 objects, 70 updated."""
    c = make_case("alt", 80, 1700, rows=permuted_rows(80, 70, 1701))
    c.z = measurements(c.X, c.rows, 1702)
    H2 = np.eye(5, 6, dtype=F32)
    H2[0, 5], H2[1, 5], H2[2, 2] = -0.2, 0.1, 0.5
    H3 = np.eye(5, 6, dtype=F32)
    H3[4, 4] = 0
    a = synth.uniform((5, 5), 1703).astype(F64) - 0.5
    c.H2, c.R2 = H2, ((a @ a.T + np.eye(5)) * 3.0).astype(F32)
    c.mu_R2 = (synth.uniform((5,), 1704) - F32(0.5)).astype(F32) * F32(2)
    a = synth.uniform((5, 5), 1705).astype(F64) - 0.5
    R3 = (a @ a.T + np.eye(5)) * 0.7
    R3[4, :], R3[:, 4], R3[4, 4] = 0, 0, 1000.0
    c.H3, c.R3 = H3, R3.astype(F32)
    c.mu_R3 = (synth.uniform((5,), 1706) - F32(0.5)).astype(F32)
    return c


def measurement_model(c, idx):
    s = "" if idx == 1 else str(idx)
    return getattr(c, "H" + s), getattr(c, "R" + s), getattr(c, "mu_R" + s)


@functools.lru_cache(maxsize=None)
def default_case():
    """The default constructor's filter on the 40 objects of kf_inputs straight after add: P = P0 = 1e4 I, F = I, H sees
    4 of the 5 measurements, R = I, so S = diag(10001 x 4, 1)."""
    _, det, directions, times, speed, upd_ids, z, _ = gc.kf_inputs()
    n = len(det)
    c = types.SimpleNamespace(name="default", n=n, F=np.eye(6, dtype=F32), Q=np.eye(6, dtype=F32), R=np.eye(5, dtype=F32),
                              mu_R=np.zeros(5, dtype=F32))
    c.H = np.zeros((5, 6), dtype=F32)
    c.H[:4, :4] = np.eye(4)
    c.X = np.concatenate((det.numpy(), np.zeros((n, 1), dtype=F32)), axis=1)
    c.P = np.repeat(np.eye(6, dtype=F32)[None] * F32(10000), n, axis=0)
    c.D, c.T = directions.numpy(), times.numpy()
    c.rows, c.z = np.array(upd_ids, dtype=np.int32), z.numpy().astype(F64)
    return c


# ------------------------------------------------------------------------------------------------ long run
LONG_STEPS, LONG_CHECK = 300, (1, 10, 100, 300)


@functools.lru_cache(maxsize=None)
def long_run_case():
    """300 cycles of predict (a float64 dt tensor) and update on the 40 objects of kf_inputs with its matrices; the
    updated subset rotates, (i + step) % 3 != 1, and the measurements are drawn around the float64 state, so the filter
    contracts and the run is well conditioned.  Holds the float64 reference and the float32 oracle after the steps of
    LONG_CHECK: ``ref[step]`` / ``orc[step]`` = (X, P, T)."""
    INIT, det, directions, times, speed, _, _, _ = gc.kf_inputs()
    n = len(det)
    c = types.SimpleNamespace(name="long_run", n=n, F=INIT["F"].numpy(), H=INIT["H"].numpy(), Q=INIT["Q"].numpy(),
                              R=INIT["R"].numpy(), mu_R=INIT["mu_R"].numpy())
    c.X = np.concatenate((det.numpy(), speed.numpy()[:, None]), axis=1)
    c.P = np.repeat(INIT["P"].numpy()[None], n, axis=0)
    c.D, c.T = directions.numpy(), times.numpy()
    c.dts = synth.uniform((LONG_STEPS, n), 1800).astype(F64) * 0.08 + 0.01
    c.rows = [np.array([i for i in range(n) if (i + s) % 3 != 1], dtype=np.int32) for s in range(LONG_STEPS)]
    c.zs, c.ref, c.orc = [], {}, {}
    ref = (c.X.astype(F64), c.P.astype(F64), c.T.copy())
    orc = (c.X, c.P, c.T.copy())
    for s in range(LONG_STEPS):
        ref = ref_predict(ref[0], ref[1], c.D, ref[2], c.F, c.Q, c.dts[s])
        z = ref[0][c.rows[s], :5] + (synth.uniform((len(c.rows[s]), 5), 1900 + s).astype(F64) - 0.5) * 3.0
        c.zs.append(z)
        ref = ref_update(ref[0], ref[1], c.rows[s], z, c.H, c.R, c.mu_R) + (ref[2],)
        o = types.SimpleNamespace(X=orc[0], P=orc[1], D=c.D, T=orc[2], F=c.F, Q=c.Q)
        orc = oracle_predict(o, c.dts[s])
        orc = oracle_update(orc[0], orc[1], c.rows[s], z, c.H, c.R, c.mu_R) + (orc[2],)
        if s + 1 in LONG_CHECK:
            c.ref[s + 1], c.orc[s + 1] = ref, orc
    return c

"""Fixed-interval smoothing (track_smooth.py, csrc/smooth.hip): the plain restatement of both passes in numpy -- fp64 with one
rounding per operation, every product and sum written out element by element in the order the device evaluates it (no ``@``, dot,
einsum or linalg: BLAS may fuse or reorder) --, the scenes and what they must show.

Layout.  A tracklet is all rows of one id in time order: offsets int64 [N+1], cols fp64 [R,7] = (t, x, y, l, w, h, v), direction
int32 [R].  The model block is fp64 [97] = q_scale Q (36), r_scale R (25), P0 (36), row-major.  A covariance is its 21 entries
a <= b, row-major (``tri``); ``filt`` [R,27] = the 6 filtered means and that triangle, ``out`` [R,12] = the 6 smoothed means and
variances.

The restatement is vectorised over tracklets: every "scalar" below is an array with one element per tracklet, and a tracklet
that is refused (a status bit) or has run out of rows keeps its state through ``np.where``.
"""
import numpy as np

NONFINITE, BAD_OFFSETS, BAD_DT, PIVOT, BAD_ORDER = 1, 2, 4, 8, 16
GATE = 20.515                                                   # chi-square, 5 degrees of freedom, 0.999
DT_DEFAULT = 1 / 30
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]


def tri(a, b):
    if a > b:
        a, b = b, a
    return a * 6 - a * (a - 1) // 2 + (b - a)


def model_block(Q, R, P0, q_scale=1.0, r_scale=1.0):
    """The packed block from float32 matrices, widened exactly, as ops.smooth_model builds it."""
    Q, R, P0 = (np.asarray(m, np.float32).astype(np.float64) for m in (Q, R, P0))
    return np.concatenate(((q_scale * Q).reshape(-1), (r_scale * R).reshape(-1), P0.reshape(-1)))


# ------------------------------------------------------------------------------------------------ the restatement
def predict(s, U, f, dt, model, dt_default):
    """F s and F P F^T + Qk in the sparse form: row 0 of G = F P, then column 0 of G F^T, only a <= b."""
    sp = list(s)
    sp[0] = s[0] + f * s[5]
    G0 = [U[tri(0, b)] + f * U[tri(5, b)] for b in range(6)]
    Um = list(U)
    Um[tri(0, 0)] = G0[0] + f * G0[5]
    for b in range(1, 6):
        Um[tri(0, b)] = G0[b]
    for a, b in PAIRS:
        Um[tri(a, b)] = Um[tri(a, b)] + (model[a * 6 + b] * dt) / dt_default
    return sp, Um


def ldl(S, n):
    """S = L D L^T, Cholesky-Crout order, no square roots; S(i, j) is read for i >= j.  -> (L, D, bad pivot)."""
    L = [[None] * n for _ in range(n)]
    D = [None] * n
    bad = False
    for j in range(n):
        v = [L[j][k] * D[k] for k in range(j)]
        acc = S(j, j)
        for k in range(j):
            acc = acc - L[j][k] * v[k]
        D[j] = acc
        bad = bad | ~(acc > 0.0) | ~np.isfinite(acc)
        for i in range(j + 1, n):
            acc = S(i, j)
            for k in range(j):
                acc = acc - L[i][k] * v[k]
            L[i][j] = acc / D[j]
    return L, D, bad


def solve(L, D, n, rhs):
    w = [None] * n
    for i in range(n):
        acc = rhs[i]
        for k in range(i):
            acc = acc - L[i][k] * w[k]
        w[i] = acc
    u = [w[i] / D[i] for i in range(n)]
    x = [None] * n
    for i in range(n - 1, -1, -1):
        acc = u[i]
        for k in range(i + 1, n):
            acc = acc - L[k][i] * x[k]
        x[i] = acc
    return x


def dotp(a, b):
    """Ascending index, left to right, starting from the first product."""
    acc = a[0] * b[0]
    for k in range(1, len(a)):
        acc = acc + a[k] * b[k]
    return acc


def update(sp, Um, z, model, gate):
    """-> (s, U, nis, flagged, bad pivot): the gated Joseph-form update of one row."""
    Rm = model[36:61]
    y = [z[j] - sp[j] for j in range(5)]
    L, D, bad = ldl(lambda i, j: Um[tri(j, i)] + Rm[j * 5 + i], 5)
    nis = dotp(y, solve(L, D, 5, y))
    flagged = (nis > gate) if gate > 0.0 else np.zeros(np.shape(nis), bool)
    K = [solve(L, D, 5, [Um[tri(a, j)] for j in range(5)]) for a in range(6)]
    s = [sp[a] + dotp(K[a], y) for a in range(6)]
    A = [[(1.0 if a == c else 0.0) - K[a][c] for c in range(5)] + [1.0 if a == 5 else 0.0] for a in range(6)]
    U = [None] * 21
    for a in range(6):
        B = [dotp(A[a], [Um[tri(c, b)] for c in range(6)]) for b in range(6)]
        KR = [dotp(K[a], [Rm[i * 5 + j] for i in range(5)]) for j in range(5)]
        for b in range(a, 6):
            U[tri(a, b)] = dotp(B, A[b]) + dotp(KR, K[b])
    s = [np.where(flagged, sp[a], s[a]) for a in range(6)]
    U = [np.where(flagged, Um[i], U[i]) for i in range(21)]
    return s, U, nis, flagged, bad


def rts_step(s, U, ss, Us, f, dt, model, dt_default):
    """One backward step: (filtered k, smoothed k+1) -> (smoothed k, bad pivot)."""
    sp, Um = predict(s, U, f, dt, model, dt_default)
    L, D, bad = ldl(lambda i, j: Um[tri(j, i)], 6)
    C = [solve(L, D, 6, [U[tri(a, 0)] + f * U[tri(a, 5)]] + [U[tri(a, b)] for b in range(1, 6)]) for a in range(6)]
    e = [ss[b] - sp[b] for b in range(6)]
    Dl = [Us[i] - Um[i] for i in range(21)]
    out_s = [s[a] + dotp(C[a], e) for a in range(6)]
    out_U = [None] * 21
    for a in range(6):
        E = [dotp(C[a], [Dl[tri(b, c)] for b in range(6)]) for c in range(6)]
        for b in range(a, 6):
            out_U[tri(a, b)] = U[tri(a, b)] + dotp(E, C[b])
    return out_s, out_U, bad


def _geometry(offsets, cols, direction):
    N, R = len(offsets) - 1, len(cols)
    lo, hi = np.asarray(offsets[:-1], np.int64), np.asarray(offsets[1:], np.int64)
    ok = (lo >= 0) & (hi > lo) & (hi <= R)
    d = np.ones(N)
    for i in np.nonzero(ok)[0]:
        d[i] = 1.0 if int(np.asarray(direction[lo[i]:hi[i]], np.int64).sum()) >= 0 else -1.0
    return N, R, lo, hi, ok, d


def smooth(offsets, cols, direction, model, gate=GATE, dt_default=DT_DEFAULT):
    """Both passes -> dict(filt [R,27], nis [R], flag uint8 [R], out [R,12], cov [R,21] = the smoothed covariances, status).  The
    rows of a refused tracklet are unspecified (zeros here)."""
    cols, model = np.asarray(cols, np.float64).reshape(-1, 7), np.asarray(model, np.float64)
    N, R, lo, hi, ok, d = _geometry(offsets, cols, direction)
    filt, nis, flag = np.zeros((R, 27)), np.zeros(R), np.zeros(R, np.uint8)
    out, cov = np.zeros((R, 12)), np.zeros((R, 21))
    status = BAD_OFFSETS if not ok.all() else 0
    if N == 0 or R == 0:
        return dict(filt=filt, nis=nis, flag=flag, out=out, cov=cov, status=status)
    n = np.where(ok, hi - lo, 0)
    row = lambda j: np.clip(lo + j, 0, R - 1)
    alive = ok.copy()
    with np.errstate(all="ignore"):
        # ---- forward
        c = cols[row(0)]
        fin = np.isfinite(c).all(axis=1)
        status |= NONFINITE if (alive & ~fin).any() else 0
        alive &= fin
        s = [c[:, 1 + a].copy() for a in range(6)]
        U = [np.full(N, model[61 + a * 6 + b]) for a, b in PAIRS]
        r = row(0)[alive]
        filt[r] = np.stack(s + U, axis=1)[alive]
        t_prev = c[:, 0]
        for j in range(1, int(n.max())):
            act = alive & (n > j)
            c = cols[row(j)]
            fin = np.isfinite(c).all(axis=1)
            status |= NONFINITE if (act & ~fin).any() else 0
            alive &= ~(act & ~fin)
            act &= fin
            dt = c[:, 0] - t_prev
            good = dt > 0.0
            status |= BAD_DT if (act & ~good).any() else 0
            alive &= ~(act & ~good)
            act &= good
            sp, Um = predict(s, U, d * dt, dt, model, dt_default)
            s2, U2, nis_j, flagged, bad = update(sp, Um, [c[:, 1 + q] for q in range(5)], model, gate)
            status |= PIVOT if (act & bad).any() else 0
            alive &= ~(act & bad)
            act &= ~bad
            s = [np.where(act, s2[a], s[a]) for a in range(6)]
            U = [np.where(act, U2[i], U[i]) for i in range(21)]
            t_prev = np.where(act, c[:, 0], t_prev)
            r = row(j)[act]
            filt[r] = np.stack(s + U, axis=1)[act]
            nis[r] = nis_j[act]
            flag[r] = flagged[act]
        # ---- backward: a tracklet joins at its own last row
        ss, Us = [np.zeros(N) for _ in range(6)], [np.zeros(N) for _ in range(21)]
        for j in range(int(n.max()) - 1, -1, -1):
            last, act = alive & (n == j + 1), alive & (n > j + 1)
            fr = filt[row(j)]
            s, U = [fr[:, a] for a in range(6)], [fr[:, 6 + i] for i in range(21)]
            dt = cols[row(j + 1), 0] - cols[row(j), 0]
            s2, U2, bad = rts_step(s, U, ss, Us, d * dt, dt, model, dt_default)
            status |= PIVOT if (act & bad).any() else 0
            alive &= ~(act & bad)
            act &= ~bad
            ss = [np.where(last, s[a], np.where(act, s2[a], ss[a])) for a in range(6)]
            Us = [np.where(last, U[i], np.where(act, U2[i], Us[i])) for i in range(21)]
            w = last | act
            r = row(j)[w]
            out[r] = np.stack(ss + [Us[tri(a, a)] for a in range(6)], axis=1)[w]
            cov[r] = np.stack(Us, axis=1)[w]
    return dict(filt=filt, nis=nis, flag=flag, out=out, cov=cov, status=int(status))


def sorted_order(offsets):
    """What the host passes: the stable argsort of descending length."""
    return np.argsort(-np.diff(np.asarray(offsets, np.int64)), kind="stable").astype(np.int32)


def full(tri21):
    """[..., 21] -> the symmetric [..., 6, 6]."""
    tri21 = np.asarray(tri21)
    M = np.zeros(tri21.shape[:-1] + (6, 6))
    for a in range(6):
        for b in range(6):
            M[..., a, b] = tri21[..., tri(a, b)]
    return M


# ------------------------------------------------------------------------------------------------ scenes
NOISY_R = np.diag([1, .25, .25, .09, .09]).astype(np.float32)
NOISY_R[0, 2] = NOISY_R[2, 0] = 0.1
NOISY_Q = np.diag([.05, .02, .001, .001, .001, .5]).astype(np.float32)
NOISY_Q[0, 5] = NOISY_Q[5, 0] = .05
NOISY_P0 = np.diag([4, 4, 4, 4, 4, 100]).astype(np.float32)
NOISY_MODEL = model_block(NOISY_Q, NOISY_R, NOISY_P0)


def full_model():
    """A full (no zero entry) symmetric positive definite Q, R and P0 in float32, for the exact scene."""
    def spd(n, seed, scale):
        g = np.random.default_rng(seed).standard_normal((n, n))
        return ((g @ g.T + n * np.eye(n)) * scale).astype(np.float32)
    mats = [spd(6, 11, 0.05), spd(5, 12, 0.2), spd(6, 13, 2.0)]
    mats = [np.triu(m) + np.triu(m, 1).T for m in mats]
    return model_block(*mats)


def pack(tracks, directions):
    """tracks: a list of [n,7] arrays -> (offsets, cols, direction)."""
    offsets = np.concatenate(([0], np.cumsum([len(t) for t in tracks]))).astype(np.int64)
    cols = np.concatenate([np.asarray(t, np.float64).reshape(-1, 7) for t in tracks]) if tracks else np.zeros((0, 7))
    direction = np.concatenate([np.full(len(t), dd, np.int32) for t, dd in zip(tracks, directions)]) if tracks else np.zeros(0, np.int32)
    return offsets, cols, direction.astype(np.int32)


def exact_scene():
    """Uneven dyadic steps, constant speed: every innovation is exactly 0."""
    k = np.array([q for q in range(20) if q not in (3, 4, 9)], np.float64)
    t = 64 + k / 32
    tr = np.stack([t, 512 - 96 * (t - 64), np.full_like(t, 30.0), np.full_like(t, 18.5), np.full_like(t, 6.25), np.full_like(t, 5.5),
                   np.full_like(t, 96.0)], axis=1)
    return pack([tr], [-1])


def noisy_tracks(n_tracks=20, n_rows=150, seed=2024, displaced=(40, 90)):
    """-> (tracks [n,7] noisy, truth [n,7], directions).  Rows drawn from 300 frames at 30 Hz; v = 100 + 8 sin(t/3 + i), x its
    trapezoid integral; noise from NOISY_R; the first speed off by 5; rows 40 and 90 displaced by 30 ft in x."""
    rng = np.random.default_rng(seed)
    Lc = np.linalg.cholesky(NOISY_R.astype(np.float64))
    tracks, truths, dirs = [], [], []
    for i in range(n_tracks):
        d = 1 if i % 2 == 0 else -1
        frames = np.arange(300)
        tf = 10.0 * i + frames / 30.0
        vf = 100 + 8 * np.sin(tf / 3 + i)
        xf = (200.0 if d > 0 else 1800.0) + d * np.concatenate(([0.0], np.cumsum((vf[1:] + vf[:-1]) / 2 * np.diff(tf))))
        pick = np.sort(rng.choice(300, n_rows, replace=False))
        truth = np.stack([tf[pick], xf[pick], np.full(n_rows, 12.0 + 6 * (i % 4)), np.full(n_rows, 15.0 + i % 5),
                          np.full(n_rows, 6.0 + 0.1 * i), np.full(n_rows, 5.0 + 0.05 * i), vf[pick]], axis=1)
        noisy = truth.copy()
        noisy[:, 1:6] += rng.standard_normal((n_rows, 5)) @ Lc.T
        noisy[:, 6] += rng.standard_normal(n_rows) * 1.5           # the speed column of rows after the first is never read
        noisy[0, 6] = truth[0, 6] + 5.0
        for r in displaced:
            if r < n_rows:
                noisy[r, 1] += 30.0
        tracks.append(noisy)
        truths.append(truth)
        dirs.append(d)
    return tracks, truths, dirs


def noisy_scene():
    tracks, truths, dirs = noisy_tracks()
    return pack(tracks, dirs) + (np.concatenate(truths),)


def check_noisy(offsets, cols, truth, res, displaced=(40, 90)):
    """The inequalities of the noisy scene, per tracklet, on any result laid out like ``smooth``'s (cov optional)."""
    assert res["status"] == 0
    for i in range(len(offsets) - 1):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        flag = res["flag"][lo:hi].astype(bool)
        assert all(flag[r] for r in displaced), (i, np.nonzero(flag)[0])
        others = int(flag.sum()) - len(displaced)
        assert others <= 1 and others <= 0.02 * (hi - lo - len(displaced)), (i, np.nonzero(flag)[0])
        rmse = lambda a: np.sqrt(((a - truth[lo:hi, 1:7]) ** 2).mean(axis=0))
        raw, fil, smo = rmse(cols[lo:hi, 1:7]), rmse(res["filt"][lo:hi, :6]), rmse(res["out"][lo:hi, :6])
        assert (smo[:5] < raw[:5]).all(), (i, smo, raw)
        assert (smo < fil).all(), (i, smo, fil)
        assert (res["out"][lo:hi, 6:] > 0).all()
        if "cov" in res:
            assert (np.linalg.eigvalsh(full(res["cov"][lo:hi])) > 0).all(), i


def _walk(rng, n, d, t0=5.0, jitter=True):
    """A short noisy tracklet of n rows."""
    t = t0 + np.cumsum(np.concatenate(([0.0], (1 + rng.integers(0, 3, n - 1)) / 30.0))) if n > 1 else np.array([t0])
    x = 700.0 + d * 95.0 * (t - t0)
    tr = np.stack([t, x, np.full(n, 40.0), np.full(n, 17.0), np.full(n, 6.5), np.full(n, 5.2), np.full(n, 95.0)], axis=1)
    if jitter:
        tr[:, 1:6] += rng.standard_normal((n, 5)) * np.array([1.0, .5, .5, .3, .3])
    return tr


def edge_scenes():
    """name -> (offsets, cols, direction, gate)."""
    rng = np.random.default_rng(77)
    out = {}
    out["short"] = pack([_walk(rng, 1, 1), _walk(rng, 2, -1), _walk(rng, 3, 1)], [1, -1, 1]) + (GATE,)
    lens = [(1, 2, 7, 130)[q % 4] for q in range(65)]
    lens[64] = 7
    out["mixed65"] = pack([_walk(rng, n, 1 if q % 3 else -1) for q, n in enumerate(lens)], [1 if q % 3 else -1 for q in range(65)]) + (GATE,)
    a, b = _walk(rng, 9, 1), _walk(rng, 9, -1)
    a[1, 1] += 40.0                                               # flagged directly after the first row
    b[8, 1] -= 40.0                                               # ... and as the last row
    out["flag_ends"] = pack([a, b], [1, -1]) + (GATE,)
    out["all_flagged"] = pack([_walk(rng, 8, 1), _walk(rng, 5, -1)], [1, -1]) + (1e-9,)
    c = _walk(rng, 12, 1)
    c[5, 1] += 40.0
    out["gate_off"] = pack([c, _walk(rng, 6, -1)], [1, -1]) + (0.0,)
    offsets, cols, direction = pack([_walk(rng, 6, 1)], [1])
    direction[:] = [1, -1, 1, -1, -1, 1]                          # sums to 0: d = +1
    out["direction_zero"] = (offsets, cols, direction, GATE)
    return out


def refusal_scenes():
    """name -> (offsets, cols, direction, model, the status bit)."""
    rng = np.random.default_rng(78)
    base = lambda: pack([_walk(rng, 5, 1), _walk(rng, 4, -1), _walk(rng, 6, 1)], [1, -1, 1])
    out = {}
    o, c, d = base()
    c[7, 3] = np.nan
    out["nan"] = (o, c, d, NOISY_MODEL, NONFINITE)
    o, c, d = base()
    out["empty"] = (np.array([0, 5, 5, 9, 15], np.int64), c, d, NOISY_MODEL, BAD_OFFSETS)
    o, c, d = base()
    c[11, 0] = c[10, 0]
    out["repeat"] = (o, c, d, NOISY_MODEL, BAD_DT)
    Q = NOISY_Q.copy()
    Q[0, 0] = -900.0                                              # indefinite: S[0][0] = P-[0][0] + R[0][0] < 0 after one step
    o, c, d = base()
    out["indefinite"] = (o, c, d, model_block(Q, NOISY_R, NOISY_P0), PIVOT)
    return out


def as_data(offsets, cols, direction, ids=None):
    """The packed arrays as ``Data_Reader.data``: one dict per unique rounded time stamp, ascending."""
    N = len(offsets) - 1
    ids = list(range(100, 100 + N)) if ids is None else ids
    frames = {}
    for i in range(N):
        for r in range(int(offsets[i]), int(offsets[i + 1])):
            ts = np.round(cols[r, 0], 4)
            item = {"id": ids[i], "timestamp": ts, "class": "sedan", "camera": "p1c1", "direction": int(direction[r]),
                    "ts_bias": {"p1c1": 0.0}, "frame": "0"}
            item.update(zip(("x", "y", "l", "w", "h", "v"), (float(v) for v in cols[r, 1:7])))
            frames.setdefault(ts, {})[ids[i]] = item
    return [frames[ts] for ts in sorted(frames)]


def golden_scene(g, n=20):
    """The first n tracklets of tests/golden/track_stitch.npz (the reference's shipped tracking output)."""
    offsets = np.asarray(g["offsets"][:n + 1], np.int64)
    R = int(offsets[-1])
    return offsets, np.asarray(g["cols"][:R], np.float64), np.asarray(g["direction"][:R], np.int32)


def fragments(seed=9):
    """One vehicle in two fragments (ids 11 and 12, frames 0-19 and 30-59 at 30 Hz) with noise on x and y -> ``data``."""
    rng = np.random.default_rng(seed)
    tracks = []
    for lo, hi in ((0, 20), (30, 60)):
        t = 100.0 + np.arange(lo, hi) / 30.0
        tr = np.stack([t, 300.0 + 95.0 * (t - 100.0), np.full_like(t, 20.0), np.full_like(t, 16.0), np.full_like(t, 6.0),
                       np.full_like(t, 5.0), np.full_like(t, 95.0)], axis=1)
        tr[:, 1:3] += rng.standard_normal((hi - lo, 2)) * np.array([0.4, 0.2])
        tracks.append(tr)
    offsets, cols, direction = pack(tracks, [1, 1])
    return as_data(offsets, cols, direction, ids=[11, 12])

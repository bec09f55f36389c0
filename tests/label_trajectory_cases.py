"""Scripted label sets and a plain fp64 restatement of the smoothing-spline trajectories (label_trajectory.py /
csrc/label_spline.hip): create_trajectory, get_splines, gen_trajectories and adjust_ts_with_trajectories of the reference's
annotator.  No GPU, no package import: tools/make_golden_label_trajectory.py runs the reference's own methods and scipy's
UnivariateSpline on ``golden_scenes()`` (-> tests/golden/label_trajectory.npz), the tests rebuild the same scenes here, and the
restatement is the oracle of the kernels on the fuzz and edge scenes.

The fit (``fit``) is FITPACK's fpcurf for iopt = 0 written with Python floats -- fp64, one rounding per operation -- statement
by statement in the kernel's order, with 1-based lists so that the indices read like FITPACK's: fpbspl, the Givens pass in
row order (fpgivs / fprota), fpback, the nplus rule, fpknot, the interpolation knots of label 10, fpdisc, the search for p and
fprati.  Where FITPACK reads its table q of basis values the restatement (like the kernel) recomputes them with the interval of
the least-squares pass.  UnivariateSpline first calls fpcurf with nest = max(m / 2, 2k + 2) and, on ier = 1, again with iopt = 1
and nest = m + k + 1 (``_reset_nest``): the second call finds the same knots and sums but enters with ier = 1, so it adds ONE
knot next instead of what the nplus rule gives, and a batch of new knots stops at the first nest; both are restated.
``int()`` of the nplus rule is the truncation of the reference's build (out of range: the most negative
integer).  A lane stops at the knot limit (``REJECTED``): with iopt = 0 knots are only added, so the reference would skip
that candidate anyway.  The scores are summed in ascending row order (numpy's np.mean sums pairwise: the golden tool asserts a
relative gap of 1e-9 between the winner and every other distinct score, so the winner is comparable exactly).

Internal entry points take the candidate lists ``tpex`` / ``tpey`` (the public defaults stay np.logspace(1, 0, 200) and
np.logspace(2, 0, 100)): a pure-Python fit costs tens of milliseconds, so the tests run the restatement on a few candidates.

golden_scenes():
  "traj"  3 cameras, 130 frames, last_frame 125, ids 0..8 and 11 (9 is the first unused id: 11 is ignored):
          0 east-bound through all cameras; 1 west-bound (y > 60: the wrapper's other side); 2 lasts just under 3 s (no spline);
          3 just over 3 s; 4 seen by one camera; 5 has exactly four boxes (k + 1 for x); 6 zig-zags in x so that every x
          candidate passes the knot limit ([None, None]); 7 zig-zags in y only (x succeeds, y fails: [None, None]); 8 is
          short-lived beside the others so that some (frame, camera) hold one kept object and some only objects without a spline.
"""
import copy
import math

import numpy as np

import label_audit_cases as lc
import label_rewrite_cases as rc

F32, F64 = np.float32, np.float64
REJECTED, STUCK, UNUSED = 99, 98, 97
MAXIT = 20
INT_MIN = -2 ** 31
STATE_KEYS = ("x", "y", "l", "w", "h", "direction")


def tpe_x(n=200):
    return list(np.logspace(1, 0, n))


def tpe_y(n=100):
    return list(np.logspace(2, 0, n))


def smoothing(tpe, m):
    """:1236 ``tpex**2*sum(interp)``: a numpy fp64 scalar times a 0-d int64 tensor is torch's product, in fp32 -- the square is
    rounded to fp32 and multiplied by fp32(m) there; scipy then reads that fp32 value as its s."""
    return float(F32(F64(tpe) * F64(tpe)) * F32(m))


# ------------------------------------------------------------------------------------------------ scenes
class Labels(rc.Labels):
    """rc.Labels (``hg`` = the scene's homography) with ``splines``."""

    def __init__(self, scene, side_cls=rc.Side, pair_cls=rc.Pair):
        rc.Labels.__init__(self, scene, side_cls, pair_cls)
        self.splines = None


def drive(s, oid, f0, n, x0, v, y, rng, step=1, cams=None, wob=4.0, wf=0.9, wy=0.0, nx=0.25, ny=0.08, zx=0.0, zy=0.0):
    """An object along x at v ft/s with a slow wobble, noise (nx, ny) and a zig-zag (zx, zy), in the cameras that see it."""
    k = 0
    for f in range(f0, f0 + n, step):
        t = (f - f0) / 30.0
        x = x0 + v * t + wob * math.sin(wf * t)
        for c in range(len(s["names"])) if cams is None else cams:
            if 60.0 * c - 15.0 <= x <= 60.0 * c + 85.0:
                z = 1.0 if k % 2 else -1.0
                lc.put(s, f, c, oid, x + rng.normal(0, nx) + zx * z, y + 0.3 * t + wy * math.sin(1.7 * t) + rng.normal(0, ny) + zy * z, cls=oid)
                k += 1


def scene_traj(seed=41, n_frames=130, last_frame=125):
    s = lc.empty_scene(3, n_frames, seed=seed, last_frame=last_frame)
    rng = np.random.RandomState(seed + 1)
    drive(s, 0, 0, 130, -10.0, 45.0, 30.0, rng, wf=2.5, wy=1.5, nx=0.12, ny=0.3)
    drive(s, 1, 2, 125, 200.0, -44.0, 90.0, rng, wf=2.0, wy=3.0, nx=0.2, ny=0.5)
    drive(s, 2, 5, 89, 0.0, 30.0, 20.0, rng)                    # under 3 s
    drive(s, 3, 10, 93, 20.0, 38.0, 40.0, rng, wf=3.0, wy=1.0, nx=0.1, ny=0.2)  # over 3 s
    drive(s, 4, 0, 120, 70.0, 14.0, 50.0, rng, cams=[1], wob=2.0, wf=1.5, wy=2.0, ny=0.6)
    drive(s, 5, 3, 121, 10.0, 15.0, 25.0, rng, step=40, cams=[0], wob=0.0)
    drive(s, 6, 0, 110, 30.0, 35.0, 35.0, rng, zx=6.0)
    drive(s, 7, 8, 110, 50.0, 30.0, 45.0, rng, zy=25.0)
    drive(s, 8, 100, 24, 150.0, 20.0, 15.0, rng, cams=[2])
    drive(s, 11, 3, 10, 10.0, 30.0, 40.0, rng)                  # above the first unused id (9)
    s["hg_old"] = rc.hg_spec(s["names"])
    return s


def golden_scenes():
    return {"traj": scene_traj()}


def without_id(scene, oid):
    """A deep copy of ``scene`` without the boxes of ``oid`` (adjust_boxes_with_trajectories indexes ``splines`` with every id
    of a frame, so the ignored id above the first unused one would end the reference's run with an IndexError)."""
    s = copy.deepcopy(scene)
    for frame in s["data"]:
        for key in [k for k, d in frame.items() if d["id"] == oid]:
            del frame[key]
    return s


def fuzz_scene(seed):
    """3 cameras x 100 frames x 6 ids: random speeds, lanes, noise; one object too short, one zig-zag."""
    rng = np.random.RandomState(900 + seed)
    s = lc.empty_scene(3, 100, seed=300 + seed, last_frame=int(rng.randint(92, 100)))
    for oid in range(6):
        west = rng.rand() < 0.4
        f0 = int(rng.randint(0, 6))
        n = int(rng.randint(92, 100 - f0 + 1)) if oid != 4 else int(rng.randint(40, 89))
        x0 = rng.uniform(150, 200) if west else rng.uniform(-10, 30)
        v = rng.uniform(25, 45) * (-1 if west else 1)
        drive(s, oid, f0, n, x0, v, rng.uniform(70, 110) if west else rng.uniform(10, 50), rng, step=int(rng.randint(1, 4)),
              wob=rng.uniform(0, 5), nx=rng.uniform(0.05, 0.5), ny=rng.uniform(0.02, 0.2), zx=5.0 if oid == 5 else 0.0)
    s["hg_old"] = rc.hg_spec(s["names"], seed=800 + seed, scale=0.002)
    return s


DIRECT_SEEDS = tuple(range(48))


def direct_case(seed):
    """A small fit of its own -> (x, y, w, k, s): 5..39 points, k 2 or 3, a sine, a square wave, noise or an exponential, and
    a smoothing factor between 1e-12 and 1e3.  Together the seeds reach ier -2, 0 and 3, the interpolation knots of both
    parities of k, and the second call of UnivariateSpline (ier = 1 at the first nest)."""
    rng = np.random.RandomState(seed)
    m, k = int(rng.randint(5, 40)), int(rng.choice([2, 3]))
    x = np.cumsum(rng.uniform(0.01, 1.0, m))
    y = [np.sin(x), np.sign(np.sin(2 * x)) * 5, rng.normal(0, 1, m), np.exp(x / x[-1] * 8)][seed % 4] + rng.normal(0, 0.05, m)
    w = rng.uniform(0.5, 20, m)
    return x, y, w, k, float(10 ** rng.uniform(-12, 3))


# ------------------------------------------------------------------------------------------------ restatement: the weights
def box_weights(state6, cam, P1, P2):
    """:1186-1196 -> fp64 [n,4] = (x_weight, y_weight, x_diff, y_diff): the state rounded to fp32, fp32 corners
    (homography.py:305-320), fp64 projection with the wrapper's switch on the corner-0 y."""
    state6 = np.asarray(state6, F64).reshape(-1, 6)
    out = np.zeros((len(state6), 4), F64)
    for i, (st, m) in enumerate(zip(state6, cam)):
        x, y, l, w, h, d = (F32(v) for v in st)
        xf = x + d * l
        half = d * w / F32(2.0)
        ylo, yhi = y - half, y + half
        P = (P2 if P2 is not None and ylo > F32(60.0) else P1)[m]
        im = [rc.project(P, F64(cx), F64(cy), F64(0.0)) for cx, cy in ((xf, ylo), (xf, yhi), (x, ylo), (x, yhi))]
        yu = ((im[0][0] - im[1][0]) + (im[2][0] - im[3][0])) / 2.0
        yv = ((im[0][1] - im[1][1]) + (im[2][1] - im[3][1])) / 2.0
        xu = ((im[0][0] - im[2][0]) + (im[1][0] - im[3][0])) / 2.0
        xv = ((im[0][1] - im[2][1]) + (im[1][1] - im[3][1])) / 2.0
        y_diff, x_diff = np.sqrt(yu * yu + yv * yv), np.sqrt(xu * xu + xv * xv)
        out[i] = (x_diff / st[2], y_diff / st[3], x_diff, y_diff)
    return out


def end_weighted(w):
    """:1220-1223 on a copy: ``w[[0, -1]] *= 50; w[[1, -2]] *= 10`` -- an index that occurs twice multiplies once."""
    w = np.array(w, F64)
    m = len(w)
    for i in sorted({0, m - 1}):
        w[i] = w[i] * 50
    for i in sorted({1 % m, (m - 2) % m}):
        w[i] = w[i] * 10
    return w


# ------------------------------------------------------------------------------------------------ restatement: FITPACK
def bspl(t, k, x, l):
    """fpbspl; t is 1-based (t[0] unused) -> h[0 .. k]."""
    h = [0.0] * (k + 2)
    hh = [0.0] * (k + 1)
    h[0] = 1.0
    for j in range(1, k + 1):
        for i in range(j):
            hh[i] = h[i]
        h[0] = 0.0
        for i in range(1, j + 1):
            tli, tlj = t[l + i], t[l + i - j]
            if tli == tlj:
                h[i] = 0.0
            else:
                f = hh[i - 1] / (tli - tlj)
                h[i - 1] = h[i - 1] + f * (tli - x)
                h[i] = f * (x - tlj)
    return h


def value(t, c, n, k, x):
    """splev with extrapolation for one argument; t, c 0-based sequences of length >= n."""
    t1 = [0.0] + [float(v) for v in t[:n]]
    k1, nk1 = k + 1, n - k - 1
    l = k1
    while not (x < t1[l + 1] or l == nk1):
        l += 1
    h = bspl(t1, k, x, l)
    sp = 0.0
    for j in range(1, k1 + 1):
        sp = sp + float(c[l - k1 + j - 1]) * h[j - 1]
    return sp


def givs(piv, ww):
    store = abs(piv)
    if store >= ww:
        r = ww / piv
        dd = store * math.sqrt(1.0 + r * r)
    else:
        r = piv / ww
        dd = ww * math.sqrt(1.0 + r * r)
    return dd, ww / dd, piv / dd


def rota(cs, sn, a, b):
    return cs * a - sn * b, cs * b + sn * a


def fortran_int(v):
    if not (-2147483649.0 < v < 2147483648.0):
        return INT_MIN
    return int(v)


def _residual(T, C, x, y, w, m, k, nk1, FP=None, nrint=0):
    k1, k2 = k + 1, k + 2
    fpart = 0.0
    i, l, lq = 1, k2, k1
    for it in range(1, m + 1):
        xi = x[it - 1]
        new = False
        if not (xi < T[l] or l > nk1):
            new = True
            l += 1
        while not (xi < T[lq + 1] or lq == nk1):
            lq += 1
        h = bspl(T, k, xi, lq)
        term = 0.0
        for j in range(1, k1 + 1):
            term = term + C[l - k2 + j] * h[j - 1]
        d = w[it - 1] * (term - y[it - 1])
        term = d * d
        fpart = fpart + term
        if FP is not None and new:
            store = term * 0.5
            FP[i] = fpart - store
            i += 1
            fpart = store
    if FP is not None:
        FP[nrint] = fpart
    return fpart


def _back(A, Z, n, kb, C):
    """fpback; A[col][i], 1-based rows; writes C (which may be Z)."""
    C[n] = Z[n] / A[0][n]
    i = n - 1
    for j in range(2, n + 1):
        store = Z[i]
        i1 = j - 1 if j <= kb - 1 else kb - 1
        mm = i
        for l in range(1, i1 + 1):
            mm += 1
            store = store - C[mm] * A[l][i]
        C[i] = store / A[0][i]
        i -= 1


def fit(x, y, w, k, s, ncap, trace=None):
    """fpcurf, iopt = 0 -> dict(n, ier, fp, iters, t [n], c [n - k - 1]); x, y, w sequences of floats, x ascending.  ``trace``: a
    list that receives (n, nplus, fp, fpint [nrint]) of every round that adds knots."""
    x, y, w = [float(v) for v in x], [float(v) for v in y], [float(v) for v in w]
    m, s = len(x), float(s)
    k1, k2 = k + 1, k + 2
    nmin, nmax = 2 * k1, m + k1
    nest, nest_full = max(m // 2, 2 * k1), max(nmax, 2 * k + 3)           # UnivariateSpline's first nest, then _reset_nest's
    N = ncap + 2
    T, C, Z, FP, NRD = ([0.0] * (N + 1) for _ in range(5))
    A = [[0.0] * (N + 1) for _ in range(k1)]
    G = [[0.0] * (N + 1) for _ in range(k2)]
    B = [[0.0] * (N + 1) for _ in range(k2)]
    acc, xb, xe = 1e-3 * s, x[0], x[m - 1]
    n, ier, nplus, iters, nk1, nrint = nmin, 0, 0, 0, 0, 0
    fp = fpold = fp0 = fpms = 0.0
    NRD[1] = m - 2
    done, again = False, True
    while again and not done:
        again = False
        for _ in range(1, m + 1):
            iters += 1
            if n == nmin:
                ier = -2
            nrint, nk1 = n - nmin + 1, n - k1
            for j in range(1, k1 + 1):
                T[j] = xb
                T[n + 1 - j] = xe
            fp = 0.0
            for i in range(1, nk1 + 1):
                Z[i] = 0.0
                for j in range(k1):
                    A[j][i] = 0.0
            l = k1
            for it in range(1, m + 1):
                xi, wi = x[it - 1], w[it - 1]
                yi = y[it - 1] * wi
                while not (xi < T[l + 1] or l == nk1):
                    l += 1
                h = bspl(T, k, xi, l)
                for i in range(k1):
                    h[i] = h[i] * wi
                j = l - k1
                for i in range(1, k1 + 1):
                    j += 1
                    piv = h[i - 1]
                    if piv == 0.0:
                        continue
                    A[0][j], cs, sn = givs(piv, A[0][j])
                    yi, Z[j] = rota(cs, sn, yi, Z[j])
                    for i1 in range(i + 1, k1 + 1):
                        h[i1 - 1], A[i1 - i][j] = rota(cs, sn, h[i1 - 1], A[i1 - i][j])
                fp = fp + yi * yi
            if ier == -2:
                fp0 = fp
            FP[n] = fp0
            FP[n - 1] = fpold
            NRD[n] = nplus
            _back(A, Z, nk1, k1, C)
            fpms = fp - s
            if abs(fpms) < acc:
                done = True
                break
            if fpms < 0.0:
                break
            if n == nmax:
                ier, done = -1, True
                break
            if n == nest:
                if nest == nest_full:
                    ier, done = 1, True
                    break
                nest = nest_full                                # ier = 1, _reset_nest, fpcurf with iopt = 1: the same knots and
                if n != nmin:                                   # sums again, but it enters with ier = 1, so nplus starts over
                    ier = 1
            if ier == 0:
                npl1 = nplus * 2
                rn = float(nplus)
                if fpold - fp > acc:
                    npl1 = fortran_int(rn * fpms / (fpold - fp))
                nplus = min(nplus * 2, max(npl1, nplus // 2, 1))
            else:
                nplus, ier = 1, 0
            fpold = fp
            _residual(T, C, x, y, w, m, k, nk1, FP, nrint)
            if trace is not None:
                trace.append((n, nplus, fp, FP[1:nrint + 1], [int(v) for v in NRD[1:nrint + 1]], T[1:n + 1], C[1:nk1 + 1]))
            for _lp in range(nplus):
                if n >= ncap:
                    ier, done = REJECTED, True
                    break
                fpmax, jbegin, number, maxpt, maxbeg = 0.0, 1, 0, 0, 0
                for j in range(1, nrint + 1):
                    jpoint = int(NRD[j])
                    if not (fpmax >= FP[j] or jpoint == 0):
                        fpmax, number, maxpt, maxbeg = FP[j], j, jpoint, jbegin
                    jbegin = jbegin + jpoint + 1
                ihalf = maxpt // 2 + 1
                nrx, nxt = maxbeg + ihalf, number + 1
                if number == 0 or nrx < 1 or nrx > m:
                    ier, done = STUCK, True
                    break
                for j in range(nxt, nrint + 1):
                    jj = nxt + nrint - j
                    FP[jj + 1] = FP[jj]
                    NRD[jj + 1] = NRD[jj]
                    T[jj + k + 1] = T[jj + k]
                NRD[number] = ihalf - 1
                NRD[nxt] = maxpt - ihalf
                am = float(maxpt)
                FP[number] = fpmax * float(ihalf - 1) / am
                FP[nxt] = fpmax * float(maxpt - ihalf) / am
                T[nxt + k] = x[nrx - 1]
                n += 1
                nrint += 1
                if n == nmax:
                    i, j = k2, k // 2 + 2
                    for _q in range(m - k1):
                        T[i] = x[j - 1] if k & 1 else (x[j - 1] + x[j - 2]) * 0.5
                        i += 1
                        j += 1
                    again = True
                    break
                if n == nest:
                    break
            if done or again:
                break
    if not done and ier != -2:
        n8 = n - nmin
        fac = float(nk1 - k) / (T[nk1 + 1] - T[k1])
        for l in range(k2, nk1 + 1):
            lmk = l - k1
            h = [0.0] * (2 * k1)
            for j in range(1, k1 + 1):
                h[j - 1] = T[l] - T[l + j - k2]
                h[j + k1 - 1] = T[l] - T[l + j]
            lp = lmk
            for j in range(1, k2 + 1):
                prod = h[j - 1]
                for i in range(1, k + 1):
                    prod = prod * h[j + i - 1] * fac
                B[j - 1][lmk] = (T[lp + k1] - T[lp]) / prod
                lp += 1
        p1, f1, p3, f3, p = 0.0, fp0 - s, -1.0, fpms, 0.0
        for i in range(1, nk1 + 1):
            p = p + A[0][i]
        p = float(nk1) / p
        ich1 = ich3 = 0
        con1, con9, con4 = 0.1, 0.9, 0.04
        ier = 3
        for it_p in range(1, MAXIT + 1):
            iters += 1
            pinv = 1.0 / p
            for i in range(1, nk1 + 1):
                C[i] = Z[i]
                G[k1][i] = 0.0
                for j in range(k1):
                    G[j][i] = A[j][i]
            for it in range(1, n8 + 1):
                h = [B[i][it] * pinv for i in range(k2)] + [0.0]
                yi = 0.0
                for j in range(it, nk1 + 1):
                    piv = h[0]
                    G[0][j], cs, sn = givs(piv, G[0][j])
                    yi, C[j] = rota(cs, sn, yi, C[j])
                    if j == nk1:
                        break
                    i2 = nk1 - j if j > n8 else k1
                    for i in range(1, i2 + 1):
                        h[i], G[i][j] = rota(cs, sn, h[i], G[i][j])
                        h[i - 1] = h[i]
                    h[i2] = 0.0
            _back(G, C, nk1, k2, C)
            fp = _residual(T, C, x, y, w, m, k, nk1)
            fpms = fp - s
            if abs(fpms) < acc:
                ier = 0
                break
            if it_p == MAXIT:
                break
            p2, f2 = p, fpms
            if ich3 == 0:
                if not (f2 - f3 > acc):
                    p3, f3 = p2, f2
                    p = p * con4
                    if p <= p1:
                        p = p1 * con9 + p2 * con1
                    continue
                if f2 < 0.0:
                    ich3 = 1
            if ich1 == 0:
                if not (f1 - f2 > acc):
                    p1, f1 = p2, f2
                    p = p / con4
                    if p3 < 0.0:
                        continue
                    if p >= p3:
                        p = p2 * con1 + p3 * con9
                    continue
                if f2 > 0.0:
                    ich1 = 1
            if f2 >= f1 or f2 <= f3:
                ier = 2
                break
            if p3 > 0.0:
                h1, h2, h3 = f1 * (f2 - f3), f2 * (f3 - f1), f3 * (f1 - f2)
                p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3)
            else:
                p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3)
            if f2 < 0.0:
                p3, f3 = p2, f2
            else:
                p1, f1 = p2, f2
    return dict(n=n, ier=ier, fp=fp, iters=iters, t=np.array(T[1:n + 1], F64), c=np.array(C[1:n - k], F64))


# ------------------------------------------------------------------------------------------------ restatement: selection
def score(t, c, n, k, x, y, w2, metric, axis):
    """The candidate's score (NaN: skipped by :1238) with the sum in ascending row order."""
    if math.isnan(value(t, c, n, k, 0.0)):
        return float("nan")
    total, mx = 0.0, -math.inf
    for xi, yi, wi in zip(x, y, w2):
        d = float(wi) * (value(t, c, n, k, float(xi)) - float(yi))
        e = d * d
        total = total + e
        if e > mx or math.isnan(e):
            mx = e
        if math.isnan(mx):
            return float("nan")
    if metric == "ape":
        return math.sqrt(total / len(x))
    return math.sqrt(mx) if axis == 0 else mx


def first_smallest(scores):
    best, idx = math.inf, -1
    for i, v in enumerate(scores):
        if v < best:
            best, idx = v, i
    return idx


def figures(t, c, n, k, x, y, w):
    """:1282-1294 of one axis -> (sqrt(mean r^2), sqrt(mean (w r)^2), sqrt(max (w r)^2))."""
    se, pe, mx = 0.0, 0.0, -math.inf
    for xi, yi, wi in zip(x, y, w):
        r = value(t, c, n, k, float(xi)) - float(yi)
        d = float(wi) * r
        e = d * d
        se = se + r * r
        pe = pe + e
        if e > mx or math.isnan(e):
            mx = e
    m = len(x)
    return math.sqrt(se / m), math.sqrt(pe / m), math.sqrt(mx)


def ncap_of(limit, k, m):
    """The n at which a lane stops: the reference's knot limit + 2k, at most m + k + 1."""
    return int(min(limit + 2 * k, m + k + 1))


def select(x, y, w, w2, k, svals, limit, metric, axis):
    """All candidates of one (object, axis) -> dict(fits, scores, win, figs)."""
    ncap = ncap_of(limit, k, len(x))
    fits = [fit(x, y, w, k, s, ncap) for s in svals]
    scores = [score(f["t"], f["c"], f["n"], k, x, y, w2, metric, axis) if f["ier"] <= 3 else float("nan") for f in fits]
    win = first_smallest(scores)
    figs = None
    if win >= 0:
        f = fits[win]
        figs = figures(f["t"], f["c"], f["n"], k, x, y, w)
    return dict(fits=fits, scores=scores, win=win, figs=figs, ncap=ncap)


# ------------------------------------------------------------------------------------------------ restatement: the passes
def compile_boxes(me, idx):
    """:1159-1174: the object's boxes frame-major up to last_frame, cameras in seq_keys order -> (boxes, camera names)."""
    boxes, cams = [], []
    for f_idx, frame in enumerate(me.data):
        if f_idx > me.last_frame:
            break
        for cam in me.seq_keys:
            box = frame.get("{}_{}".format(cam, idx))
            if box is not None:
                boxes.append(box)
                cams.append(cam)
    return boxes, cams


def object_rows(me, idx):
    """-> None (no boxes) or dict(t, x, y, xw, yw, duration), sorted by timestamp (stable)."""
    boxes, cams = compile_boxes(me, idx)
    if not boxes:
        return None
    names = [c.name for c in me.cameras]
    state = np.array([[float(b[k]) for k in STATE_KEYS] for b in boxes], F64)
    ts = np.array([float(b["timestamp"]) for b in boxes], F64)
    P1, P2 = rc.tables(me.hg, names)
    wts = box_weights(state, [names.index(c) for c in cams], P1, P2)
    order = np.argsort(ts, kind="stable")
    return dict(t=ts[order], x=state[order, 0], y=state[order, 1], xw=wts[order, 0], yw=wts[order, 1],
                duration=float(ts.max() - ts.min()))


def ref_create_trajectory(me, idx, y_order=2, x_order=3, metric="ape", complexity=4, tpex=None, tpey=None):
    """-> dict(t, x, y: (t, c, n, k, ier, fp) or None, figs..., sel_x, sel_y) or None where the reference returns Nones."""
    rows = object_rows(me, idx)
    if rows is None or rows["duration"] < 3:
        return None
    tpex = tpe_x() if tpex is None else tpex
    tpey = tpe_y() if tpey is None else tpey
    m = len(rows["t"])
    dur = math.floor(rows["duration"])
    sx = [smoothing(v, m) for v in tpex]
    sy = [smoothing(v, m) for v in tpey]
    sel_x = select(rows["t"], rows["x"], rows["xw"], end_weighted(rows["xw"]), x_order, sx, dur * complexity + 2, metric, 0)
    sel_y = select(rows["t"], rows["y"], rows["yw"], rows["yw"], y_order, sy, dur + 2, metric, 1)
    out = dict(rows=rows, sel_x=sel_x, sel_y=sel_y, x=None, y=None)
    if sel_x["win"] >= 0 and sel_y["win"] >= 0:
        for key, sel, k in (("x", sel_x, x_order), ("y", sel_y, y_order)):
            f = sel["fits"][sel["win"]]
            out[key] = dict(t=f["t"], c=f["c"], n=f["n"], k=k, ier=f["ier"], fp=f["fp"])
    return out


def ref_get_splines(me, metric="mpe", tpex=None, tpey=None):
    """-> (splines: [[x, y]] of dicts or None, ases, apes)."""
    splines, ases, apes = [], [], []
    for idx in range(lc.unused_id(me.data)):
        got = ref_create_trajectory(me, idx, metric=metric, tpex=tpex, tpey=tpey)
        if got is None or got["x"] is None:
            splines.append([None, None])
            continue
        splines.append([got["x"], got["y"]])
        ases.append(got["sel_x"]["figs"][0])
        apes.append(got["sel_x"]["figs"][1])
    return splines, ases, apes


def spline_value(sp, x):
    return value(sp["t"], sp["c"], sp["n"], sp["k"], float(x))


def ref_gen_trajectories(me, splines):
    """:1317-1336 -> a deep copy of me.data with x, y from the splines."""
    data = copy.deepcopy(me.data)
    for idx, (xs, ys) in enumerate(splines):
        if xs is None:
            continue
        for frame in data:
            for cam in me.seq_keys:
                box = frame.get("{}_{}".format(cam, idx))
                if box is not None:
                    box["x"] = spline_value(xs, box["timestamp"])
                    box["y"] = spline_value(ys, box["timestamp"])
    return data


def ts_shift_entry(kept, xlabel, ts, run, shifts, use_run, metric):
    """One (frame, camera) of :1416-1442 -> (best_time, best_error, init_error, best index)."""
    def err(time, how):
        total, mx = 0.0, -math.inf
        for sp, xl in zip(kept, xlabel):
            d = float(F32(spline_value(sp, time))) - float(xl)
            q = d * d
            total = total + q
            if q > mx or math.isnan(q):
                mx = q
        return math.sqrt(total / len(kept)) if how == "ape" else math.sqrt(mx)
    init = err(ts, "ape")
    best, best_i, best_t = math.inf, -1, ts
    for j, sh in enumerate(shifts):
        t = ts + float(sh)
        if use_run:
            t = t + run
        e = err(t, metric)
        if e < best:
            best, best_i, best_t = e, j, t
    return best_t, best, init, best_i


def ref_adjust_ts(me, splines, max_shift=0.01, trials=21, overwrite_ts_data=False, metric="ape", use_running_error=True):
    """:1353-1458 -> [(frame, camera index, best_time, best_error, init_error, best index)]; rewrites me.data (and all_ts)."""
    shifts = np.linspace(-max_shift, max_shift, trials)
    running = [float(me.ts_bias[i]) for i in range(len(me.seq_keys))]
    n_ids = lc.unused_id(me.data)
    out = []
    for f_idx, frame in enumerate(me.data):
        if f_idx > me.last_frame or len(frame) == 0:
            break
        for c_idx, cam in enumerate(me.seq_keys):
            ids = [i for i in range(n_ids) if frame.get("{}_{}".format(cam, i)) is not None]
            kept = [i for i in ids if splines[i][0] is not None]
            if not kept:
                continue
            ts = me.all_ts[f_idx][cam]
            got = ts_shift_entry([splines[i][0] for i in kept], [frame["{}_{}".format(cam, i)]["x"] for i in kept], float(ts),
                                 running[c_idx], shifts, use_running_error, metric)
            out.append((f_idx, c_idx) + got)
            for i in ids:
                frame["{}_{}".format(cam, i)]["timestamp"] = got[0]
            if overwrite_ts_data:
                me.all_ts[f_idx][cam] = got[0]
            if use_running_error:
                running[c_idx] += shifts[-1]
    return out


def ref_adjust_boxes(me, splines, max_shift_x=2, max_shift_y=2):
    """manual_annotator_state_v3.py:1440-1515 -> pixel_shifts; moves x and y of every box of frames <= last_frame towards its
    object's splines by at most l / x_diff * max_shift_x (w / y_diff * max_shift_y), in the frames' own dict order."""
    names = [c.name for c in me.cameras]
    P1, P2 = rc.tables(me.hg, names)
    shifts = []
    for f_idx, frame in enumerate(me.data):
        if f_idx > me.last_frame:
            break
        if len(frame) == 0:
            continue
        items = list(frame.values())
        state = np.array([[float(b[k]) for k in STATE_KEYS] for b in items], F64)
        ts = [float(b["timestamp"]) for b in items]
        wts = box_weights(state, [names.index(b["camera"]) for b in items], P1, P2)
        y_lim = state[:, 3] / wts[:, 3] * max_shift_y
        x_lim = state[:, 2] / wts[:, 2] * max_shift_x
        for i, box in enumerate(items):
            xs, ys = splines[box["id"]]
            if xs is not None:
                x_diff = F64(spline_value(xs, ts[i])) - state[i, 0]
                if x_diff < -x_lim[i]:
                    x_diff = -x_lim[i]
                elif x_diff > x_lim[i]:
                    x_diff = x_lim[i]
                box["x"] += x_diff
            if ys is not None:
                y_diff = F64(spline_value(ys, ts[i])) - state[i, 1]
                if y_diff < -y_lim[i]:
                    y_diff = -y_lim[i]
                elif y_diff > y_lim[i]:
                    y_diff = y_lim[i]
                box["y"] += y_diff
                shifts.append(np.sqrt(x_diff ** 2 + y_diff ** 2))
    return shifts


def dump_xyt(data, names):
    """Every datum of ``data`` in (frame, camera, id) order -> (idx int64 [n,3], val fp64 [n,3] = x, y, timestamp)."""
    idx, val = [], []
    for f, frame in enumerate(data):
        rows = sorted((names.index(d["camera"]), d["id"], d) for d in frame.values())
        for c, i, d in rows:
            idx.append((f, c, i))
            val.append((d["x"], d["y"], d["timestamp"]))
    return np.array(idx, np.int64).reshape(-1, 3), np.array(val, F64).reshape(-1, 3)

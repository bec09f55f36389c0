"""Camera calibration (homography.py:96-154, 336-371, 554-666): a CPU restatement in numpy of the four kernels of
csrc/calibrate.hip, operation by operation, and the case tables the host and GPU tests share.

Every sum is written out in the order the kernels use, and ``np.arange`` / ``np.linspace`` are restated by their formulas
(tests/test_calibration_host.py holds the formulas against numpy itself):

  arange(start, stop, g):  n = ceil((stop - start) / g);  a[0] = start, a[1] = start + g,
                           a[i] = start + i * delta  with  delta = a[1] - a[0]        (numpy's fill, not i * g)
  linspace(lo, hi, 10):    step = (hi - lo) / 9;  y[i] = i * step + lo;  y[9] = hi

Order of the reprojection means (rn_hg_reproj_error, rn_hg_scale_z): per box the four corner distances are added in corner
order, ((e0 + e1) + e2) + e3; box b goes to partial[b % 256], partials take their boxes in ascending b starting from 0.0;
the 256 partials fold pairwise, partial[t] += partial[t + s] for s = 128, 64, ..., 1; the mean is partial[0] / (4 d).
"""
import math

import numpy as np

VP_LEVELS = 16
VP_MAX_AXIS = 32
VP_FEW_LINES, VP_BAD_START, VP_LONG_AXIS = 1, 2, 4          # status bits of rn_vanishing_points
SZ_MAX_ITERS = 64
SZ_BAD_FIRST_STEP, SZ_NO_WINNER, SZ_TOO_MANY = 1, 2, 4      # status bits of rn_hg_scale_z
FIT_FEW_POINTS, FIT_DEGENERATE, FIT_NOT_FINITE = 1, 2, 4    # status bits of rn_fit_homography
FIT_SWEEPS = 12
FIT_GN_STEPS = 10
BLOCK = 256


# ------------------------------------------------------------------------------------------------ numpy's rules
def arange_axis(p, g):
    """np.arange(p - g*15, p + g*15, g) -> (values, (start, stop))."""
    start = p - g * 15.0
    stop = p + g * 15.0
    q = (stop - start) / g
    if not math.isfinite(q):
        raise ValueError("arange: cannot compute length")
    n = max(int(math.ceil(q)), 0)
    out = np.empty(n, np.float64)
    if n > 0:
        out[0] = start
    if n > 1:
        out[1] = start + g
        delta = out[1] - out[0]
        for i in range(2, n):
            out[i] = start + float(i) * delta
    return out, (start, stop)


def linspace10(lo, hi):
    step = (hi - lo) / 9.0
    y = np.array([float(i) * step + lo for i in range(10)], np.float64)
    y[9] = hi
    return y


# ------------------------------------------------------------------------------------------------ vanishing points
def vp_start(lines):
    """homography.py:113-122 as written (the precedence slips are the reference's)."""
    l0, l1 = np.asarray(lines[0], np.float64), np.asarray(lines[1], np.float64)
    with np.errstate(all="ignore"):
        a = (l0[3] - l0[1]) / l0[2] - l0[0]
        b = (l1[3] - l1[1]) / l1[2] - l1[0]
        c = l0[1] - a * l0[0]
        d = l1[1] - c * l1[0]
        px = (d - c) / (a - b)
        py = a * (d - c) / (a - b) + c
    return float(px), float(py)


def vanishing_point(lines):
    """find_vanishing_point (homography.py:96-154) -> dict(point [2], best, trace [16,3] = (px, py, best) each level
    STARTED with, bounds [16,2,3] = (start, stop, length) of the x and y axis, status)."""
    lines = np.asarray(lines, np.float64).reshape(-1, 4)
    if len(lines) < 2:
        raise IndexError("list index out of range")
    px, py = vp_start(lines)
    trace = np.zeros((VP_LEVELS, 3))
    bounds = np.zeros((VP_LEVELS, 2, 3))
    best = np.inf
    status = 0
    if not (math.isfinite(px) and math.isfinite(py)):
        return dict(point=np.array([px, py]), best=best, trace=trace, bounds=bounds, status=VP_BAD_START)
    g = 1e16
    with np.errstate(all="ignore"):
        for lvl in range(VP_LEVELS):
            assert g > 1
            trace[lvl] = (px, py, best)
            xs, bx = arange_axis(px, g)
            ys, by = arange_axis(py, g)
            bounds[lvl, 0] = (bx[0], bx[1], len(xs))
            bounds[lvl, 1] = (by[0], by[1], len(ys))
            if len(xs) > VP_MAX_AXIS or len(ys) > VP_MAX_AXIS:
                status |= VP_LONG_AXIS
                xs, ys = xs[:VP_MAX_AXIS], ys[:VP_MAX_AXIS]
            if len(xs) and len(ys):
                X = np.repeat(xs, len(ys))                       # x outer, y inner
                Y = np.tile(ys, len(xs))
                dist = np.zeros(len(X))
                for ln in lines:
                    dx, dy = ln[2] - ln[0], ln[3] - ln[1]
                    num = np.abs(dx * (ln[1] - Y) - dy * (ln[0] - X))
                    q = num / (np.sqrt(dx * dx + dy * dy) + 1e-08)
                    dist = dist + q * q
                k = int(np.argmin(np.where(np.isnan(dist), np.inf, dist)))      # the first of equal minima
                if dist[k] < best:
                    px, py, best = float(X[k]), float(Y[k]), float(dist[k])
            g = g / 10.0
    assert g == 1.0
    return dict(point=np.array([px, py]), best=best, trace=trace, bounds=bounds, status=status)


# ------------------------------------------------------------------------------------------------ reprojection error
def _fold(per_box):
    part = np.zeros(BLOCK)
    for b, v in enumerate(per_box):
        part[b % BLOCK] = part[b % BLOCK] + v
    s = BLOCK // 2
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def reproj_error(boxes, heights, H, P):
    """test_transformation's arithmetic (homography.py:581-587) -> (top, bottom) fp64."""
    b = np.asarray(boxes, np.float64)
    d = b.shape[0]
    H = np.asarray(H, np.float64)
    P = np.asarray(P, np.float64)
    hd = np.asarray(heights, np.float32).astype(np.float64)
    f32 = np.float32
    with np.errstate(all="ignore"):
        bx, by = b[:, :, 0], b[:, :, 1]
        u = (H[0, 0] * bx + H[0, 1] * by) + H[0, 2]
        v = (H[1, 0] * bx + H[1, 1] * by) + H[1, 2]
        w = (H[2, 0] * bx + H[2, 1] * by) + H[2, 2]
        x, y = u / w, v / w
        z = np.zeros((d, 8))
        z[:, 4:] = hd[:, None]
        fx, rx = x[:, 0] + x[:, 1], x[:, 2] + x[:, 3]
        st = np.zeros((d, 6), f32)
        st[:, 0] = (rx / 2.0).astype(f32)
        st[:, 1] = ((((y[:, 0] + y[:, 1]) + y[:, 2]) + y[:, 3]) / 4.0).astype(f32)
        dl = (fx - rx) / 2.0
        st[:, 2] = np.abs(dl).astype(f32)
        dw = ((y[:, 0] + y[:, 2]) - (y[:, 1] + y[:, 3])) / 2.0
        st[:, 3] = np.abs(dw).astype(f32)
        hs = np.zeros(d)
        for k in range(4):
            hs = hs + np.abs(z[:, k] - z[:, k + 4])
        st[:, 4] = (hs / 4.0).astype(f32)
        st[:, 5] = np.sign(dl).astype(f32)
        xr, yc, ln, wd, h, dr = (st[:, k] for k in range(6))
        xf = xr + dr * ln
        half = dr * wd / f32(2.0)
        cx = np.stack([xf, xf, xr, xr, xf, xf, xr, xr], 1).astype(np.float64)
        ylo, yhi = yc - half, yc + half
        cy = np.stack([ylo, yhi] * 4, 1).astype(np.float64)
        zero = np.zeros(d, f32)
        cz = np.stack([zero] * 4 + [-h] * 4, 1).astype(np.float64)
        pu = ((P[0, 0] * cx + P[0, 1] * cy) + P[0, 2] * cz) + P[0, 3]
        pv = ((P[1, 0] * cx + P[1, 1] * cy) + P[1, 2] * cz) + P[1, 3]
        pw = ((P[2, 0] * cx + P[2, 1] * cy) + P[2, 2] * cz) + P[2, 3]
        ex, ey = np.abs(bx - pu / pw), np.abs(by - pv / pw)
        e = np.sqrt(ex * ex + ey * ey)
        bot = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]
        top = ((e[:, 4] + e[:, 5]) + e[:, 6]) + e[:, 7]
        n = float(4 * d)
        return _fold(top) / n, _fold(bot) / n


def scaled_P(P_orig, C):
    P = np.array(P_orig, np.float64)
    P[:, 2] = P[:, 2] * C
    return P


def reproj_errors(boxes, heights, H, P_orig, Cs):
    """-> [K,2] (top, bottom) for P[:,2] = P_orig[:,2] * C."""
    return np.array([reproj_error(boxes, heights, H, scaled_P(P_orig, float(C))) for C in Cs]).reshape(-1, 2)


def scale_z(boxes, heights, H, P_orig, granularity=1e-06, max_scale=10.0):
    """scale_Z (homography.py:607-666) -> dict(trace [iters,10,2] = (C, error), iters, last_C, best_C, best_error, status)."""
    grid = linspace10(granularity, max_scale)
    step = grid[1] - grid[0]
    trace = []
    best_C, best_err, last_C, status = math.nan, math.inf, math.nan, 0
    if not step > granularity:
        status |= SZ_BAD_FIRST_STEP
    while step > granularity:
        if len(trace) == SZ_MAX_ITERS:
            status |= SZ_TOO_MANY
            break
        best_err, bi = math.inf, -1
        row = []
        for i, C in enumerate(grid):
            top, bot = reproj_error(boxes, heights, H, scaled_P(P_orig, float(C)))
            err = top + bot
            row.append((float(C), err))
            if err < best_err:
                best_err, bi = err, i
        trace.append(row)
        last_C = float(grid[9])
        if bi < 0:
            status |= SZ_NO_WINNER
            break
        best_C = float(grid[bi])
        grid = linspace10(best_C - step, best_C + step)
        step = grid[1] - grid[0]
    return dict(trace=np.array(trace, np.float64).reshape(-1, 10, 2), iters=len(trace), last_C=last_C, best_C=best_C,
                best_error=best_err, status=status)


# ------------------------------------------------------------------------------------------------ homography fit
def _hartley(p):
    n = len(p)
    mx = my = 0.0
    for x, y in p:
        mx, my = mx + x, my + y
    mx, my = mx / n, my / n
    md = 0.0
    for x, y in p:
        md = md + math.sqrt((x - mx) * (x - mx) + (y - my) * (y - my))
    md = md / n
    s = math.sqrt(2.0) / md if md > 0 else math.inf
    return mx, my, s


def _jacobi(A):
    """Cyclic Jacobi on a symmetric 9x9, FIT_SWEEPS sweeps -> (eigenvalues, eigenvector columns)."""
    A = A.copy()
    n = A.shape[0]
    V = np.eye(n)
    for _ in range(FIT_SWEEPS):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    akp, akq = A[k, p], A[k, q]
                    A[k, p], A[k, q] = c * akp - s * akq, s * akp + c * akq
                for k in range(n):
                    apk, aqk = A[p, k], A[q, k]
                    A[p, k], A[q, k] = c * apk - s * aqk, s * apk + c * aqk
                for k in range(n):
                    vkp, vkq = V[k, p], V[k, q]
                    V[k, p], V[k, q] = c * vkp - s * vkq, s * vkp + c * vkq
    return np.diag(A).copy(), V


def _solve8(M, r):
    """Gaussian elimination with partial pivoting; None if a pivot is zero or not finite."""
    n = len(r)
    M, r = M.copy(), r.copy()
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if not (abs(M[p, c]) > 0 and math.isfinite(M[p, c])):
            return None
        if p != c:
            M[[c, p]], r[[c, p]] = M[[p, c]], r[[p, c]]
        for k in range(c + 1, n):
            f = M[k, c] / M[c, c]
            M[k, c:] = M[k, c:] - f * M[c, c:]
            r[k] = r[k] - f * r[c]
    x = np.zeros(n)
    for c in range(n - 1, -1, -1):
        acc = r[c]
        for k in range(c + 1, n):
            acc = acc - M[c, k] * x[k]
        x[c] = acc / M[c, c]
    return x


def _transfer_cost(h, s, t):
    w = h[6] * s[:, 0] + h[7] * s[:, 1] + 1.0
    ru = (h[0] * s[:, 0] + h[1] * s[:, 1] + h[2]) / w - t[:, 0]
    rv = (h[3] * s[:, 0] + h[4] * s[:, 1] + h[5]) / w - t[:, 1]
    c = 0.0
    for a, b in zip(ru, rv):
        c = c + (a * a + b * b)
    return c


def fit_homography(src, dst, refine=True):
    """The plane homography dst ~ H [src; 1] (stands in for cv2.findHomography(src, dst), method 0; parity with cv2 is
    unpinned) -> (H [3,3] with H[2,2] = 1, status).  Hartley-normalised DLT on the 9x9 normal matrix, cyclic Jacobi,
    and for n > 4 FIT_GN_STEPS damped Gauss-Newton steps on the forward transfer error in the normalised frame."""
    src, dst = np.asarray(src, np.float64).reshape(-1, 2), np.asarray(dst, np.float64).reshape(-1, 2)
    n = len(src)
    bad = np.full((3, 3), np.nan)
    if n < 4 or len(dst) != n:
        return bad, FIT_FEW_POINTS
    with np.errstate(all="ignore"):
        sx, sy, ss = _hartley(src)
        tx, ty, ts = _hartley(dst)
        if not (math.isfinite(ss) and math.isfinite(ts)):
            return bad, FIT_DEGENERATE
        s = np.stack(((src[:, 0] - sx) * ss, (src[:, 1] - sy) * ss), 1)
        t = np.stack(((dst[:, 0] - tx) * ts, (dst[:, 1] - ty) * ts), 1)
        N = np.zeros((9, 9))
        for (x, y), (u, v) in zip(s, t):
            for r in (np.array([-x, -y, -1.0, 0, 0, 0, u * x, u * y, u]), np.array([0, 0, 0, -x, -y, -1.0, v * x, v * y, v])):
                N = N + r[:, None] * r[None, :]
        lam, V = _jacobi(N)
        order = np.argsort(lam, kind="stable")
        if not np.isfinite(lam).all() or not lam[order[1]] > 1e-12 * lam[order[8]]:
            return bad, FIT_DEGENERATE                  # a second null direction: collinear or repeated points
        h = V[:, order[0]].copy()
        if h[8] == 0 or not np.isfinite(h).all():
            return bad, FIT_NOT_FINITE
        h = h / h[8]
        if refine and n > 4:
            lm = 1e-3
            cost = _transfer_cost(h, s, t)
            for _ in range(FIT_GN_STEPS):
                JtJ, Jtr = np.zeros((8, 8)), np.zeros(8)
                for (x, y), (u, v) in zip(s, t):
                    w = h[6] * x + h[7] * y + 1.0
                    pu, pv = (h[0] * x + h[1] * y + h[2]) / w, (h[3] * x + h[4] * y + h[5]) / w
                    ju = np.array([x / w, y / w, 1.0 / w, 0, 0, 0, -pu * x / w, -pu * y / w])
                    jv = np.array([0, 0, 0, x / w, y / w, 1.0 / w, -pv * x / w, -pv * y / w])
                    JtJ = JtJ + ju[:, None] * ju[None, :]
                    JtJ = JtJ + jv[:, None] * jv[None, :]
                    Jtr = Jtr + ju * (pu - u)
                    Jtr = Jtr + jv * (pv - v)
                M = JtJ + lm * np.diag(np.diag(JtJ))
                delta = _solve8(M, -Jtr)
                if delta is None:
                    lm = lm * 10.0
                    continue
                trial = h.copy()
                trial[:8] = h[:8] + delta
                c2 = _transfer_cost(trial, s, t)
                if c2 < cost:
                    h, cost, lm = trial, c2, lm * 0.1
                else:
                    lm = lm * 10.0
        Hn = h.reshape(3, 3)
        Ts = np.array([[ss, 0, -ss * sx], [0, ss, -ss * sy], [0, 0, 1.0]])
        Ti = np.array([[1.0 / ts, 0, tx], [0, 1.0 / ts, ty], [0, 0, 1.0]])
        Hm = Ti @ Hn @ Ts
        if Hm[2, 2] == 0 or not np.isfinite(Hm).all():
            return bad, FIT_NOT_FINITE
        Hm = Hm / Hm[2, 2]
        if not np.isfinite(Hm).all():
            return bad, FIT_NOT_FINITE
    return Hm, 0


def transfer_rms(H, src, dst):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    p = np.concatenate((src, np.ones((len(src), 1))), 1) @ np.asarray(H, np.float64).T
    return float(np.sqrt((((p[:, :2] / p[:, 2:3]) - dst) ** 2).sum(1).mean()))


# ------------------------------------------------------------------------------------------------ case tables
# A start whose first level (g = 1e16) has a 31-point x axis, found by a search over px = 4.5e17 + 64 k: there px has a
# 64 ulp but px + 1.5e17 a 128 ulp, so for odd k the stop is a tie and rounds to even -- up by 64 for k = 3 -- and
# (stop - start) / 1e16 comes to 30.000000000000004 (tests/test_calibration_host.py checks the length against numpy).
VP31_START = 4.5e17 + 192.0


def lines_for_start(px, py=0.0):
    """Two lines whose start point (homography.py:113-122) is exactly (px, 0): line0 = (0, 0, 1, 0) gives a = 0, c = 0;
    line1 = (1, px, 2, px) gives b = 0 / 2 - 1 = -1 and d = px, so the start is (px / 1, 0).  Both are horizontal, so
    the distance does not depend on x and every x of a grid ties: the lowest scan index has to win."""
    assert py == 0.0
    return np.array([[0.0, 0.0, 1.0, 0.0], [1.0, px, 2.0, px]])


def converging_lines(n, vp, seed, noise=0.3):
    """n image lines through vp (+ noise px on each end point), portable generators."""
    from retinanet_mi355x import synth
    u = synth.uniform((n, 3), seed).astype(np.float64)
    e = synth.normal((n, 4), seed + 1, std=noise).astype(np.float64)
    a = np.stack((200 + 1500 * u[:, 0], 300 + 700 * u[:, 1]), 1)
    t = 0.15 + 0.3 * u[:, 2:3]
    b = a + t * (np.asarray(vp, np.float64)[None] - a)
    return np.concatenate((a, b), 1) + e


VP_SETS = {                     # name -> (number of lines, vanishing point, seed); the golden holds those marked True
    "n2": (2, (2400.0, -350.0), 101, True),
    "n3": (3, (-900.0, 120.0), 103, True),
    "n8": (8, (1013.0, -2210.0), 105, True),
    "n65": (65, (3100.0, 400.0), 107, False),
}


def vp_lines(name):
    if name in VP_SETS:
        n, vp, seed, _ = VP_SETS[name]
        return converging_lines(n, vp, seed)
    if name == "axis31":
        return lines_for_start(VP31_START)
    if name == "empty":                         # start so large that start == stop at every level: all grids are empty
        return lines_for_start(1e40)
    if name == "nan":                           # a third line whose cross term is inf - inf far from the point
        return np.concatenate((converging_lines(2, (2400.0, -350.0), 109), [[0.0, 0.0, 1e300, 1e300]]), 0)
    raise KeyError(name)


VP_GOLDEN = ("n2", "n3", "n8", "axis31", "empty", "nan")
VP_ALL = VP_GOLDEN + ("n65",)

SZ_D = (1, 3, 17, 65, 300)


def sz_case(d, P_true, H):
    """Boxes of d vehicles seen through (H, P_true) with pixel noise, their heights, and the P add_correspondence would
    build (third column = (vp_z, 1) * 0.01, homography.py:370)."""
    from retinanet_mi355x import synth
    st = synth.vehicle_states(d, seed=300 + d).numpy()
    st[:, 1] = np.where(st[:, 1] > 60, st[:, 1] - 60, st[:, 1])
    heights = st[:, 4].copy()
    P_true = np.asarray(P_true, np.float64)
    P0 = P_true.copy()
    P0[:, 2] = np.array([P_true[0, 2] / P_true[2, 2], P_true[1, 2] / P_true[2, 2], 1.0]) * 0.01
    return st, heights, P0


def fit_case(n, H_true, seed, noise=0.0):
    """n image points (not collinear) and their road-plane positions through H_true (+ noise px on the image side)."""
    from retinanet_mi355x import synth
    u = synth.uniform((n, 2), seed).astype(np.float64)
    im = np.stack((150 + 1600 * u[:, 0], 250 + 750 * u[:, 1]), 1)
    if n == 4:
        im = np.array([[200.0, 300.0], [1700.0, 350.0], [1500.0, 950.0], [300.0, 900.0]])
    p = np.concatenate((im, np.ones((n, 1))), 1) @ np.asarray(H_true, np.float64).T
    sp = p[:, :2] / p[:, 2:3]
    if noise:
        im = im + synth.normal((n, 2), seed + 1, std=noise).astype(np.float64)
    return im, sp


FIT_N = (4, 5, 12, 65)

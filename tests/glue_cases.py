"""Cases, float64 references and error bounds for the per-step glue kernels: csrc/elementwise.hip, csrc/elementwise_bf16.hip, the weight
transforms rn_wino_weights / rn_wino_dw of csrc/conv_wino.hip and csrc/optim.hip.  CPU only (numpy): tests/test_glue_cases_host.py proves
what is here against torch's float64 functions and shows that every comparison rejects a wrong answer; tests/test_gpu_glue.py holds the
kernels to it.

Bounds.  u = 2^-24 (fp32 unit roundoff), u_b = 2^-8 (bf16).  Every bound is per element, against the float64 reference r, and has the form
(number of fp32 roundings on the longest path to that element) * u * (sum of the magnitudes of the terms): the standard gamma_n bound, times
1.01 for n u / (1 - n u).  A constant such as 1.f / 6.f that the reference holds exactly counts as one rounding.  Contraction into FMAs only
removes roundings; sqrtf and division are correctly rounded.  Each count is stated beside its bound and comes from the kernel's source.
Where a bound is 0 (padding, masked elements, elements no window names) the result must be exactly zero.

Layouts are the C ABI's: activations NHWC, packed weights [rows][taps][c_pad] padded to a multiple of 32, U / dU [36][rows][Kpad]."""
import collections

import numpy as np

from retinanet_mi355x import synth

U = 2.0 ** -24
UB = 2.0 ** -8
SLACK = 1.01


def nu(n):
    """n roundings."""
    return SLACK * n * U


# ---------------------------------------------------------------------------------------------- comparisons
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    """Bit for bit: -0.0 is not +0.0, a NaN equals the same NaN."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.array_equal(bits(got), bits(want)))


def same_values(got, want):
    """As values: -0.0 equals 0.0, a NaN equals nothing."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all(got == want))


def worst(got, ref, bound):
    """Largest |got - ref| / bound over the elements.  An exact element counts 0 whatever its bound; an error against a zero bound, a NaN
    or an infinity in `got` counts inf."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref)
        frac = np.where(err == 0, 0.0, err / bound)
    frac = np.where(np.isfinite(got) & ~np.isnan(frac), frac, np.inf)
    return float(frac.max())


def within(got, ref, bound):
    return worst(got, ref, bound) <= 1.0


def bf16_rne(x):
    """fp32 -> bf16 bits (uint16), round to nearest even: what a (__bf16) conversion does to a finite value or an infinity."""
    b = bits(np.asarray(x, dtype=np.float32)).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_trunc(x):
    """The wrong conversion: the low 16 bits dropped."""
    return (bits(np.asarray(x, dtype=np.float32)) >> 16).astype(np.uint16)


def bf16_value(b):
    """bf16 bits -> the fp32 value they stand for."""
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_rne(x))


def kpad(taps, c):
    return (taps * c + 31) // 32 * 32


def s2_classes(k, pad):
    """conv.s2_classes' tap subsets (r0, nr, s0, ns) of a stride-2 data gradient, recomputed here: taps r0 + 2i, s0 + 2j."""
    out = []
    for ph in (0, 1):
        r0 = (ph + pad) % 2
        nr = len(range(r0, k, 2))
        for pw in (0, 1):
            s0 = (pw + pad) % 2
            ns = len(range(s0, k, 2))
            if nr and ns:
                out.append((r0, nr, s0, ns))
    return out


# ---------------------------------------------------------------------------------------------- 1. weight packs
PackCase = collections.namedtuple("PackCase", "name cout cin kh kw kw_pad c_pad mode scaled taps")
PACK = [
    PackCase("stem-7x7-kw8-c4", 5, 3, 7, 7, 8, 4, 0, False, None),
    PackCase("3x3-fwd", 6, 8, 3, 3, 3, 8, 0, False, None),
    PackCase("3x3-dgrad-scaled", 6, 8, 3, 3, 3, 8, 1, True, None),
    PackCase("1x1-dgrad-cpad8", 7, 5, 1, 1, 1, 8, 1, False, None),
] + [PackCase("3x3-s2-class-%d%d%d%d" % t, 6, 8, 3, 3, 3, 8, 2, True, t) for t in s2_classes(3, 1)]


def pack_inputs(c, seed=100):
    w = synth.normal((c.cout, c.cin, c.kh, c.kw), seed)
    scale = synth.normal((c.cout,), seed + 1, 0.5, 1.0) if c.scaled else None
    return w, scale


def pack_ref(w, kw_pad, c_pad, mode, scale=None, taps=None, kw_taken=None):
    """rn_pack_weights in index arithmetic: fp32 [rows, Kpad], padding +0.0; mode 0: row = co, [r][s][ci]; modes 1 / 2: row = ci,
    [r][s][co], times scale[co] as ONE fp32 product (numpy's float32 product is the same correctly rounded one).
    kw_taken: the tap-row pitch actually used (the fault "kw_pad taken as kw" passes kw)."""
    cout, cin, kh, kw = w.shape
    pitch = kw_pad if kw_taken is None else kw_taken
    ntap = taps[1] * taps[3] if taps is not None else kh * kw_pad
    rows, chans = (cout, cin) if mode == 0 else (cin, cout)
    out = np.zeros((rows, kpad(ntap, c_pad)), dtype=np.float32)
    ws = w if (scale is None or mode == 0) else w * scale.astype(np.float32)[:, None, None, None]
    assert ws.dtype == np.float32
    for tap in range(ntap):
        if taps is not None:
            r, s = taps[0] + 2 * (tap // taps[3]), taps[2] + 2 * (tap % taps[3])
        else:
            r, s = tap // pitch, tap % pitch
            if r >= kh or s >= kw:
                continue
        out[:, tap * c_pad:tap * c_pad + chans] = ws[:, :, r, s] if mode == 0 else ws[:, :, r, s].T
    return out


# ---------------------------------------------------------------------------------------------- 1. batch-norm fold
FOLD_C = (1, 255, 256, 257)
FOLD_EPS = 1e-5


def fold_inputs(C, seed=120):
    """gamma with zeros and negatives, var cycling through 0, 1e-12, 1 and 1e6, mean and beta of either sign."""
    gamma = synth.normal((C,), seed)
    gamma[3::7] = 0.0
    gamma[5::11] = -np.abs(gamma[5::11]) - np.float32(0.25)
    beta = synth.normal((C,), seed + 1)
    mean = synth.normal((C,), seed + 2, 3.0)
    var = np.array([0.0, 1e-12, 1.0, 1e6], dtype=np.float32)[np.arange(C) % 4]
    return gamma, beta, mean, var


def fold_ref(gamma, beta, mean, var, eps=FOLD_EPS):
    """-> (rstd, scale, shift) in float64 and their bounds.  eps is the fp32 value the kernel receives.
    rstd = 1.0f / sqrtf(var + eps): add, sqrt, divide = 3 roundings.
    scale = gamma * rstd: one more = 4.
    shift = beta - mean * scale: the product carries scale's 4 and its own rounding (5 on |mean scale|), the subtraction one more on both
    terms: at most 6 u (|beta| + |mean scale|)."""
    g, b, m, v = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (gamma, beta, mean, var))
    rstd = 1.0 / np.sqrt(v + np.float64(np.float32(eps)))
    scale = g * rstd
    shift = b - m * scale
    return (rstd, scale, shift), (nu(3) * np.abs(rstd), nu(4) * np.abs(scale), nu(6) * (np.abs(b) + np.abs(m * scale)))


# ---------------------------------------------------------------------------------------------- 1. / 2. Winograd F(4x4, 3x3) weight side
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
             dtype=np.float64)
WINO_W = [(5, 8), (3, 40)]             # (Cout, Cin): K padded to 32 and 64
WINO_DW = [(3, 8), (2, 40)]


def wino_w_inputs(cout, cin, seed=140):
    return synth.normal((cout, cin, 3, 3), seed), synth.normal((cout,), seed + 1, 0.5, 1.0)


def wino_weights_ref(w, mode, scale=None, flip=True):
    """U = G g G^T -> float64 [36, rows, Kpad] and its bound.  mode 0: row = co, k = ci, g = w[co][ci]; mode 1: row = ci, k = co,
    g = w[co][ci] rotated by 180 degrees (flip=False is the fault that forgets it), times scale[co].  Columns k >= the real count are 0.
    Roundings per stage, longest path (a / 24 + b / 12 + c / 6, or -(a + b + c) / 6): the constant, the product, two additions = 4; two
    stages = 8; the product with scale one more = 9.  On n u (|G| |g| |G|^T)."""
    g = np.asarray(w, dtype=np.float32).astype(np.float64)
    if mode == 1:
        g = (g[:, :, ::-1, ::-1] if flip else g).transpose(1, 0, 2, 3)
        if scale is not None:
            g = g * np.asarray(scale, dtype=np.float32).astype(np.float64)[None, :, None, None]
    rows, k = g.shape[:2]
    out = np.zeros((36, rows, kpad(1, k)), dtype=np.float64)
    bound = np.zeros_like(out)
    # (G g G^T)[i][j] = sum_rs G[i][r] G[j][s] g[r][s]: one product with kron(G, G) [6 i + j, 3 r + s] over all (row, k) pairs
    ggt = lambda m, t: (t.reshape(rows * k, 9) @ np.kron(m, m).T).T.reshape(36, rows, k)
    out[:, :, :k] = ggt(G, g)
    n = 8 + (1 if (mode == 1 and scale is not None) else 0)
    bound[:, :, :k] = nu(n) * ggt(np.abs(G), np.abs(g))
    return out, bound


def wino_dw_inputs(cout, cin, seed=160):
    """dU [36, Cout, Ku] with NaN in the columns ci >= Cin, dw [Cout, Kpad] random in its first 9 Cin columns (the kernel adds to them)
    and NaN behind."""
    ku, kp = kpad(1, cin), kpad(9, cin)
    dU = np.full((36, cout, ku), np.nan, dtype=np.float32)
    dU[:, :, :cin] = synth.normal((36, cout, cin), seed)
    dw = np.full((cout, kp), np.nan, dtype=np.float32)
    dw[:, :9 * cin] = synth.normal((cout, 9 * cin), seed + 1)
    return dU, dw


def wino_dw_ref(dU, dw_before, cin):
    """dw[co][(3r + s) Cin + ci] += (G^T dU G)[r][s] -> float64 [Cout, 9 Cin] and its bound.
    Roundings per stage, longest path ((v3 + v4 - v1 - v2) * (1.f / 6.f) + v5): three additions, the constant, the product, the last
    addition = 6; two stages = 12; the += into dw one more on both terms: 13 u (|G|^T |dU| |G|) + u |dw_before|."""
    cout = dU.shape[1]
    d = dU[:, :, :cin].astype(np.float64).reshape(6, 6, cout, cin).transpose(2, 3, 0, 1)                       # [a, b, 6, 6]
    before = dw_before[:, :9 * cin].astype(np.float64)
    gtg = lambda m, t: np.ascontiguousarray((m.T @ t @ m).transpose(0, 2, 3, 1)).reshape(cout, 9 * cin)        # -> [a, 3 r + s, b]
    add, mag = gtg(G, d), gtg(np.abs(G), np.abs(d))
    return before + add, nu(13) * mag + nu(1) * np.abs(before)


# ---------------------------------------------------------------------------------------------- 1. batched preparation: chunk counts
def prep_blocks(kind, rows=0, Kpad=0, Cout=0):
    """Workgroups job `kind` of prep_batched_kernel needs (chunk rows (job, 0 .. blocks - 1)), from the kernel's own indexing: kind 0 one
    thread per channel; kind 5 four rows per workgroup; kind 4 eight values per thread; kinds 1, 2, 3 one thread per element of [rows, Kpad]."""
    n = {0: Cout, 5: (rows + 3) // 4 * 256, 4: rows * Kpad // 8}.get(kind, rows * Kpad)
    return (n + 255) // 256


# ---------------------------------------------------------------------------------------------- 2. weight-gradient unpack
UnpackCase = collections.namedtuple("UnpackCase", "name cout cin kh kw kw_pad c_pad")
UNPACK = [
    UnpackCase("stem-7x7-kw8-c4", 3, 3, 7, 7, 8, 4),
    UnpackCase("3x3", 5, 8, 3, 3, 3, 8),
    UnpackCase("1x1-n300-wraps", 2, 300, 1, 1, 1, 300),
    UnpackCase("1x1-n4-one-wave", 4, 4, 1, 1, 1, 4),
]
UNPACK_BATCHED = UNPACK[:3]
UNPACK_FORMS = ("bn", "bias", "plain")


def unpack_slots(c):
    """Packed column of OIHW element (ci, r, s), flattened in that order."""
    ci, r, s = np.meshgrid(np.arange(c.cin), np.arange(c.kh), np.arange(c.kw), indexing="ij")
    return ((r * c.kw_pad + s) * c.c_pad + ci).ravel()


def unpack_inputs(c, seed=180, cancel=True):
    """Packed dw and w_packed [Cout, Kpad] with NaN in every padded slot, and the per-channel operands.  cancel: channel 0's mean is chosen
    so that mean * colsum has the size of the dot product and the subtraction in dgamma cancels."""
    kp, slots = kpad(c.kh * c.kw_pad, c.c_pad), unpack_slots(c)
    n = c.cin * c.kh * c.kw
    d = {"g": synth.normal((c.cout, n), seed), "w": synth.normal((c.cout, n), seed + 1)}
    for name, key in (("dw", "g"), ("wp", "w")):
        d[name] = np.full((c.cout, kp), np.nan, dtype=np.float32)
        d[name][:, slots] = d[key]
    d["scale"] = synth.normal((c.cout,), seed + 2, 0.5, 1.0)
    d["mean"] = synth.normal((c.cout,), seed + 3)
    d["rstd"] = np.abs(synth.normal((c.cout,), seed + 4)) + np.float32(0.5)
    d["colsum"] = synth.normal((c.cout,), seed + 5, 2.0)
    if cancel:
        dot = float((d["w"][0].astype(np.float64) * d["g"][0].astype(np.float64)).sum())
        d["mean"][0] = np.float32(dot / float(d["colsum"][0]))
    return d


def unpack_ref(d, scaled=True, drop_mean=False):
    """-> dweight (fp32, to be met bit for bit: ONE product scale * g, or g itself), dgamma (float64) and its bound.
    dgamma = (sum w g - mean colsum) rstd is accumulated and formed in double and rounded to fp32 once: 1 u |r|; what the double
    arithmetic adds (n <= 300 products and additions at 2^-53) lies under 1e-12 of the terms' magnitudes.
    drop_mean: the fault that leaves the mean * colsum term out."""
    g, w = d["g"], d["w"]
    dweight = d["scale"][:, None] * g if scaled else g.copy()
    assert dweight.dtype == np.float32
    f = lambda k: d[k].astype(np.float64)
    dot = (w.astype(np.float64) * g.astype(np.float64)).sum(1)
    mag = np.abs(w.astype(np.float64) * g.astype(np.float64)).sum(1)
    mc = f("mean") * f("colsum")
    dgamma = (dot - (0.0 if drop_mean else mc)) * f("rstd")
    return dweight, dgamma, nu(1) * np.abs(dgamma) + 1e-12 * (mag + np.abs(mc)) * np.abs(f("rstd"))


# ---------------------------------------------------------------------------------------------- 3. max-pool 3x3 / stride 2 / padding 1
POOL = [(1, 4, 1, 1), (1, 4, 2, 3), (2, 4, 4, 4), (3, 12, 13, 10), (1, 40, 30, 26), (1, 32, 5, 7)]       # (N, C, H, W)
POOL_VALUES = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0], dtype=np.float32)


def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def pool_x(shape, seed=200, fine=False):
    """NHWC input of case (N, C, H, W).  Six values, so that nearly every window ties and many are all negative; every second zero is
    -0.0.  fine: normal values instead, which bf16 cannot hold."""
    N, C, H, W = shape
    if fine:
        return synth.normal((N, H, W, C), seed)
    x = POOL_VALUES[synth.randint((N, H, W, C), seed, 6)]
    z = np.flatnonzero(x == 0)
    x.reshape(-1)[z[::2]] = -0.0
    return x


def pool_ref(x, last=False, pad_value=-np.inf):
    """-> (y fp32, argmax uint8) [N, Ho, Wo, C]: the maximum over the in-bounds values of rows 2 oh - 1 .. 2 oh + 1 (the padding is -inf,
    which no finite value loses to) and the FIRST maximum in (r, s) order, coded 3 r + s.
    last: the fault that takes the last maximum; pad_value=0: the fault that counts padding as 0."""
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = np.full((N, H + 2, W + 2, C), pad_value, dtype=np.float32)
    xp[:, 1:H + 1, 1:W + 1] = x
    y = np.full((N, Ho, Wo, C), -np.inf, dtype=np.float32)
    arg = np.zeros((N, Ho, Wo, C), dtype=np.uint8)
    for r in range(3):
        for s in range(3):
            v = xp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2]
            take = (v >= y) if last else (v > y)
            y = np.where(take, v, y)
            arg = np.where(take, np.uint8(3 * r + s), arg)
    return y, arg


def pool_bwd_ref(arg, dy, H, W, keep=None):
    """-> dx float64 [N, H, W, C] and its bound: every input element takes dy of the windows whose code names it.
    At most four windows hold an element; the first addition is to 0.f and exact, the others round: 3 u sum |terms|.  keep (bool, the ReLU
    mask x > 0): elements off it are exactly 0, as are those no window names."""
    N, Ho, Wo, C = arg.shape
    dy = np.asarray(dy, dtype=np.float64)
    dxp, mag = np.zeros((N, H + 3, W + 3, C)), np.zeros((N, H + 3, W + 3, C))
    for r in range(3):
        for s in range(3):
            hit = arg == 3 * r + s
            dxp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += np.where(hit, dy, 0.0)
            mag[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += np.where(hit, np.abs(dy), 0.0)
    dx, mag = dxp[:, 1:H + 1, 1:W + 1], mag[:, 1:H + 1, 1:W + 1]
    if keep is not None:
        dx, mag = np.where(keep, dx, 0.0), np.where(keep, mag, 0.0)
    return dx, nu(3) * mag


def sign_words(x):
    """rn_mask_load4's operand: bit i & 31 of word i >> 5 over the flat index = (x > 0)."""
    b = (np.asarray(x).reshape(-1, 32) > 0).astype(np.uint32)
    return (b << np.arange(32, dtype=np.uint32)).sum(1, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- 4. FPN top-down gradient
UPSAMPLE = [((9, 13), (5, 7)), ((10, 14), (5, 7)), ((1, 1), (1, 1)), ((2, 1), (1, 1))]      # (Hs, Ws) -> (Hd, Wd)
UPSAMPLE_N, UPSAMPLE_C = 2, (4, 12)


def upsample_inputs(case, C, seed=220, bf16=False):
    (Hs, Ws), (Hd, Wd) = case
    src, dst = synth.normal((UPSAMPLE_N, Hs, Ws, C), seed), synth.normal((UPSAMPLE_N, Hd, Wd, C), seed + 1)
    return (bf16_round(src), bf16_round(dst)) if bf16 else (src, dst)


def upsample_add_bwd_ref(src, dst, bf16=False, crop=0):
    """dst[n, h, w] + the in-bounds children src[n, 2h + dy, 2w + dx] -> float64 and its bound.
    dst and up to four children are added one by one: 4 roundings on sum |terms|.  bf16 (operands hold bf16 values, fp32 arithmetic, one
    bf16 rounding on the store): u_b |r| more.  crop=1: the fault that leaves the last source row and column out."""
    src, out = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64).copy()
    mag = np.abs(out)
    Hs, Ws = src.shape[1] - crop, src.shape[2] - crop
    for dy in range(2):
        for dx in range(2):
            sub = src[:, dy:Hs:2, dx:Ws:2]
            out[:, :sub.shape[1], :sub.shape[2]] += sub
            mag[:, :sub.shape[1], :sub.shape[2]] += np.abs(sub)
    return out, nu(4) * mag + (SLACK * UB * np.abs(out) if bf16 else 0.0)


# ---------------------------------------------------------------------------------------------- 4. head-output gradient slices
SIGMOID_B, SIGMOID_ROWS = 2, 35
SIGMOID = [(72, 96), (5, 8), (8, 8)]                       # (C, ld); B * rows * ld is no multiple of 256 for any of them
SIG_LO = 2.0 ** -20


def concat_slice(B, rows, C, seed, before=3, after=2, std=1.0):
    """A head level's slice of a wider concatenated [B, A, C] tensor: -> (the whole tensor with NaN outside the slice, the slice's values
    [B, rows, C], the slice's offset in floats, the batch stride A * C)."""
    A = before + rows + after
    whole = np.full((B, A, C), np.nan, dtype=np.float32)
    vals = synth.normal((B, rows, C), seed, std)
    whole[:, before:before + rows] = vals
    return whole, vals, before * C, A * C


def sigmoid_values(shape, seed):
    """s in [2^-20, 1 - 2^-20] with both ends present, and exact 0 and 1."""
    s = np.clip(synth.uniform(shape, seed), np.float32(SIG_LO), np.float32(1.0 - SIG_LO)).astype(np.float32)
    f = s.reshape(-1)
    f[0::13], f[1::13], f[2::13], f[3::13] = 0.0, 1.0, SIG_LO, 1.0 - SIG_LO
    return s


def signed_zeros(a, step=9):
    """dy with +0.0 and -0.0 among its values (in place)."""
    f = a.reshape(-1)
    f[4::step] = 0.0
    f[8::2 * step] = -0.0
    return a


def sigmoid_bwd_pad_ref(dy, s, ld, bf16=False):
    """dy, s [B, rows, C] -> float64 [B * rows, ld] and its bound: dy s (1 - s) in the first C columns, 0 in the padding.
    1.0f - s, s * (1 - s), dy * (...): 3 roundings, all relative; without s the value is copied (the bound only allows what it allows).
    Where s is 0 or 1 the reference is 0 and so is its bound.  bf16: one bf16 rounding on the store, u_b |r| more."""
    B, rows, C = dy.shape
    r = dy.astype(np.float64)
    if s is not None:
        r = r * (s.astype(np.float64) * (1.0 - s.astype(np.float64)))
    out = np.zeros((B * rows, ld))
    out[:, :C] = r.reshape(B * rows, C)
    return out, (nu(3) if s is not None else 0.0) * np.abs(out) + (SLACK * UB * np.abs(out) if bf16 else 0.0)


def flags_ref(H, W, pixels, halo=True):
    """Tile activity flags [len(pixels), ceil(H/4), ceil(W/4)] uint8 for images whose only non-zero value is at pixels[b] = (h, w) (None:
    no non-zero value): tile (th, tw) is 1 iff the pixel lies in its 6 x 6 patch, rows 4 th - 1 .. 4 th + 4 and columns 4 tw - 1 .. 4 tw + 4.
    halo=False: the fault that sets the pixel's own tile only."""
    TH, TW = (H + 3) // 4, (W + 3) // 4
    out = np.zeros((len(pixels), TH, TW), dtype=np.uint8)
    e = 1 if halo else 0
    for b, p in enumerate(pixels):
        if p is None:
            continue
        for th in range(TH):
            for tw in range(TW):
                if 4 * th - e <= p[0] <= 4 * th + 3 + e and 4 * tw - e <= p[1] <= 4 * tw + 3 + e:
                    out[b, th, tw] = 1
    return out


def flags_inputs(H, W, C, extra_empty=False):
    """One image per pixel position: image b's only non-zero dy is at pixel b, channel b % C (extra_empty: every such image is followed by
    an all-zero one, so that a write to a neighbouring flag shows even where every image has one tile); then an image whose only
    non-zero is a -0.0 (it is a zero: no flag), an all-zero image, and an image with a non-zero dy under s = 1 (the product is 0).
    -> dy [B, H * W, C], s [B, H * W, C], pixels."""
    pixels = []
    for p in range(H * W):
        pixels.append((p // W, p % W))
        if extra_empty:
            pixels.append(None)
    B = len(pixels) + 3
    dy = np.zeros((B, H * W, C), dtype=np.float32)
    s = np.full((B, H * W, C), 0.25, dtype=np.float32)
    k = 0
    for b, p in enumerate(pixels):
        if p is not None:
            dy[b, p[0] * W + p[1], k % C] = 1.5 if k % 2 else -0.75
            k += 1
    b = len(pixels)
    dy[b, (H * W) // 2, 1] = -0.0
    dy[b + 2, H * W - 1, C - 1] = 2.0
    s[b + 2, H * W - 1, C - 1] = 1.0
    return dy, s, pixels + [None, None, None]


# ---------------------------------------------------------------------------------------------- 4. column sums
COLSUM = [(1, 257, 260), (3, 256, 256), (3, 1, 4), (4, 257, 260), (5, 36, 40), (511, 36, 40), (512, 1, 4), (512, 36, 40), (513, 36, 40),
          (513, 1, 4), (1027, 36, 40), (1027, 257, 260)]                                  # (rows, C, ld)
CS_ROWS = 512


def colsum_inputs(rows, C, ld, seed=260):
    """[rows, ld] with NaN in the columns past C (never read); column 0 alternates +-1e4 plus a small term, so its sum is small and an error
    the size of 1e-5 of the largest column sum would pass a tolerance relative to that."""
    g = np.full((rows, ld), np.nan, dtype=np.float32)
    g[:, :C] = synth.normal((rows, C), seed)
    g[:, 0] = g[:, 0] * np.float32(0.01) + np.where(np.arange(rows) % 2 == 0, np.float32(1e4), np.float32(-1e4))
    return g, synth.normal((C,), seed + 1, 5.0)


def colsum_ref(g, C, before=None):
    """-> float64 [C] and its bound.  A first-pass workgroup takes 512 rows on four accumulators: 127 quads, and for a 511-row chunk
    three more rows on the first = at most 130 additions into one accumulator (the first, to 0.f, is exact but counted), two to combine
    the four, and the final rounding of the double second pass (whose own additions, at 2^-53, vanish in the 1.01): n = 133 on sum |g|;
    accumulate adds u |out_before|."""
    v = g[:, :C].astype(np.float64)
    s, mag = v.sum(0), np.abs(v).sum(0)
    if before is None:
        return s, nu(133) * mag
    b = before.astype(np.float64)
    return s + b, nu(133) * mag + nu(1) * np.abs(b)


# ---------------------------------------------------------------------------------------------- 4. small elementwise
RELU_BF16_N = (4, 1020, 1024, 1028)
ADD_N = (255, 256, 257)
NHWC4 = [(1, 15, 17), (1, 16, 16), (1, 1, 257), (2, 10, 13)]      # (N, H, W): 255, 256, 257 pixels and 2 x 130


def relu_bf16_inputs(n, seed=280):
    """bf16 bits: normal values with +-0 and +-inf among them."""
    x = synth.normal((n,), seed)
    x[0], x[1], x[2], x[3] = 0.0, -0.0, np.inf, -np.inf
    return bf16_rne(x)


def nhwc4_ref(img):
    """[N, 3, H, W] -> [N, H, W, 4] with the fourth channel +0.0."""
    N, _, H, W = img.shape
    out = np.zeros((N, H, W, 4), dtype=np.float32)
    out[..., :3] = img.transpose(0, 2, 3, 1)
    return out


# ---------------------------------------------------------------------------------------------- 5. clip + Adam
OPT_CHUNK = 4096
OPT_SIZES = [1] * 1100 + [4096, 4097]                      # 1100 + 1 + 2 = 1103 chunks: past the 1024-thread loop of the norm's final pass
OPT_HP = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.1)
OPT_GRAD_STD = (1e-4, 10.0, 1e-4)                          # step 1 not clipped, step 2 clipped, step 3 not clipped


def opt_chunks(sizes):
    """[(tensor, chunk inside the tensor)] in ClipAdam's order."""
    return [(t, c) for t, n in enumerate(sizes) for c in range((n + OPT_CHUNK - 1) // OPT_CHUNK)]


def opt_params(seed=300):
    return [synth.normal((n,), seed + i % 7, 0.5) for i, n in enumerate(OPT_SIZES)]


def opt_grads(step, mult=1.0, seed=320):
    return [synth.normal((n,), seed + 10 * step + i % 9, OPT_GRAD_STD[step]) * np.float32(mult) for i, n in enumerate(OPT_SIZES)]


def f32(x):
    """The hyper-parameters reach the kernels as fp32 values."""
    return np.float64(np.float32(x))


def opt_norm_ref(grads, grad_scale=1.0, skip_chunk=None):
    """sqrt(sum g^2) * grad_scale in float64 and its bound.  A thread of the first pass adds up to 16 squares in fp32 (product and
    addition: the first term sees its product's rounding and 15 additions = 16 roundings on the sum of squares, every term non-negative);
    the rest is double.  The square root halves a relative error (8), the cast to fp32 adds one: 9 u relative.
    skip_chunk: the fault that leaves one chunk's partial sum out."""
    t = 0.0
    for k, (ti, c) in enumerate(opt_chunks([g.size for g in grads])):
        if k != skip_chunk:
            t += float((grads[ti][c * OPT_CHUNK:(c + 1) * OPT_CHUNK].astype(np.float64) ** 2).sum())
    r = np.sqrt(t) * f32(grad_scale)
    return r, nu(9) * r


def opt_step_ref(p, g, m, v, norm, step, grad_scale=1.0, hp=OPT_HP):
    """One step of opt_adam_kernel in float64 from the fp32 state (p, m, v), the fp32 gradient g and the fp32 norm the kernel itself read
    (its own first pass's result, held to opt_norm_ref separately) -> dict of (reference, bound) for "g", "m", "v", "p".
      coef = min(1, max_norm / (norm + 1e-6f)) * grad_scale: addition and division round (2); the product with grad_scale is a third
      rounding unless grad_scale is a power of two.
      g' = g coef: one more: 3 (4) u |g'|.
      m' = beta1 m + (1 - beta1) g' (1 - beta1 is exact in fp32 for beta1 in [0.5, 1]): beta1 m sees its product and the addition (2), the
      other term g's 3 (4), its product and the addition (5 / 6).
      v' = beta2 v + ((1 - beta2) g') g': beta2 v 2; the other term twice g's 3 (4), two products, the addition (9 / 11).
      p' = p - step (m' / denom), step = lr / bc1, denom = sqrtf(v') / bc2_sqrt + eps, bc1 and bc2_sqrt double results cast to fp32:
      denom carries half of v's relative error (v' is a sum of non-negative terms: at most 9 (11) / 2, rounded up to 5 (6)), sqrtf, the cast, the
      division, the addition = 9 (10) relative; m' / denom one more, step two (cast, division), their product one: 13 (14) u |update|, plus
      m's own bound scaled by step / denom (m' may cancel, so that bound is not relative to m'); the subtraction rounds once: u |p'|."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    p, g, m, v = f(p), f(g), f(m), f(v)
    lr, b1, b2, eps, max_norm, gs = f32(hp["lr"]), f32(hp["beta1"]), f32(hp["beta2"]), f32(hp["eps"]), f32(hp["max_norm"]), f32(grad_scale)
    pow2 = float(np.frexp(float(gs))[0]) == 0.5
    ng = 3 if pow2 else 4
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, max_norm / (np.float64(np.float32(norm)) + f32(1e-6)))
    coef *= gs
    g1 = g * coef
    t1, t2 = b1 * m, (1.0 - b1) * g1
    m1 = t1 + t2
    m_bound = nu(2) * np.abs(t1) + nu(ng + 2) * np.abs(t2)
    s1, s2 = b2 * v, (1.0 - b2) * g1 * g1
    v1 = s1 + s2
    v_bound = nu(2) * s1 + nu(2 * ng + 3) * s2
    bc1, bc2s = 1.0 - b1 ** step, np.sqrt(1.0 - b2 ** step)
    denom = np.sqrt(v1) / bc2s + eps
    upd = (lr / bc1) * (m1 / denom)
    p1 = p - upd
    nd = (2 * ng + 3 + 1) // 2 + 4
    p_bound = nu(1) * np.abs(p1) + nu(nd + 4) * np.abs(upd) + (lr / bc1) * m_bound / denom
    return {"g": (g1, nu(ng) * np.abs(g1)), "m": (m1, m_bound), "v": (v1, v_bound), "p": (p1, p_bound)}

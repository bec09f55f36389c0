"""Cases, float64 references and error bounds for the two Winograd F(4x4, 3x3) transform kernels of csrc/conv_wino.hip, wino_in_kernel and
wino_out_kernel, in their dense forms.  CPU only (numpy): tests/test_wino_cases_host.py proves what is here against torch's float64
convolution and shows that every comparison rejects a wrong answer; tests/test_gpu_wino_transforms.py holds the kernels to it.

References are written from the mathematics and the documented layouts: the matrices B^T, G and A^T of Lavin & Gray ("Fast Algorithms for
Convolutional Neural Networks", F(4x4, 3x3)) are literal arrays, V / Z / M are [36][T][C] with position 6 i + j and the tiles of a problem
[N, H, W, C] in the order n, th, tw, groups are the concatenation of their problems in table order.

Two operand sets.  EXACT: small integers (x, dy, addends in [-8, 8], M in [-16, 16], scales from {0.5, 1, 2, 4}, integer shifts).  B^T and A
hold integers only, so every intermediate of either transform, in any order of operations and however multiply-adds are contracted, is a
multiple of 1/2 far below 2^23 and therefore exact in fp32: the result must EQUAL the reference as numbers (check_exact asserts the
condition on the sum of magnitudes, which bounds every intermediate).  REAL: normal values, another power of two per problem; the result
must lie within the per-element bound gamma_k (|B^T| |d| |B|) of the float64 reference (the same with |A| for Z and for the output transform),
gamma_k = k u / (1 - k u), u = 2^-24, k = the number of fp32 roundings on the longest path from an input to an output, counted from the
kernel's source without contraction (contraction only removes roundings; a product with a power of two is exact):

  bt6 (conv_wino.hip:43-48)   3 per 1-D pass: o[0] = 4 d0 - 5 d2 + d4 rounds 5 d2, the difference and the sum (line 43; lines 45-48 alike,
                              line 44 has 2), so K_V = 6 for B^T d B
  a6  (conv_wino.hip:117-123) 2 per 1-D pass: o[1] = (v0 + v2) + (v1 + v3) (lines 117, 119), o[3] = (v0 + 4 v2) + (2 v1 + 8 v3) (lines
                              121-122): no path holds more than two sums, so K_Z = 4 for A dy A^T (the issue's first count of 3 was one
                              too many; the tighter count stands)
  at6 (conv_wino.hip:52-56)   3 per 1-D pass: o[0] = (m0 + (m1 + m2)) + (m3 + m4) (lines 52-53), o[3] = ((m1 - m2) + 8 (m3 - m4)) + m5
                              (lines 52, 56), so K_OUT = 6 for A^T m A
  epilogue (conv_wino.hip:383, 395)   one more each for the product with scale, the sum with shift and the sum with the addend; masks and
                              ReLU round nothing.  Sigmoid: 3 u |s| for expf, the sum and the quotient (the count glue_cases.py uses for the
                              sigmoid kernels) on top of the bound at its input times |s'| <= 1/4.
Where a bound is 0 (masked elements) the result must be exactly zero."""
import collections
import functools

import numpy as np

U = 2.0 ** -24
RN_MAX_GROUP = 5
MASK_BITS = 4                                   # RN_MASK_BITS of include/retinanet_mi355x.h
GAIN_BT, GAIN_A = 7, 8                          # log2 gains of the derived amax words: B^T d B, and A dy A^T / the fused both-form
K_BT6, K_A6, K_AT6 = 3, 2, 3                    # roundings per 1-D pass (above)
K_V, K_Z, K_OUT = 2 * K_BT6, 2 * K_A6, 2 * K_AT6

BT = np.array([[4, 0, -5, 0, 1, 0],
               [0, -4, -4, 1, 1, 0],
               [0, 4, -4, -1, 1, 0],
               [0, -2, -1, 2, 1, 0],
               [0, 2, -1, -2, 1, 0],
               [0, 4, 0, -5, 0, 1]], dtype=np.float64)
G = np.array([[1 / 4, 0, 0],
              [-1 / 6, -1 / 6, -1 / 6],
              [-1 / 6, 1 / 6, -1 / 6],
              [1 / 24, 1 / 12, 1 / 6],
              [1 / 24, -1 / 12, 1 / 6],
              [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0],
               [0, 1, -1, 2, -2, 0],
               [0, 1, 1, 4, 4, 0],
               [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------- comparisons
def same_values(got, want):
    """As numbers, element for element: -0.0 equals 0.0, a NaN equals nothing."""
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


def check_exact(mag):
    """The exactness condition of the EXACT operand set on a sum of magnitudes (which bounds every intermediate of every order of
    operations): a multiple of 1/2 below 2^23.  Returns the largest magnitude."""
    mag = np.asarray(mag, dtype=np.float64)
    assert np.array_equal(2.0 * mag, np.round(2.0 * mag)) and mag.max() < 2.0 ** 23, mag.max()
    return float(mag.max())


# ---------------------------------------------------------------------------------------------- geometry
def n_tiles(shape):
    N, H, W = shape[:3]
    return N * ((H + 3) // 4) * ((W + 3) // 4)


def tile_ends(shapes):
    return np.cumsum([n_tiles(s) for s in shapes]).tolist()


def patches(x, corner, size, wrap=False):
    """x [N, H, W, C] -> float64 [N, TH, TW, size, size, C]: per 4x4 output tile (th, tw) the size x size patch whose corner is
    (4 th + corner, 4 tw + corner); pixels outside the image are zero.  wrap (a WRONG form, for the host test): a pixel left or right of the
    image is taken from the flat offset h W + w instead, the end of the row above or the start of the row below."""
    N, H, W, C = x.shape
    TH, TW = (H + 3) // 4, (W + 3) // 4
    hh = (4 * np.arange(TH)[:, None] + corner + np.arange(size)[None, :])[:, None, :, None]
    ww = (4 * np.arange(TW)[:, None] + corner + np.arange(size)[None, :])[None, :, None, :]
    flat = hh * W + ww
    ok = (hh >= 0) & (hh < H) & ((flat >= 0) & (flat < H * W) if wrap else (ww >= 0) & (ww < W))
    d = x.reshape(N, H * W, C).astype(np.float64)[:, np.where(ok, flat, 0)]
    return np.where(ok[None, ..., None], d, 0.0)


# ---------------------------------------------------------------------------------------------- the transforms
def ref_v(x, absolute=False, bt=BT, corner=-1, wrap=False, swap=False):
    """x [N, H, W, C] -> [36, T, C]: position 6 i + j of tile (n, th, tw) is (B^T d B)[i][j], d the 6x6 patch with corner
    (4 th - 1, 4 tw - 1).  absolute: |B^T| |d| |B|, the sum of magnitudes the bound is made of.  bt / corner / wrap / swap: the wrong forms
    of the host test (another matrix, another corner, wrapped halo pixels, positions 6 i + j and 6 j + i exchanged)."""
    d = patches(x, corner, 6, wrap)
    if absolute:
        bt, d = np.abs(bt), np.abs(d)
    v = np.einsum("ia,nhwabc,jb->ijnhwc", bt, d, bt)
    if swap:
        v = v.swapaxes(0, 1)
    return v.reshape(36, -1, x.shape[3])


def ref_z(dy, absolute=False):
    """dy [N, H, W, C] -> [36, T, C]: position 6 a + b is (A dy A^T)[a][b] of the tile's own 4x4 block, zero past the edge."""
    d, a = patches(dy, 0, 4), AT.T
    if absolute:
        a, d = np.abs(a), np.abs(d)
    return np.einsum("ai,nhwijc,bj->abnhwc", a, d, a).reshape(36, -1, dy.shape[3])


def ref_y(M, shape, absolute=False):
    """M [36, T, C] of one problem (N, H, W) -> [N, H, W, C]: A^T m A per tile, cut to H x W."""
    N, H, W = shape
    TH, TW = (H + 3) // 4, (W + 3) // 4
    m, at = np.asarray(M, dtype=np.float64).reshape(6, 6, N, TH, TW, -1), AT
    if absolute:
        m, at = np.abs(m), np.abs(at)
    return np.einsum("ai,ijnhwc,bj->nhawbc", at, m, at).reshape(N, 4 * TH, 4 * TW, -1)[:, :H, :W]


def concat(parts, second_early=False):
    """The group's tensor: the problems' [36, T_p, C] in table order.  second_early (WRONG): the second problem starts one row early."""
    if not second_early:
        return np.concatenate(parts, axis=1)
    assert len(parts) > 1
    out = np.zeros((36, sum(p.shape[1] for p in parts), parts[0].shape[2]))
    start = 0
    for i, p in enumerate(parts):
        at = start - 1 if i == 1 else start
        out[:, at:at + p.shape[1]] = p
        start += p.shape[1]
    return out


def expect_in(xs, kind, **wrong):
    """The group's V (kind "v") or Z ("z") of the sources xs -> (float64 reference [36, T, C], per-element bound).  **wrong: a wrong form."""
    second_early = wrong.pop("second_early", False)
    f, k = (ref_v, K_V) if kind == "v" else (ref_z, K_Z)
    ref = concat([f(x, **wrong) for x in xs], second_early)
    return ref, gamma(k) * concat([f(x, absolute=True) for x in xs])


def f32_tree_product(mat, d, axis):
    """mat (r x s) applied along `axis` (of length s) of the float32 array d, in float32: the products one by one, summed as a binary tree
    over neighbours.  A sum with an exact zero rounds nothing, so no path has more roundings than the kernel's expressions (above)."""
    terms_of = lambda row: [np.float32(c) * np.take(d, k, axis=axis) for k, c in enumerate(row)]
    rows = []
    for row in mat:
        t = terms_of(row)
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        assert t[0].dtype == np.float32
        rows.append(t[0])
    return np.stack(rows, axis=axis)


def f32_transform(mat, d, axes, order):
    """mat d mat^T over the two `axes` of float32 d, the first axis first (order 0) or the second first (order 1)."""
    for ax in (axes if order == 0 else axes[::-1]):
        d = f32_tree_product(mat, d, ax)
    return d


# ---------------------------------------------------------------------------------------------- amax words
def word(e, gain):
    """The derived word of a tensor whose source's largest exponent field is e: exponent min(e + gain, 254), full mantissa; 0 for e <= 0."""
    return 0 if e <= 0 else (min(e + gain, 254) << 23) | 0x7fffff


def table_exp(table):
    """The highest set byte of one image's 256-byte table, 0 for an empty one."""
    nz = np.flatnonzero(np.asarray(table).reshape(256))
    return int(nz[-1]) if nz.size else 0


def row_words(shapes, tables, gain=GAIN_BT):
    """Per row of the group's V: the word of its own image's table (tables: per problem uint8 [N, 256], or None: NULL, word 0)."""
    out = []
    for (N, H, W), t in zip(shapes, tables):
        per_image = ((H + 3) // 4) * ((W + 3) // 4)
        for n in range(N):
            out += [word(0 if t is None else table_exp(t[n]), gain)] * per_image
    return np.array(out, dtype=np.uint32)


def tensor_word(tables, gain, start=0):
    """The tensor word: of the highest set byte over all images of all problems, raised by maximum into what the caller left there."""
    e = max([table_exp(img) for t in tables if t is not None for img in t] + [0])
    return max(int(start), word(e, gain))


def make_table(*images):
    """Per image a list of set bytes -> uint8 [N, 256]."""
    t = np.zeros((len(images), 256), dtype=np.uint8)
    for n, bytes_set in enumerate(images):
        t[n, list(bytes_set)] = 1
    return t


def out_tables(y):
    """What the output transform notes for a stored result y (fp32 [N, H, W, C]): uint8 [N, 256], byte e set exactly when some thread (one
    tile x 4 channels) stored a largest magnitude with exponent field e."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    N, H, W, C = y.shape
    t = np.zeros((N, 256), dtype=np.uint8)
    for n in range(N):
        for h0 in range(0, H, 4):
            for w0 in range(0, W, 4):
                am = np.abs(y[n, h0:h0 + 4, w0:w0 + 4]).reshape(-1, C // 4, 4).max(axis=(0, 2))
                t[n, (am.view(np.uint32) >> 23) & 0xff] = 1
    return t


def sign_words(y):
    """Bit (off & 31) of word (off >> 5) is set where the element at dense offset off is > 0."""
    on = (np.asarray(y).reshape(-1) > 0).astype(np.uint8)
    assert on.size % 32 == 0
    return np.packbits(on, bitorder="little").view("<u4").astype(np.uint32)


def mask_on(mask, bits, shift_mask=31):
    """Where the mask counts as on, in y's dense geometry `mask.shape` / `bits[1]`: mask > 0 of a float tensor, or bit (off & 31) of word
    (off >> 5) of sign words (bits = (words, shape)).  shift_mask (WRONG): 27, a nibble shift of off & 24, reads the low nibble of each byte."""
    if bits is None:
        with np.errstate(invalid="ignore"):
            return np.asarray(mask) > 0
    words, shape = bits
    off = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((np.asarray(words, dtype=np.uint32)[off >> 5] >> (off & shift_mask).astype(np.uint32)) & 1).astype(bool).reshape(shape)


# ---------------------------------------------------------------------------------------------- the output transform's epilogue
def ref_epilogue(v, mag, k, scale=None, shift=None, on=None, mask_mode=0, add=None, act=0):
    """The epilogue of wino_out_kernel in its documented order on float64 v with sum of magnitudes mag after k roundings ->
    (reference, bound): scale v + shift; mask (mode 1); addend; act (1 ReLU, 2 sigmoid); mask (mode 2)."""
    r, mag = np.array(v, dtype=np.float64), np.array(mag, dtype=np.float64)
    if scale is not None:
        r, mag, k = r * scale, mag * np.abs(scale), k + 1
    if shift is not None:
        r, mag, k = r + shift, mag + np.abs(shift), k + 1
    if mask_mode == 1:
        r, mag = np.where(on, r, 0.0), np.where(on, mag, 0.0)
    if add is not None:
        r, mag, k = r + add, mag + np.abs(add), k + 1
    bound = gamma(k) * mag
    if act == 1:
        r = np.maximum(r, 0.0)
    elif act == 2:
        with np.errstate(over="ignore"):
            r = 1.0 / (1.0 + np.exp(-r))
        bound = gamma(3) * r + 0.25 * bound
    if mask_mode == 2:
        r, bound = np.where(on, r, 0.0), np.where(on, bound, 0.0)
    return r, bound


# ---------------------------------------------------------------------------------------------- cases
G5 = [(2, 9, 6), (1, 4, 4), (3, 1, 1), (1, 2, 11), (2, 5, 8)]      # ragged on both edges; one full tile; images smaller than a tile; H < 4; H ragged
G5_HEAD = [(2, H, W) for _, H, W in G5]                             # N = 2 for every problem: one [N, A, n] buffer holds all five
WIDE = [(2, 13, 18)]                                                # 40 tiles x 65 threads = 2600 threads, 11 workgroups, 216 threads past the end
SINGLE = [(2, 5, 7)]
PLACEMENTS = [(48, 0), (64, 21)]                                    # (Tpad, tile_offset)
assert len(G5) == RN_MAX_GROUP and tile_ends(G5) == [12, 13, 16, 19, 27] and tile_ends(G5_HEAD)[-1] == 30 and tile_ends(WIDE) == [40]
assert all(off + 40 <= tpad for tpad, off in PLACEMENTS) and 21 + 27 == 48

IN_CASES = [("G5", G5, 4), ("G5", G5, 12), ("G5", G5, 64), ("wide", WIDE, 260), ("single", SINGLE, 12)]
POW2 = (0, 3, -3, 6, -6)                                            # REAL: problem i is scaled by 2^POW2[i]
POW2_HEAD = (0, 1, -1, 2, -3)                                       # ... in front of a sigmoid


def in_operands(shapes, C, exact, seed=400):
    """The sources of the input-side transforms, fp32 [N, H, W, C] per problem."""
    rng = np.random.default_rng([seed, C, int(exact)])
    if exact:
        return [rng.integers(-8, 9, size=s + (C,)).astype(np.float32) for s in shapes]
    return [(rng.standard_normal(s + (C,)) * 2.0 ** POW2[i]).astype(np.float32) for i, s in enumerate(shapes)]


def in_tables(shapes):
    """Hand-made amax tables of the sources, per problem uint8 [N, 256] or None (a NULL table).  G5: a highest byte with lower bytes set
    beside it (they must be ignored), an empty table, byte 250 (the word clamps at 254), byte 1, a NULL problem.  The other cases: no byte
    near the clamp, so that the two gains give different tensor words."""
    if shapes == G5:
        return [make_table([3, 100, 129, 130], []), make_table([250, 17]), make_table([1], [127, 126], [200, 4, 8]), None,
                make_table([90], [140, 139, 0])]
    if shapes == G5_HEAD:
        return [make_table([3, 100, 130], []), make_table([250, 17], [2]), make_table([1], [127, 126]), None, make_table([90], [140, 139, 0])]
    return [make_table([5, 100, 131], [77])]


Epilogue = collections.namedtuple("Epilogue", "scale shift mask_mode bits add act signs amax head real_only")
Epilogue.__new__.__defaults__ = (False, False, 0, False, (), 0, False, False, False, False)
ALL = (0, 1, 2, 3, 4)
EPILOGUES = {
    "plain": Epilogue(),
    "fwd": Epilogue(scale=True, shift=True, act=1, signs=True, amax=True),
    "head": Epilogue(shift=True, act=2, head=True, real_only=True),
    "dgrad1": Epilogue(scale=True, mask_mode=1, add=ALL),                       # the PADD instance
    "dgrad2-mixed": Epilogue(mask_mode=2, add=(0, 2, 3), act=1),                # the plain instance with a per-problem add pointer
    "bits1-add": Epilogue(mask_mode=1, bits=True, add=ALL),                     # PBITS and PADD
    "bits2": Epilogue(shift=True, mask_mode=2, bits=True, signs=True),          # PBITS alone
    "wide": Epilogue(scale=True, shift=True, act=1, amax=True),
    "single": Epilogue(scale=True, mask_mode=1, add=(0,)),
}
OUT_CASES = [("plain", G5, 32), ("plain", G5, 12), ("fwd", G5, 32), ("head", G5_HEAD, 12), ("dgrad1", G5, 32), ("dgrad2-mixed", G5, 32),
             ("bits1-add", G5, 64), ("bits2", G5, 64), ("wide", WIDE, 260), ("single", SINGLE, 12)]
MASK_VALUES = np.array([1.5, -2.0, 0.0, -0.0, np.nan, 0.25, -0.125, 3.0], dtype=np.float32)      # positive, negative, +0, -0, NaN


def head_layout(shapes, cout, before=3, between=1, after=2):
    """The five results as slices of ONE buffer [N, A, cout], as the heads store them: -> (A, the slices' first rows)."""
    rows, at = [], before
    for _, H, W in shapes:
        rows.append(at)
        at += H * W + between
    return at - between + after, rows


OutOperands = collections.namedtuple("OutOperands", "M scale shift masks bits adds")


def out_operands(name, shapes, cout, exact, seed=500):
    """Operands of one output-side case: M per problem fp32 [36, T_p, cout], scale / shift [cout] or None, per problem the float mask, its
    sign words and the addend (each or None)."""
    e = EPILOGUES[name]
    assert not (exact and e.real_only)
    rng = np.random.default_rng([seed, cout, int(exact), sorted(EPILOGUES).index(name)])
    pw = POW2_HEAD if e.head else POW2
    scale = shift = None
    if exact:
        M = [rng.integers(-16, 17, size=(36, n_tiles(s), cout)).astype(np.float32) for s in shapes]
        if e.scale:
            scale = rng.choice(np.array([0.5, 1.0, 2.0, 4.0], dtype=np.float32), size=cout)
        if e.shift:
            shift = rng.integers(-8, 9, size=cout).astype(np.float32)
    else:
        M = [(rng.standard_normal((36, n_tiles(s), cout)) * 2.0 ** pw[i]).astype(np.float32) for i, s in enumerate(shapes)]
        if e.scale:
            scale = rng.uniform(0.5, 2.0, size=cout).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=cout)
        if e.shift:
            shift = rng.standard_normal(cout).astype(np.float32)
    masks, bits, adds = [], [], []
    for i, s in enumerate(shapes):
        mask = rng.choice(MASK_VALUES, size=s + (cout,)) if e.mask_mode else None
        masks.append(mask)
        bits.append(sign_words(mask) if e.bits else None)
        if i not in e.add:
            adds.append(None)
        elif exact:
            adds.append(rng.integers(-8, 9, size=s + (cout,)).astype(np.float32))
        else:
            adds.append((rng.standard_normal(s + (cout,)) * 2.0 ** pw[i]).astype(np.float32))
        if mask is not None:
            assert all((mask.view(np.uint32) == v.view(np.uint32)).any() for v in MASK_VALUES)       # -0.0 and NaN among them
        if mask is not None and adds[-1] is not None:
            assert (~mask_on(mask, None) & (adds[-1] != 0)).any(), "modes 1 and 2 must differ somewhere"
    return OutOperands(M, scale, shift, masks, bits, adds)


def expect_out(name, shapes, ops, p, modes_swapped=False, edge_addend=False, shift_mask=31):
    """Problem p of an output-side case -> (float64 reference [N, H, W, cout], per-element bound, sum of magnitudes).  modes_swapped /
    edge_addend / shift_mask: wrong forms (mask modes 1 and 2 exchanged; the pixels of a tile that is ragged on the right take the
    addend of the image's last column; the mask bit's shift loses a bit)."""
    e, shape = EPILOGUES[name], shapes[p]
    on = None
    if e.mask_mode:
        on = mask_on(ops.masks[p], (ops.bits[p], ops.masks[p].shape) if e.bits else None, shift_mask)
    add = None if ops.adds[p] is None else ops.adds[p].astype(np.float64)
    if edge_addend and add is not None and shape[2] % 4:
        add = add.copy()
        add[:, :, shape[2] // 4 * 4:] = add[:, :, -1:]
    f64 = lambda a: None if a is None else a.astype(np.float64)
    mode = e.mask_mode if not modes_swapped else {0: 0, 1: 2, 2: 1}[e.mask_mode]
    args = dict(scale=f64(ops.scale), shift=f64(ops.shift), on=on, mask_mode=mode, add=add, act=e.act)
    ref, bound = ref_epilogue(ref_y(ops.M[p], shape), ref_y(ops.M[p], shape, absolute=True), K_OUT, **args)
    args.update(scale=None if ops.scale is None else np.abs(f64(ops.scale)), shift=None if ops.shift is None else np.abs(f64(ops.shift)),
                add=None if add is None else np.abs(add), act=0, mask_mode=1 if mode == 1 else 0)
    mag = ref_epilogue(ref_y(ops.M[p], shape, absolute=True), 0.0, 0, **args)[0]
    return ref, bound, mag


def head_buffer(shapes, cout, results, stride_ignored=False):
    """The heads' shared buffer [N, A, cout]: NaN except the five slices.  stride_ignored (WRONG): images H W cout apart, from the slice's
    start."""
    A, rows = head_layout(shapes, cout)
    N = shapes[0][0]
    buf = np.full((N, A, cout), np.nan)
    flat = buf.reshape(-1)
    for (_, H, W), r0, y in zip(shapes, rows, results):
        if stride_ignored:
            flat[r0 * cout:r0 * cout + y.size] = y.reshape(-1)
        else:
            buf[:, r0:r0 + H * W] = y.reshape(N, H * W, cout)
    return buf


@functools.lru_cache(maxsize=None)
def in_case(name, C, exact):
    """(sources, {"v": (reference, bound), "z": ...}) of an input-side case, computed once."""
    shapes = {n: s for n, s, _ in IN_CASES}[name]
    xs = in_operands(shapes, C, exact)
    if exact:
        check_exact(concat([ref_v(x, absolute=True) for x in xs]))
        check_exact(concat([ref_z(x, absolute=True) for x in xs]))
    return shapes, xs, {k: expect_in(xs, k) for k in ("v", "z")}


@functools.lru_cache(maxsize=None)
def out_case(name, cout, exact):
    """(shapes, operands, per problem (reference, bound)) of an output-side case, computed once."""
    shapes = {(n, c): s for n, s, c in OUT_CASES}[(name, cout)]
    ops = out_operands(name, shapes, cout, exact)
    want = [expect_out(name, shapes, ops, p) for p in range(len(shapes))]
    if exact:
        for _, _, mag in want:
            check_exact(mag)
    return shapes, ops, [(r, b) for r, b, _ in want]

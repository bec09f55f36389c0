"""CPU: what tests/glue_cases.py gives tests/test_gpu_glue.py is right.  Every float64 reference is held to torch's float64 functions (or
to a direct loop) at the case tables the GPU tests use, and every comparison is shown to REJECT a wrong answer: a small deliberate fault
is applied to the reference's own output and the comparison the GPU test makes must fail.  The float64-against-float64 checks use the
references' own bounds (they are of fp32 size, a float64 result lies far inside them) -- no tolerance here is a bare number either."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as gc

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
NCHW = lambda a: np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))
NHWC = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))
F64 = 2.0 ** -20                  # a float64 result lies at least this far inside a bound of fp32 size


# ---------------------------------------------------------------------------------------------- the comparisons themselves
def test_comparisons_reject():
    r = np.array([1.0, -2.0, 0.0])
    b = gc.nu(1) * np.abs(r)
    assert gc.within(r, r, b) and gc.within(r * (1 + gc.U), r, b)
    assert not gc.within(r * (1 + 3 * gc.U), r, b)
    assert not gc.within(r + np.array([0, 0, 1e-30]), r, b), "a zero bound asks for an exact zero"
    assert not gc.within(np.array([1.0, np.nan, 0.0]), r, b) and not gc.within(np.array([1.0, -2.0, np.inf]), r, np.inf)
    z = np.array([0.0, -0.0], dtype=np.float32)
    assert gc.same_values(z, z[::-1]) and not gc.same_bits(z, z[::-1].copy())
    assert not gc.same_values(np.array([np.nan]), np.array([np.nan]))


def test_bf16_rounding_against_torch_and_truncation_rejected():
    x = np.concatenate([gc.synth.normal((4096,), 5), np.array([0.0, -0.0, np.inf, -np.inf, 1.00390625, 1.01171875], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert gc.same_bits(gc.bf16_rne(x), want)
    assert gc.same_bits(gc.bf16_value(want), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert not gc.same_bits(gc.bf16_trunc(x), want), "a truncating store must differ on this table"
    # ... and on the pooled maxima the bf16 pool test uses
    for shape in gc.POOL:
        y, _ = gc.pool_ref(gc.pool_x(shape, fine=True))
        if y.size >= 16:
            assert not gc.same_bits(gc.bf16_trunc(y), gc.bf16_rne(y)), shape


# ---------------------------------------------------------------------------------------------- 1. packs, fold, Winograd weights
def pack_by_loop(w, kw_pad, c_pad, mode, scale, taps):
    """rn_pack_weights' contract written element by element (include/retinanet_mi355x.h)."""
    cout, cin, kh, kw = w.shape
    rows = cout if mode == 0 else cin
    nr, ns = (taps[1], taps[3]) if taps else (kh, kw_pad)
    out = np.zeros((rows, gc.kpad(nr * ns, c_pad)), dtype=np.float32)
    for row in range(rows):
        for i in range(nr):
            for j in range(ns):
                r, s = (taps[0] + 2 * i, taps[2] + 2 * j) if taps else (i, j)
                if s >= kw:
                    continue
                for c in range(cin if mode == 0 else cout):
                    v = w[row, c, r, s] if mode == 0 else w[c, row, r, s] * (np.float32(1) if scale is None else scale[c])
                    out[row, (i * ns + j) * c_pad + c] = v
    return out


@pytest.mark.parametrize("c", gc.PACK, ids=lambda c: c.name)
def test_pack_reference(c):
    w, scale = gc.pack_inputs(c)
    got = gc.pack_ref(w, c.kw_pad, c.c_pad, c.mode, scale, c.taps)
    assert got.shape[1] % 32 == 0 and gc.same_bits(got, pack_by_loop(w, c.kw_pad, c.c_pad, c.mode, scale, c.taps))


def test_pack_with_kw_pad_taken_as_kw_rejected():
    c = gc.PACK[0]
    assert c.kw_pad > c.kw
    w, scale = gc.pack_inputs(c)
    assert not gc.same_bits(gc.pack_ref(w, c.kw_pad, c.c_pad, c.mode, scale, c.taps, kw_taken=c.kw),
                            gc.pack_ref(w, c.kw_pad, c.c_pad, c.mode, scale, c.taps))


@pytest.mark.parametrize("C", gc.FOLD_C)
def test_fold_reference(C):
    """y = scale x + shift is eval-mode batch norm; rstd is 1 / sqrt(var + eps)."""
    gamma, beta, mean, var = gc.fold_inputs(C)
    if C > 1:
        assert (gamma == 0).any() and (gamma < 0).any() and set(var.tolist()) == {0.0, np.float32(1e-12), 1.0, 1e6}
        assert (mean > 0).any() and (mean < 0).any()
    (rstd, scale, shift), (b_rstd, b_scale, b_shift) = gc.fold_ref(gamma, beta, mean, var)
    x = T64(gc.synth.normal((3, C, 2, 2), 7, 2.0))
    eps = float(np.float32(gc.FOLD_EPS))
    want = F.batch_norm(x, T64(mean), T64(var), T64(gamma), T64(beta), False, 0.0, eps).numpy()
    got = x.numpy() * scale[None, :, None, None] + shift[None, :, None, None]
    mag = np.abs(x.numpy()) * np.abs(scale)[None, :, None, None] + (np.abs(beta.astype(np.float64)) + np.abs(mean * scale))[None, :, None, None]
    assert gc.within(got, want, gc.nu(1) * mag)
    assert gc.within(rstd, (T64(var) + eps).rsqrt().numpy(), b_rstd)
    # a fold that forgets eps is outside the bound wherever var is small
    if C > 1:
        with np.errstate(divide="ignore"):
            assert not gc.within(1.0 / np.sqrt(var.astype(np.float64)), rstd, b_rstd)


BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
              dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def wino_tile(Umat, d):
    """A^T [sum_k U[., row, k] (.) (B^T d[k] B)] A: Umat [36, rows, K], d [K, 6, 6] -> [rows, 4, 4]."""
    V = np.einsum("ia,kab,jb->ijk", BT, d, BT).reshape(36, -1)
    M = np.einsum("prk,pk->pr", Umat, V).reshape(6, 6, -1)
    return np.einsum("ai,ijr,bj->rab", AT, M, AT)


@pytest.mark.parametrize("cout,cin", gc.WINO_W)
def test_wino_weights_reference(cout, cin):
    """Mode 0 against F.conv2d through the Winograd identity; mode 1 (flipped, transposed, scaled) against the convolution's data
    gradient; padded columns zero; unflipped taps rejected."""
    w, scale = gc.wino_w_inputs(cout, cin)
    U0, b0 = gc.wino_weights_ref(w, 0)
    assert U0.shape == (36, cout, gc.kpad(1, cin)) and not U0[:, :, cin:].any() and not b0[:, :, cin:].any()
    d = gc.synth.normal((cin, 6, 6), 9).astype(np.float64)
    want = F.conv2d(T64(d)[None], T64(w)).numpy()[0]
    mag = F.conv2d(T64(np.abs(d))[None], T64(np.abs(w))).numpy()[0]
    assert gc.within(wino_tile(U0[:, :, :cin], d), want, gc.nu(1) * mag)
    for sc in (None, scale):
        U1, b1 = gc.wino_weights_ref(w, 1, sc)
        assert U1.shape == (36, cin, gc.kpad(1, cout)) and not U1[:, :, cout:].any()
        x = torch.zeros((1, cin, 8, 8), dtype=torch.float64, requires_grad=True)
        dy = gc.synth.normal((cout, 6, 6), 10).astype(np.float64)
        y = F.conv2d(x, T64(w))
        if sc is not None:
            y = y * T64(sc)[None, :, None, None]
        (y * T64(dy)[None]).sum().backward()
        want = x.grad.numpy()[0, :, 2:6, 2:6]
        mag = F.conv_transpose2d(T64(np.abs(dy))[None], T64(np.abs(w))).numpy()[0, :, 2:6, 2:6] * (1.0 if sc is None else np.abs(sc).max())
        assert gc.within(wino_tile(U1[:, :, :cout], dy), want, gc.nu(1) * mag)
        bad, _ = gc.wino_weights_ref(w, 1, sc, flip=False)
        assert not gc.within(bad, U1, b1), "taps not flipped must be outside the bound"
    # the scale changes the result by more than the bound allows: leaving it out is seen
    assert not gc.within(gc.wino_weights_ref(w, 1, None)[0], *gc.wino_weights_ref(w, 1, scale))


@pytest.mark.parametrize("cout,cin", gc.WINO_DW)
def test_wino_dw_reference(cout, cin):
    """G^T dU G is the weight gradient of the Winograd identity: dU = (A dY A^T) (.) (B^T d B) summed over nothing (one tile)."""
    d = gc.synth.normal((cin, 6, 6), 11).astype(np.float64)
    dY = gc.synth.normal((cout, 4, 4), 12).astype(np.float64)
    w = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    (F.conv2d(T64(d)[None], w)[0] * T64(dY)).sum().backward()
    V = np.einsum("ia,kab,jb->ijk", BT, d, BT)
    Z = np.einsum("ai,rab,bj->ijr", AT, dY, AT)
    dU = np.zeros((36, cout, gc.kpad(1, cin)), dtype=np.float32)
    dU64 = np.einsum("ijr,ijk->ijrk", Z, V).reshape(36, cout, cin)
    dU[:, :, :cin] = dU64                                   # (rounded to fp32: the reference takes fp32 operands)
    before = np.zeros((cout, gc.kpad(9, cin)), dtype=np.float32)
    got, bound = gc.wino_dw_ref(dU, before, cin)
    want = w.grad.numpy().transpose(0, 2, 3, 1).reshape(cout, 9 * cin)     # [co][r][s][ci]
    assert gc.within(got, want, bound)
    # the inputs the GPU test uses: NaN past Cin and past 9 Cin never reach the reference, and it ADDS
    dUn, dwn = gc.wino_dw_inputs(cout, cin)
    got, bound = gc.wino_dw_ref(dUn, dwn, cin)
    assert np.isfinite(got).all() and got.shape == (cout, 9 * cin)
    zero, _ = gc.wino_dw_ref(dUn, np.zeros_like(dwn), cin)
    assert not gc.within(zero, got, bound), "a store instead of an accumulation must be outside the bound"


def test_prep_block_counts():
    """The kernel's indexing: a chunk covers 256 threads; kind 5 a wave per row; kind 4 eight values per thread."""
    assert gc.prep_blocks(0, Cout=256) == 1 and gc.prep_blocks(0, Cout=257) == 2
    assert gc.prep_blocks(5, rows=1, Kpad=32) == 1 and gc.prep_blocks(5, rows=5, Kpad=96) == 2
    assert gc.prep_blocks(4, rows=6, Kpad=96) == 1 and gc.prep_blocks(4, rows=36 * 5, Kpad=32) == 3
    assert gc.prep_blocks(1, rows=5, Kpad=224) == 5 and gc.prep_blocks(3, rows=8, Kpad=32) == 1


# ---------------------------------------------------------------------------------------------- 2. unpack
@pytest.mark.parametrize("c", gc.UNPACK, ids=lambda c: c.name)
def test_unpack_reference(c):
    """The packed slots are pack_ref's (a packed weight unpacks to itself); dgamma / dbeta are autograd's for y = gamma (x - mean) rstd +
    beta folded into the convolution: d/dgamma = (sum w dw_packed - mean colsum) rstd with dw_packed the gradient of the FOLDED weight."""
    d = gc.unpack_inputs(c)
    w4 = d["w"].reshape(c.cout, c.cin, c.kh, c.kw)
    packed = gc.pack_ref(w4, c.kw_pad, c.c_pad, 0)
    assert packed.shape == d["wp"].shape
    real = np.isfinite(d["wp"])
    assert gc.same_bits(packed[real], d["wp"][real]) and not packed[~real].any() and np.isnan(d["dw"][~real]).all()
    assert real.sum() == c.cout * c.cin * c.kh * c.kw
    dweight, dgamma, bound = gc.unpack_ref(d)
    assert gc.same_bits(dweight, (T64(d["scale"]).float()[:, None] * torch.from_numpy(d["g"])).numpy())
    # autograd: L = sum_co [ sum_k (gamma rstd w)_k g_k + (beta - mean gamma rstd) colsum ]   (g = dL/d folded weight, colsum = dL/d shift)
    gamma = torch.ones(c.cout, dtype=torch.float64, requires_grad=True)
    beta = torch.zeros(c.cout, dtype=torch.float64, requires_grad=True)
    L = ((gamma * T64(d["rstd"]))[:, None] * T64(d["w"]) * T64(d["g"])).sum() + ((beta - T64(d["mean"]) * gamma * T64(d["rstd"])) * T64(d["colsum"])).sum()
    L.backward()
    assert gc.within(dgamma, gamma.grad.numpy(), bound) and gc.same_values(beta.grad.numpy(), d["colsum"].astype(np.float64))
    # channel 0 cancels: the two terms are of one size
    dot0 = float((d["w"][0].astype(np.float64) * d["g"][0]).sum())
    assert abs(dot0 - float(d["mean"][0]) * float(d["colsum"][0])) <= gc.nu(2) * abs(dot0)
    bad = gc.unpack_ref(d, drop_mean=True)[1]
    assert not gc.within(bad, dgamma, bound), "a dgamma without the mean * colsum term must be outside the bound"
    plain, _, _ = gc.unpack_ref(d, scaled=False)
    assert gc.same_bits(plain, d["g"])


# ---------------------------------------------------------------------------------------------- 3. pools
def pool_by_loop(x):
    N, H, W, C = x.shape
    Ho, Wo = gc.pool_out(H), gc.pool_out(W)
    y, arg = np.zeros((N, Ho, Wo, C), dtype=np.float32), np.zeros((N, Ho, Wo, C), dtype=np.uint8)
    for n in range(N):
        for oh in range(Ho):
            for ow in range(Wo):
                for c in range(C):
                    best, code = None, 0
                    for r in range(3):
                        for s in range(3):
                            ih, iw = 2 * oh - 1 + r, 2 * ow - 1 + s
                            if 0 <= ih < H and 0 <= iw < W and (best is None or x[n, ih, iw, c] > best):
                                best, code = x[n, ih, iw, c], 3 * r + s
                    y[n, oh, ow, c], arg[n, oh, ow, c] = best, code
    return y, arg


@pytest.mark.parametrize("shape", gc.POOL, ids=str)
def test_pool_forward_reference(shape):
    x = gc.pool_x(shape)
    y, arg = gc.pool_ref(x)
    assert gc.same_values(y, NHWC(F.max_pool2d(torch.from_numpy(NCHW(x)), 3, 2, 1).numpy()))
    if x.size <= 4096:
        yl, al = pool_by_loop(x)
        assert gc.same_bits(y, yl) and gc.same_bits(arg, al)
    fine = gc.pool_x(shape, fine=True)
    assert gc.same_bits(gc.pool_ref(fine)[0], NHWC(F.max_pool2d(torch.from_numpy(NCHW(fine)), 3, 2, 1).numpy()))


def test_pool_table_has_ties_negative_windows_and_signed_zeros():
    ties = neg = 0
    for shape in gc.POOL:
        x = gc.pool_x(shape)
        y, arg = gc.pool_ref(x)
        ties += int((gc.pool_ref(x, last=True)[1] != arg).sum())
        neg += int((y < 0).sum())
        assert shape[2] * shape[3] < 8 or (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    assert ties > 1000 and neg > 20


@pytest.mark.parametrize("shape", gc.POOL[1:], ids=str)
def test_pool_faults_rejected(shape):
    x = gc.pool_x(shape)
    y, arg = gc.pool_ref(x)
    assert not gc.same_bits(gc.pool_ref(x, last=True)[1], arg), "argmax taking the last maximum must differ"
    assert not gc.same_bits(gc.pool_ref(x, pad_value=0.0)[0], y), "padding counted as 0 must differ in an all-negative border window"


@pytest.mark.parametrize("shape", gc.POOL, ids=str)
def test_pool_backward_reference(shape):
    """Against autograd on tie-free inputs (with ties torch's choice of maximum is its own business); on the tied table against the direct
    scatter; the masks; a wrong argmax is outside the bound."""
    N, C, H, W = shape
    fine = gc.pool_x(shape, fine=True)
    _, arg = gc.pool_ref(fine)
    dy = gc.synth.normal(arg.shape, 13)
    xt = T64(NCHW(fine)).requires_grad_(True)
    (F.max_pool2d(xt, 3, 2, 1) * T64(NCHW(dy))).sum().backward()
    dx, bound = gc.pool_bwd_ref(arg, dy, H, W)
    assert gc.within(dx, NHWC(xt.grad.numpy()), bound)
    x = gc.pool_x(shape)
    _, arg = gc.pool_ref(x)
    dx, bound = gc.pool_bwd_ref(arg, dy, H, W)
    want = np.zeros((N, H, W, C))
    for idx in np.ndindex(*arg.shape):
        n, oh, ow, c = idx
        want[n, 2 * oh - 1 + int(arg[idx]) // 3, 2 * ow - 1 + int(arg[idx]) % 3, c] += float(dy[idx])
    assert gc.within(dx, want, bound) and not dx[bound == 0].any()
    keep = x > 0
    dxm, bm = gc.pool_bwd_ref(arg, dy, H, W, keep)
    assert gc.within(dxm, want * keep, bm) and not dxm[~keep].any() and not bm[~keep].any()
    assert not keep[x == 0].any(), "-0.0 and 0 are off the mask"
    if H * W > 1:
        _, arg_last = gc.pool_ref(x, last=True)
        assert not gc.within(gc.pool_bwd_ref(arg_last, dy, H, W)[0], dx, bound)


def test_sign_words():
    x = gc.pool_x(gc.POOL[-1])
    words = gc.sign_words(x)
    flat = x.reshape(-1)
    assert words.dtype == np.uint32 and words.size == flat.size // 32
    for i in range(flat.size):
        assert bool((int(words[i >> 5]) >> (i & 31)) & 1) == bool(flat[i] > 0)


# ---------------------------------------------------------------------------------------------- 4. FPN, head, small kernels
@pytest.mark.parametrize("case", gc.UPSAMPLE, ids=str)
@pytest.mark.parametrize("C", gc.UPSAMPLE_C)
def test_upsample_add_bwd_reference(case, C):
    (Hs, Ws), (Hd, Wd) = case
    for bf16 in (False, True):
        src, dst = gc.upsample_inputs(case, C, bf16=bf16)
        if bf16:
            assert gc.same_bits(src, gc.bf16_round(src)) and gc.same_bits(dst, gc.bf16_round(dst))
        small = torch.zeros((gc.UPSAMPLE_N, C, Hd, Wd), dtype=torch.float64, requires_grad=True)
        up = F.interpolate(small, scale_factor=2, mode="nearest")[..., :Hs, :Ws]
        (up * T64(NCHW(src))).sum().backward()
        got, bound = gc.upsample_add_bwd_ref(src, dst, bf16=bf16)
        assert gc.within(got, NHWC(small.grad.numpy()) + dst.astype(np.float64), bound)
        if Hs > 1 and Ws > 1:
            assert not gc.within(gc.upsample_add_bwd_ref(src, dst, bf16=bf16, crop=1)[0], got, bound), "a crop off by one must be outside the bound"
        if bf16:                                                   # the store's rounding, and truncation instead of it
            stored = gc.bf16_round(got.astype(np.float32))
            assert gc.within(stored, got, bound)


@pytest.mark.parametrize("C,ld", gc.SIGMOID)
def test_sigmoid_bwd_pad_reference(C, ld):
    B, rows = gc.SIGMOID_B, gc.SIGMOID_ROWS
    assert (B * rows * ld) % 256 != 0
    whole, dy, off, stride = gc.concat_slice(B, rows, C, 17)
    assert stride > rows * C and np.isnan(whole.reshape(B, -1)[:, :off]).all() and np.isnan(whole.reshape(B, -1)[:, off + rows * C:]).all()
    gc.signed_zeros(dy)
    s = gc.sigmoid_values((B, rows, C), 18)
    assert {0.0, 1.0, gc.SIG_LO, 1.0 - gc.SIG_LO} <= set(s.reshape(-1)[:13].astype(np.float64).tolist())
    assert (np.signbit(dy) & (dy == 0)).any() and (~np.signbit(dy) & (dy == 0)).any()
    # sigmoid's autograd gives s (1 - s): z = logit(s) where that is finite
    mid = (s > 0) & (s < 1)
    z = torch.logit(T64(s)[torch.from_numpy(mid)]).requires_grad_(True)
    (torch.sigmoid(z) * T64(dy)[torch.from_numpy(mid)]).sum().backward()
    got, bound = gc.sigmoid_bwd_pad_ref(dy, s, ld)
    assert got.shape == (B * rows, ld) and not got[:, C:].any() and not bound[:, C:].any()
    inner = got[:, :C].reshape(B, rows, C)
    assert gc.within(inner[mid], z.grad.numpy(), gc.nu(1) * np.abs(z.grad.numpy()))
    assert not inner[~mid].any() and not bound[:, :C].reshape(B, rows, C)[~mid].any()
    copy, b0 = gc.sigmoid_bwd_pad_ref(dy, None, ld)
    assert gc.same_values(copy[:, :C].reshape(B, rows, C), dy) and not b0.any()
    # a wrong batch stride reads the next rows: outside the bound
    shifted = np.roll(dy, 1, axis=1)
    assert not gc.within(gc.sigmoid_bwd_pad_ref(shifted, s, ld)[0], got, bound)
    # bf16: the rounded store is inside, the truncated one outside
    _, bb = gc.sigmoid_bwd_pad_ref(dy, s, ld, bf16=True)
    g32 = got.astype(np.float32)
    assert gc.within(gc.bf16_round(g32), got, bb)
    assert not gc.same_bits(gc.bf16_trunc(g32), gc.bf16_rne(g32))


@pytest.mark.parametrize("H,W,extra", [(9, 6, False), (4, 4, True)])
def test_flags_reference(H, W, extra):
    """The patch rule against the kernel's wording of it (own tile; the neighbour above iff the pixel is in its tile's first row and there
    is one, and so on), every pixel position once."""
    dy, s, pixels = gc.flags_inputs(H, W, 5, extra_empty=extra)
    TH, TW = (H + 3) // 4, (W + 3) // 4
    flags = gc.flags_ref(H, W, pixels)
    assert flags.shape == (len(pixels), TH, TW) and dy.shape[0] == len(pixels)
    assert [p for p in pixels if p is not None] == [(h, w) for h in range(H) for w in range(W)]
    for b, p in enumerate(pixels):
        nz = np.flatnonzero(dy[b].reshape(-1) != 0)
        if p is None:
            assert not flags[b].any() and (nz.size == 0 or s[b].reshape(-1)[nz[0]] == 1.0)
            continue
        assert nz.size == 1 and nz[0] // 5 == p[0] * W + p[1]
        want = np.zeros((TH, TW), dtype=np.uint8)
        th, tw, hi, wi = p[0] // 4, p[1] // 4, p[0] % 4, p[1] % 4
        for a in (-1, 0, 1):
            for e in (-1, 0, 1):
                rows_ok = a == 0 or (hi == 0 and th > 0 if a < 0 else hi == 3 and th + 1 < TH)
                cols_ok = e == 0 or (wi == 0 and tw > 0 if e < 0 else wi == 3 and tw + 1 < TW)
                if rows_ok and cols_ok:
                    want[th + a, tw + e] = 1
        assert gc.same_bits(flags[b], want), (b, p)
    assert (np.signbit(dy) & (dy == 0)).any()
    if TH * TW > 1:
        assert not gc.same_bits(gc.flags_ref(H, W, pixels, halo=False), flags), "a flag without its halo must differ"
    else:
        assert flags.reshape(-1)[1:len(pixels) - 3:2].sum() == 0, "the empty images between keep a neighbour's write visible"


@pytest.mark.parametrize("rows,C,ld", gc.COLSUM)
def test_colsum_reference(rows, C, ld):
    g, before = gc.colsum_inputs(rows, C, ld)
    assert np.isnan(g[:, C:]).all()
    s, bound = gc.colsum_ref(g, C)
    want = T64(g[:, :C]).sum(0).numpy()
    assert gc.within(s, want, gc.nu(1) * np.abs(g[:, :C].astype(np.float64)).sum(0) * F64)
    acc, bacc = gc.colsum_ref(g, C, before)
    assert gc.within(acc, want + before, bacc * F64)
    if rows >= 511:
        # a row left out (the tail loop's last one) is outside the bound
        assert not gc.within(gc.colsum_ref(g[:-1], C)[0], s, bound)
    if rows >= 511 and rows % 2 and C > 1:
        # column 0 sums to about 1e4, every other column to a few tens: an error of 1e-5 of the LARGEST sum in one of those -- what a
        # tolerance relative to the largest sum lets through -- is far outside their own bound
        assert np.abs(s[0]) == np.abs(s).max() and np.abs(s[0]) > 100 * np.abs(s[1:]).max()
        off = s.copy()
        off[1] += 1e-5 * np.abs(s).max()
        assert not gc.within(off, s, bound)


def test_small_elementwise_references():
    for n in gc.RELU_BF16_N:
        b = gc.relu_bf16_inputs(n)
        v = gc.bf16_value(b)
        assert np.isinf(v).sum() == 2 and (v == 0).sum() >= 2 and gc.same_bits(gc.bf16_rne(v), b)
    for N, H, W in gc.NHWC4:
        img = gc.synth.normal((N, 3, H, W), 21)
        out = gc.nhwc4_ref(img)
        assert gc.same_bits(out[..., :3], torch.from_numpy(img).permute(0, 2, 3, 1).contiguous().numpy())
        assert gc.same_bits(out[..., 3], np.zeros((N, H, W), dtype=np.float32))
    assert sorted(N * H * W for N, H, W in gc.NHWC4) == [255, 256, 257, 260]


# ---------------------------------------------------------------------------------------------- 5. clip + Adam
@pytest.mark.parametrize("grad_scale,mult", [(1.0, 1.0), (0.25, 4.0)])
def test_optimizer_reference_against_torch(grad_scale, mult):
    """Three steps of the per-step reference, chained in float64, against clip_grad_norm_ + torch.optim.Adam in float64 on the scaled
    gradients; the clip is off in steps 1 and 3 and on in step 2; a chunk left out of the norm is rejected."""
    hp = gc.OPT_HP
    assert len(gc.opt_chunks(gc.OPT_SIZES)) == 1103
    params = [torch.nn.Parameter(T64(p)) for p in gc.opt_params()]
    # the fp32 values of the hyper-parameters, as the kernels see them
    opt = torch.optim.Adam(params, lr=float(gc.f32(hp["lr"])), betas=(float(gc.f32(hp["beta1"])), float(gc.f32(hp["beta2"]))), eps=float(gc.f32(hp["eps"])))
    state = [(p.astype(np.float64), np.zeros(p.size), np.zeros(p.size)) for p in gc.opt_params()]
    for step in range(3):
        grads = gc.opt_grads(step, mult)
        norm, nb = gc.opt_norm_ref(grads, grad_scale)
        for p, g in zip(params, grads):
            p.grad = T64(g) * grad_scale
        tn = float(torch.nn.utils.clip_grad_norm_(params, float(gc.f32(hp["max_norm"]))))
        assert gc.within(norm, tn, nb * F64)
        assert (norm > hp["max_norm"]) == (step == 1), "step 2 alone is clipped"
        opt.step()
        state = chain_step(state, grads, norm, step + 1, grad_scale)
        worst = max(gc.worst(s[0], p.detach().numpy(), gc.nu(1) * np.abs(s[0])) for s, p in zip(state, params))
        assert worst <= 1.0, (step, worst)
        for k in (1023, 1024, 1099, 1100, 1102):
            assert not gc.within(gc.opt_norm_ref(grads, grad_scale, skip_chunk=k)[0], norm, nb), "chunk %d left out must be outside the bound" % k


def chain_step(state, grads, norm, step, grad_scale):
    """opt_step_ref from a float64 state: its fp32 casts of p, m, v are bypassed by feeding the float64 arrays through the same formulas."""
    out = []
    for (p, m, v), g in zip(state, grads):
        r = step_f64(p, g, m, v, norm, step, grad_scale)
        out.append(r)
    return out


def step_f64(p, g, m, v, norm, step, grad_scale):
    """The formulas of gc.opt_step_ref on float64 state (no fp32 cast between steps), checked against it on fp32-representable state."""
    hp = gc.OPT_HP
    lr, b1, b2, eps, mn = (gc.f32(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "max_norm"))
    gs = gc.f32(grad_scale)
    coef = min(1.0, mn / (norm + gc.f32(1e-6))) * gs
    g1 = g.astype(np.float64) * coef
    m1 = b1 * m + (1.0 - b1) * g1
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    p1 = p - (lr / (1.0 - b1 ** step)) * (m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** step) + eps))
    return p1, m1, v1


def test_optimizer_step_reference_is_the_chained_formula():
    """gc.opt_step_ref (fp32 state in, one step) equals the chained formula on the same state; its bounds are positive where they must be."""
    p, g = gc.synth.normal((4097,), 31, 0.5), gc.synth.normal((4097,), 32, 10.0)
    m, v = gc.synth.normal((4097,), 33, 0.1), np.abs(gc.synth.normal((4097,), 34, 0.01))
    norm = np.float32(gc.opt_norm_ref([g])[0])
    for gs in (1.0, 0.25):
        r = gc.opt_step_ref(p, g, m, v, norm, 2, gs)
        p1, m1, v1 = step_f64(p.astype(np.float64), g, m.astype(np.float64), v.astype(np.float64), float(norm), 2, gs)
        for key, want in (("p", p1), ("m", m1), ("v", v1)):
            assert gc.within(r[key][0], want, r[key][1] * F64), key
            assert (r[key][1] > 0).all()
        assert gc.within(r["g"][0], g.astype(np.float64) * min(1.0, gc.f32(0.1) / (float(norm) + gc.f32(1e-6))) * gs, r["g"][1] * F64)
    # a clip that is skipped is outside every bound
    r = gc.opt_step_ref(p, g, m, v, norm, 2, 1.0)
    free = gc.opt_step_ref(p, g, m, v, np.float32(1e-3), 2, 1.0)
    assert not gc.within(free["g"][0], *r["g"]) and not gc.within(free["m"][0], *r["m"]) and not gc.within(free["v"][0], *r["v"])

"""Cases, float64 references and allocators for the fp32 weight gradient's launch paths (csrc/conv_wgrad.hip: wgrad_launch).  CPU only:
tests/test_wgrad_cases_host.py proves what is here, tests/test_gpu_wgrad_paths.py holds the kernels to it.

A case is one problem; what it EXPECTS of rn_conv_wgrad_plan (tile shape, xcd_map, kernel, slice length ...) is part of the case, so a
retuning of the launcher that moves a case off the path it is named for fails that case by name.

Layouts as the C ABI's: x [N, Hi, Wi, Cin], dy [N, Ho, Wo, ldy >= Cout], dw [Cout][kh][kw][Cin] (the packed row, padded to Kpad = a multiple
of 32), colsum [Cout].  kw may exceed the tap count of the convolution (the stem's 7 x 7 runs with kw = 8): the output size follows from
k = kh, the extra tap is computed like any other (the packed weight's column there is zero; the gradient's is not)."""
import collections

import torch

Case = collections.namedtuple("Case", "name cin cout k stride pad N H W kw ldy relu expect")


def case(name, cin, cout, k, stride, pad, N, H, W, kw=None, ldy=None, relu=False, **expect):
    return Case(name, cin, cout, k, stride, pad, N, H, W, kw or k, ldy or cout, relu, expect)


# expect: shape (0: 64 x 256, 1: 256 x 64, 2: 128 x 128), xcd_map, once (the 128 x 128 tile's kernel of the split modes), surplus (final
# slices not a multiple of 8 under xcd_map: padding workgroups leave at slice >= splits), per_split_over / per_split_is, pixels.
LARGE = [
    # 144 tiles, slices rounded up to 16, 704 pixels = 44 K-steps = three pixel-table batches per slice
    case("xcd-512-512-3x3-60x60", 512, 512, 3, 1, 1, 3, 60, 60, shape=2, xcd_map=1, once=True, per_split_over=512),
    # 54 tiles; 39 slices (native) and 31 (split modes) in 40 and 32 workgroup groups: the padding group's return in EVERY mode, where
    # 256 -> 512 at 18500 pixels reaches it in native mode only (31 against 24 slices) at the same 43.6 GFLOP
    case("xcd-surplus-256-384-3x3-70x88", 256, 384, 3, 1, 1, 4, 70, 88, shape=2, xcd_map=1, once=True, surplus=True, per_split_over=512),
    # 896 pixels = 56 K-steps = four table batches: both table slots are reused
    case("four-batches-512-512-3x3-59x59", 512, 512, 3, 1, 1, 4, 59, 59, shape=2, xcd_map=1, once=True, per_split_over=768),
]
RELU = [
    case("relu-64-64-3x3", 64, 64, 3, 1, 1, 2, 40, 40, relu=True, shape=0, once=False),
    case("relu-64-256-1x1", 64, 256, 1, 1, 0, 2, 40, 40, relu=True, shape=1, once=False),
    case("relu-128-128-3x3", 128, 128, 3, 1, 1, 2, 40, 40, relu=True, shape=2, once=True),
]
SWITCH = [
    case("cout-64", 64, 64, 3, 1, 1, 2, 13, 17, shape=0),
    case("cout-65", 64, 65, 3, 1, 1, 2, 13, 17, ldy=68, shape=2),
    case("kflat-64", 64, 128, 1, 1, 0, 2, 13, 17, shape=1),
    case("kflat-68", 68, 128, 1, 1, 0, 2, 13, 17, shape=2),
    case("cout-1", 64, 1, 3, 1, 1, 2, 13, 17, ldy=4, shape=0),
    case("cin-4", 4, 128, 3, 1, 1, 2, 13, 17, shape=1),
]
PIXELS = [
    case("pixels-1", 128, 128, 1, 1, 0, 1, 1, 1, shape=2, pixels=1),
    case("pixels-15", 128, 128, 1, 1, 0, 1, 3, 5, shape=2, pixels=15),
    case("pixels-16", 128, 128, 1, 1, 0, 2, 2, 4, shape=2, pixels=16),
    case("pixels-17", 128, 128, 1, 1, 0, 1, 1, 17, shape=2, pixels=17),
    case("pixels-512-one-slice", 128, 128, 1, 1, 0, 1, 16, 32, shape=2, pixels=512, per_split_is=512, splits=1),
    case("pixels-513-two-slices", 128, 128, 1, 1, 0, 1, 19, 27, shape=2, pixels=513, splits=2),
    # 512 pixels are one slice of exactly per_split pixels; one more and the range is cut in two (the 513-pixel plan: 2 x 288, the second
    # slice 225 pixels).  288 and 289 pixels: a single slice that ends on a K-step and one pixel into the next.
    case("pixels-288", 128, 128, 1, 1, 0, 1, 12, 24, shape=2, pixels=288, per_split_is=288, splits=1),
    case("pixels-289", 128, 128, 1, 1, 0, 1, 17, 17, shape=2, pixels=289, splits=1),
    case("image-1x1-under-3x3", 128, 128, 3, 1, 1, 3, 1, 1, shape=2, pixels=3),
]
STRIDE = [
    case("s2-3x3-17x21", 128, 128, 3, 2, 1, 2, 17, 21, shape=2),
    case("s2-3x3-18x20", 128, 128, 3, 2, 1, 2, 18, 20, shape=2),
    case("s2-1x1-17x15", 256, 128, 1, 2, 0, 2, 17, 15, shape=2),
    case("stem-7x7-s2-kw8", 4, 64, 7, 2, 3, 2, 37, 45, kw=8, shape=0),
]
LDY = [
    case("ldy-108-128", 256, 108, 3, 1, 1, 1, 9, 15, ldy=128, shape=2),
    case("ldy-72-96", 256, 72, 3, 1, 1, 2, 11, 14, ldy=96, shape=2),
]
DENSE = LARGE + RELU + SWITCH + PIXELS + STRIDE + LDY
ONEHOT = [
    case("onehot-128-128-3x3-s1", 128, 128, 3, 1, 1, 3, 23, 29, shape=2, once=True),
    case("onehot-64-64-3x3-s2", 64, 64, 3, 2, 1, 3, 23, 29, shape=0, once=False),
    LARGE[0]._replace(name="onehot-" + LARGE[0].name),
]
BY_NAME = {c.name: c for c in DENSE + ONEHOT}
assert len(BY_NAME) == len(DENSE) + len(ONEHOT)

# the batched form (the Winograd weight gradient's 36 positions, here 3): flat 1 x 1 problems of T pixels, operands of entry b at b * stride;
# from 64 channels on the 256 x 64 tile, from 128 on the 128 x 128 tile (the once kernel in the split modes: what the Winograd layers run)
BATCHED = {cin: dict(nbatch=3, T=700, Tpad=704, cin=cin, cout=128, kpad=cin, gap=64, colsum_batch=2, shape=shape)
           for cin, shape in ((64, 1), (128, 2))}

TOL = 2e-5                       # of the reference's max magnitude, dw and colsum (tests/test_gpu_conv.py::test_wgrad_long_k's bound)
SENTINEL = 12345.0               # columns Kflat .. Kpad of dw and the gaps between batch entries
GUARD = 4096                     # floats of NaN before and after a guarded tensor


def out_hw(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def pixels(c):
    ho, wo = out_hw(c)
    return c.N * ho * wo


def kflat(c):
    return c.k * c.kw * c.cin


def kpad(c):
    return (kflat(c) + 31) // 32 * 32


def geom(c):
    """The geometry arguments of rn_conv_wgrad_batched from N on."""
    ho, wo = out_hw(c)
    return (c.N, c.H, c.W, c.cin, ho, wo, c.cout, c.k, c.kw, c.stride, c.pad, int(c.relu))


def _gen(name, salt):
    return torch.Generator().manual_seed((sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 31 + salt) % (2 ** 31))


def inputs(c):
    """-> (x [N,H,W,Cin], dy [N,Ho,Wo,ldy]) fp32, standard normal (x about half negative); the columns Cout .. ldy of dy are random too, at
    the data's scale: in split3 mode the amax words legitimately cover them, a product that leaked them would be O(1) wrong."""
    ho, wo = out_hw(c)
    x = torch.randn((c.N, c.H, c.W, c.cin), generator=_gen(c.name, 1))
    dy = torch.randn((c.N, ho, wo, c.ldy), generator=_gen(c.name, 2))
    return x, dy


def taps(x, c, relu=None):
    """Yields (r, s, float64 [N*Ho*Wo, Cin]): the input pixel each output pixel meets under tap (r, s), zero outside the image."""
    ho, wo = out_hw(c)
    xd = x.double()
    if c.relu if relu is None else relu:
        xd = xd.clamp_min(0.0)
    need_h, need_w = (ho - 1) * c.stride + c.k, (wo - 1) * c.stride + c.kw
    xp = torch.zeros((c.N, max(need_h, c.H + c.pad), max(need_w, c.W + c.pad), c.cin), dtype=torch.float64)
    xp[:, c.pad:c.pad + c.H, c.pad:c.pad + c.W] = xd
    for r in range(c.k):
        for s in range(c.kw):
            v = xp[:, r:r + (ho - 1) * c.stride + 1:c.stride, s:s + (wo - 1) * c.stride + 1:c.stride]
            yield r, s, v.reshape(-1, c.cin)


def reference(x, dy, c):
    """float64 (dw [Cout, kh, kw, Cin], colsum [Cout]): im2col(x)^T dy as one GEMM per tap."""
    g = dy[..., :c.cout].double().reshape(-1, c.cout)
    gt = g.t().contiguous()
    dw = torch.zeros((c.cout, c.k, c.kw, c.cin), dtype=torch.float64)
    for r, s, v in taps(x, c):
        dw[:, r, s] = gt @ v
    return dw, g.sum(0)


def onehot_dw(x, c, hot, dtype=torch.float32):
    """Closed form for dy = 0 except value g at (pixel p, channel ch), hot = [(p, ch, g)] with distinct channels:
    dw[ch][r][s][:] = g * x[n, oh*stride - pad + r, ow*stride - pad + s, :], exactly 0 where the tap is outside the image and in every
    other row.  In `dtype` arithmetic: float32 gives the one rounding the fp32 matrix core makes on the single product."""
    ho, wo = out_hw(c)
    assert len({ch for _, ch, _ in hot}) == len(hot)
    xs = x.to(dtype)
    if c.relu:
        xs = xs.clamp_min(0)
    dw = torch.zeros((c.cout, c.k, c.kw, c.cin), dtype=dtype)
    for p, ch, g in hot:
        n, rem = divmod(p, ho * wo)
        oh, ow = divmod(rem, wo)
        for r in range(c.k):
            for s in range(c.kw):
                ih, iw = oh * c.stride - c.pad + r, ow * c.stride - c.pad + s
                if 0 <= ih < c.H and 0 <= iw < c.W:
                    dw[ch, r, s] = torch.tensor(g, dtype=dtype) * xs[n, ih, iw]
    return dw


def seam_pixels(per_split, howo, npix):
    """Output pixels at the places a K slice plan can lose or repeat one: both ends of the range, both sides of the first two slice seams,
    both sides of the first image seam, both ends of the last slice.  Sorted, distinct, all < npix."""
    cand = [0, npix - 1, per_split - 1, per_split, 2 * per_split - 1, 2 * per_split, howo - 1, howo]
    last = (npix - 1) // per_split * per_split
    cand += [last, npix - 1]
    return sorted({p for p in cand if 0 <= p < npix})


def onehot_inputs(c, per_split):
    """-> (x, dy, hot): x = +-2^u, u uniform in (-6, 2) -- every element within 2^-8 of the tensor's maximum, inside the 2^-18 down to which
    the fp16 two-term split keeps 22 significand bits (csrc/mfma_split.h) --, dy zero but one value per seam pixel, each in its own channel."""
    ho, wo = out_hw(c)
    g = _gen(c.name, 3)
    mag = torch.exp2(torch.rand((c.N, c.H, c.W, c.cin), generator=g) * 8 - 6)
    x = torch.where(torch.rand(mag.shape, generator=g) < 0.5, -mag, mag)
    px = seam_pixels(per_split, ho * wo, pixels(c))
    assert len(px) <= c.cout
    hot = [(p, (5 + 6 * i) % c.cout, (-1.0) ** i * (1.0 + 0.125 * (i + 1))) for i, p in enumerate(px)]
    dy = torch.zeros((c.N, ho, wo, c.ldy))
    flat = dy.view(-1, c.ldy)
    for p, ch, val in hot:
        flat[p, ch] = val
    return x, dy, hot


def guarded(t, device=None):
    """-> (buffer, view): t copied into the middle of a larger buffer with GUARD NaNs before and after it; the view is contiguous, so a
    consumer that takes the amax of the tensor sees only the tensor.  A read outside the tensor turns the result NaN."""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=t.dtype)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    if device is not None:
        buf = buf.to(device)
    return buf, buf[GUARD:GUARD + t.numel()].view(t.shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def start_dw(c, zero=False):
    """dw [Cout, Kpad] before the call: random nonzero D0 in the packed row (zero: 0.0), SENTINEL in the columns Kflat .. Kpad; colsum [Cout]."""
    g = _gen(c.name, 4)
    dw = torch.full((c.cout, kpad(c)), SENTINEL)
    dw[:, :kflat(c)] = 0.0 if zero else torch.randn((c.cout, kflat(c)), generator=g) + 3.0
    return dw, torch.randn(c.cout, generator=g) - 3.0


_CACHE = {}


def get(name):
    """(case, x, dy, dw_ref [Cout, Kflat] float64, colsum_ref) of a dense case, computed once per process."""
    if name not in _CACHE:
        c = BY_NAME[name]
        x, dy = inputs(c)
        dw, cs = reference(x, dy, c)
        _CACHE[name] = (c, x, dy, dw.reshape(c.cout, -1), cs)
    return _CACHE[name]


def batched_inputs(cin):
    """A batched case: dy [nbatch][Tpad][cout] and x [nbatch][Tpad][cin] with the rows T .. Tpad of every entry NaN (no pixel past T may
    be read), and the float64 (dw [nbatch, cout, cin], colsum of entry colsum_batch)."""
    b = BATCHED[cin]
    g = _gen("batched", cin)
    dy = torch.full((b["nbatch"], b["Tpad"], b["cout"]), float("nan"))
    x = torch.full((b["nbatch"], b["Tpad"], b["cin"]), float("nan"))
    dy[:, :b["T"]] = torch.randn((b["nbatch"], b["T"], b["cout"]), generator=g)
    x[:, :b["T"]] = torch.randn((b["nbatch"], b["T"], b["cin"]), generator=g)
    gd, xd = dy[:, :b["T"]].double(), x[:, :b["T"]].double()
    return x, dy, torch.einsum("btm,btc->bmc", gd, xd), gd[b["colsum_batch"]].sum(0)


def check_plan(c, plan, split_mode):
    """The plan rn_conv_wgrad_plan reports is the path the case is named for; -> list of complaints."""
    e, bad = c.expect, []
    if plan is None:
        return ["refused"]
    if "shape" in e and plan["shape"] != e["shape"]:
        bad.append("tile shape %d, case wants %d" % (plan["shape"], e["shape"]))
    if "xcd_map" in e and plan["xcd_map"] != e["xcd_map"]:
        bad.append("xcd_map %d" % plan["xcd_map"])
    if "once" in e and plan["kernel"] != int(e["once"] and split_mode):
        bad.append("kernel %d" % plan["kernel"])
    if e.get("surplus") and not (plan["xcd_map"] == 1 and plan["splits"] % 8 != 0 and plan["grid"] > plan["tiles"] * plan["splits"]):
        bad.append("no padding workgroups: %d slices" % plan["splits"])
    if "per_split_over" in e and not plan["per_split"] > e["per_split_over"]:
        bad.append("per_split %d" % plan["per_split"])
    if "per_split_is" in e and plan["per_split"] != e["per_split_is"]:
        bad.append("per_split %d" % plan["per_split"])
    if "splits" in e and plan["splits"] != e["splits"]:
        bad.append("%d slices" % plan["splits"])
    if "pixels" in e and pixels(c) != e["pixels"]:
        bad.append("%d pixels" % pixels(c))
    return bad

"""Cases, exact references and allocators for the bf16 weight gradient's launch paths (csrc/conv_wgrad_bf16.hip: rn_conv_wgrad_bf16 and
rn_conv_wgrad_bf16_grouped).  CPU only: tests/test_wgrad_plan_host.py holds the slice planner (csrc/conv_wgrad_plan.h) to the plans
recorded here, tests/test_gpu_wgrad_bf16_paths.py runs the kernels.

Inputs are small integers -- dy and x drawn from {-2 .. 2}, stored as bf16 --, so every product and every partial sum is an integer
below 2^24 (4 x pixels < 2^24) and exact in fp32 whatever the order of the atomics: dw and colsum must EQUAL the float64 reference.  A
dropped, repeated or misplaced slice, pixel or tap is an integer error.

Layouts as the C ABI's: x [N, Hi, Wi, Cin] bf16, dy [N, Ho, Wo, ldy >= Cout] bf16, dw fp32 [Cout][Kpad] (Kpad = kh * kw * Cin rounded up
to 32), colsum fp32 [Cout].

PLAN holds, per case, what the launcher's planner decides: (tiles, K slices, pixels per slice, xcd_map, workgroups), at the default
target of 768 workgroups.  It was RECORDED ON THE PARENT of the commit that introduced conv_wgrad_plan.h, from wgrad_bf16_fill's own
arithmetic, so the shared planner is held to what the launcher did before; a retuning of the planner changes these rows knowingly."""
import collections

import torch

Case = collections.namedtuple("Case", "name cin cout k stride pad N H W ldy")
TARGET_WGS = 768                 # rn_conv_wgrad_bf16's default (RN_WGRAD_BF16_WGS unset)


def case(name, cin, cout, k, stride, pad, N, H, W, ldy=None):
    return Case(name, cin, cout, k, stride, pad, N, H, W, ldy or cout)


CASES = [
    # 4 tiles, 9 slices of 512 pixels in 16-slot groups of the XCD order: the padding group's early return
    case("xcd-surplus-256-256-1x1-48x48", 256, 256, 1, 1, 0, 2, 48, 48),
    # one tile, four slices, the plain order
    case("plain-128-128-1x1-40x40", 128, 128, 1, 1, 0, 1, 40, 40),
    # 36 tiles, 832 pixels = 26 K-steps = four pixel-table batches per slice: both table slots are refilled
    case("table-reuse-128-512-3x3-94x94", 128, 512, 3, 1, 1, 2, 94, 94),
    # one tile; a slice that ends on a K-step and one pixel into the next, below and above one slice
    case("pixels-1", 128, 128, 1, 1, 0, 1, 1, 1),
    case("pixels-31", 128, 128, 1, 1, 0, 1, 1, 31),
    case("pixels-32", 128, 128, 1, 1, 0, 2, 4, 4),
    case("pixels-33", 128, 128, 1, 1, 0, 1, 3, 11),
    case("pixels-511", 128, 128, 1, 1, 0, 1, 7, 73),
    case("pixels-512", 128, 128, 1, 1, 0, 1, 16, 32),
    case("pixels-513", 128, 128, 1, 1, 0, 1, 19, 27),
    # edges of the matrix: rows past Cout inside ldy, a second M tile of two rows, Kflat = 360 (chunks that straddle a tap, a last N
    # tile of 104 columns)
    case("cout-72-ldy-96", 64, 72, 3, 1, 1, 2, 11, 14, ldy=96),
    case("cout-130", 64, 130, 3, 1, 1, 2, 11, 14, ldy=136),
    case("cin-40-3x3", 40, 64, 3, 1, 1, 2, 11, 14),
    case("s2-3x3-17x21", 64, 64, 3, 2, 1, 2, 17, 21),
    case("s2-3x3-18x20", 64, 64, 3, 2, 1, 2, 18, 20),
    case("s2-1x1-17x15", 64, 64, 1, 2, 0, 2, 17, 15),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# name -> (tiles, splits, per_split, xcd_map, workgroups); recorded on the parent (see above)
PLAN = {
    "xcd-surplus-256-256-1x1-48x48": (4, 9, 512, 1, 64),
    "plain-128-128-1x1-40x40": (1, 4, 416, 0, 4),
    "table-reuse-128-512-3x3-94x94": (36, 22, 832, 1, 864),
    "pixels-1": (1, 1, 32, 0, 1),
    "pixels-31": (1, 1, 32, 0, 1),
    "pixels-32": (1, 1, 32, 0, 1),
    "pixels-33": (1, 1, 64, 0, 1),
    "pixels-511": (1, 1, 512, 0, 1),
    "pixels-512": (1, 1, 512, 0, 1),
    "pixels-513": (1, 2, 288, 0, 2),
    "cout-72-ldy-96": (5, 1, 320, 0, 5),
    "cout-130": (10, 1, 320, 0, 10),
    "cin-40-3x3": (3, 1, 320, 0, 3),
    "s2-3x3-17x21": (5, 1, 224, 0, 5),
    "s2-3x3-18x20": (5, 1, 192, 0, 5),
    "s2-1x1-17x15": (1, 1, 160, 0, 1),
}

# Grouped launches: the pyramid levels of one 3x3, 64 -> 64 layer (5 tiles), N = 2, with column sums.  Per level: (H, W).
#   share-zero: the smallest level's share of the target, 768 * 24 / 20114, rounds to ZERO slices, so it takes one; its 5 workgroups are
#       padded to 8 (ids 5 .. 7: slice >= splits under the plain order); the largest level runs in the XCD order.
#   pyramid: the sizes of a 264 x 480 frame's levels; again the first level in the XCD order, the others plain and padded.
GROUPS = {
    "share-zero": dict(cin=64, cout=64, k=3, stride=1, pad=1, N=2, levels=[(72, 130), (17, 30), (9, 15), (5, 8), (3, 4)]),
    "pyramid": dict(cin=64, cout=64, k=3, stride=1, pad=1, N=2, levels=[(33, 60), (17, 30), (9, 15), (5, 8), (3, 4)]),
}
# group -> per level (share of the target, tiles, splits, per_split, xcd_map, workgroups incl. padding); recorded on the parent
GROUP_PLAN = {
    "share-zero": [(714, 5, 37, 512, 1, 200), (38, 5, 2, 512, 0, 16), (10, 5, 1, 288, 0, 8), (3, 5, 1, 96, 0, 8), (0, 5, 1, 32, 0, 8)],
    "pyramid": [(568, 5, 8, 512, 1, 40), (146, 5, 2, 512, 0, 16), (38, 5, 1, 288, 0, 8), (11, 5, 1, 96, 0, 8), (3, 5, 1, 32, 0, 8)],
}

SENTINEL = 12345.0               # columns Kflat .. Kpad of dw
GUARD = 4096                     # elements of NaN before and after a guarded tensor


def out_hw(c, H=None, W=None):
    H, W = c.H if H is None else H, c.W if W is None else W
    return (H + 2 * c.pad - c.k) // c.stride + 1, (W + 2 * c.pad - c.k) // c.stride + 1


def pixels(c):
    ho, wo = out_hw(c)
    return c.N * ho * wo


def kflat(c):
    return c.k * c.k * c.cin


def kpad(c):
    return (kflat(c) + 31) // 32 * 32


def tiles(c):
    return ((c.cout + 127) // 128) * ((kflat(c) + 127) // 128)


def planner_row(c, target=TARGET_WGS, pad8=False):
    """The planner's inputs for a case: pixels tiles target wk ldy elem_bytes HoWo img_bytes policy xcd_enabled pad8 (conv_wgrad_plan.h)."""
    ho, wo = out_hw(c)
    return (pixels(c), tiles(c), target, 32, c.ldy, 2, ho * wo, c.H * c.W * c.cin * 2, 1, 1, int(pad8))


def group_cases(name):
    """The levels of a group as single cases, with each level's share of the target as rn_conv_wgrad_bf16_grouped computes it."""
    g = GROUPS[name]
    cs = [case("%s-L%d" % (name, i), g["cin"], g["cout"], g["k"], g["stride"], g["pad"], g["N"], h, w) for i, (h, w) in enumerate(g["levels"])]
    total = sum(pixels(c) for c in cs)
    return cs, [TARGET_WGS * pixels(c) // total for c in cs]


def _gen(name, salt):
    return torch.Generator().manual_seed((sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 31 + salt) % (2 ** 31))


def inputs(c):
    """-> (x [N,H,W,Cin], dy [N,Ho,Wo,ldy]) float32 holding integers of {-2 .. 2} (exact in bf16); the columns Cout .. ldy of dy too: a
    product that leaked them would be an integer error."""
    ho, wo = out_hw(c)
    x = torch.randint(-2, 3, (c.N, c.H, c.W, c.cin), generator=_gen(c.name, 1)).float()
    dy = torch.randint(-2, 3, (c.N, ho, wo, c.ldy), generator=_gen(c.name, 2)).float()
    return x, dy


def reference(x, dy, c):
    """float64 (dw [Cout, Kflat], colsum [Cout]) on the tensors' device: one GEMM per tap, every value an integer below 2^24 -- exact."""
    ho, wo = out_hw(c)
    assert 4 * pixels(c) < 2 ** 24
    g = dy[..., :c.cout].double().reshape(-1, c.cout)
    gt = g.t().contiguous()
    need_h, need_w = (ho - 1) * c.stride + c.k, (wo - 1) * c.stride + c.k
    xp = torch.zeros((c.N, max(need_h, c.H + c.pad), max(need_w, c.W + c.pad), c.cin), dtype=torch.float64, device=x.device)
    xp[:, c.pad:c.pad + c.H, c.pad:c.pad + c.W] = x.double()
    dw = torch.zeros((c.cout, c.k, c.k, c.cin), dtype=torch.float64, device=x.device)
    for r in range(c.k):
        for s in range(c.k):
            v = xp[:, r:r + (ho - 1) * c.stride + 1:c.stride, s:s + (wo - 1) * c.stride + 1:c.stride]
            dw[:, r, s] = gt @ v.reshape(-1, c.cin)
    return dw.reshape(c.cout, -1), g.sum(0)


def guarded(t, device=None):
    """-> (buffer, view): t in the middle of a larger buffer with GUARD NaNs before and after it."""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=t.dtype)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    if device is not None:
        buf = buf.to(device)
    return buf, buf[GUARD:GUARD + t.numel()].view(t.shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def start_dw(c):
    """dw [Cout, Kpad] before the call: small integers in the packed row (the kernel ADDS to them), SENTINEL in the columns Kflat .. Kpad;
    colsum [Cout] likewise integers."""
    g = _gen(c.name, 4)
    dw = torch.full((c.cout, kpad(c)), SENTINEL)
    dw[:, :kflat(c)] = torch.randint(-3, 4, (c.cout, kflat(c)), generator=g).float()
    return dw, torch.randint(-3, 4, (c.cout,), generator=g).float()

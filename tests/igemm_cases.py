"""Cases, the float64 reference and the expected launch paths for the fp32 forward / data-gradient convolutions: rn_conv_igemm,
rn_conv_igemm_splitk and rn_conv_igemm_grouped (csrc/conv_igemm.hip, conv_igemm_split.hip, conv_igemm_mf16.hip, conv_igemm_splitk.hip).
CPU only (numpy): tests/test_igemm_cases_host.py proves the reference against torch's float64 convolutions and the expected paths against
the launchers' own answer (rn_conv_igemm_plan is host code); tests/test_gpu_igemm_paths.py runs every case on every path it names.

The reference is the definition of rn_conv_desc in include/retinanet_mi355x.h, written as a gather over (n, oh, ow, r, s):
    nh = oh*a + p + r*b, nw = ow*a + p_w + s*b; the tap counts iff nh, nw >= 0, both are multiples of 1 << div_shift and
    nh >> div_shift < Hi, nw >> div_shift < Wi;  v = scale*acc + shift;  mask_mode 1: v = mask > 0 ? v : 0;  v += add (+ add2 where the
    STORED position has even row and column);  act;  mask_mode 2;  store at (oh*os + oo_h, ow*os + oo_w) of [N, Hy, Wy, Cout] with
    y_batch_stride between images.  mask and a same-geometry addend are read where y is written.

Operands come in two kinds.  EXACT: integers in [-4, 4] for x, w, add and add2, scale a signed power of two in {1, 2, 4}, shift an integer,
mask integers in [-2, 2] (real zeros and negatives), activation none or ReLU -- every product, partial sum and epilogue value is an integer
below 2^24, so the result is the same bits in every product mode (fp32 MFMA, three bf16 terms, two fp16 terms of power-of-two-scaled
operands, first bf16 term only), at any K, in any summation order: one dropped, doubled or misplaced product changes an element by at
least 1.  REAL: synth.normal operands, any scale, sigmoid allowed; compared at the bounds the suite already holds these kernels to.

A case carries its descriptor, which operands exist, and `runs`: configuration -> the name of the plan (plan_name) the launcher must
report there.  CONFIGS are product mode x conv.PRESPLIT x run-time options; everything is reached in-process.

Paths that only an environment variable read once at start-up can reach are NOT forced (UNREACHABLE); each of them launches a kernel
instance that another condition reaches too, so every instance the launchers can name for a non-listed launch is in REACHABLE."""
import collections
import zlib

import numpy as np

from retinanet_mi355x import synth

MASK_BITS = 4
GUARD = 64                                       # floats of NaN before and after every input, bytes of poison behind every output

# ---------------------------------------------------------------------------------------------- configurations
# name -> (product mode, conv.PRESPLIT, {option name: value}); options not named: SPLITK 0, MF16 1, MF16_MIN 1
CONFIGS = collections.OrderedDict([
    ("native", ("native", True, {})),
    ("split", ("split", True, {})),                       # weights pre-split once (w_format 1) where the packed row is >= 64 long
    ("split-ik", ("split", False, {})),                   # both operands split in the kernel (w_format 0)
    ("split-nomf", ("split", True, {"MF16": 0})),
    ("split-min3", ("split", True, {"MF16_MIN": 3})),
    ("split3", ("split3", True, {})),                     # fp16 twin (w_format 3)
    ("split3-nomf", ("split3", True, {"MF16": 0})),
    ("split3-min3", ("split3", True, {"MF16_MIN": 3})),
    ("native-sk", ("native", True, {"SPLITK": 1})),
    ("split3-sk", ("split3", True, {"SPLITK": 1})),
])
OPTION_DEFAULTS = {"SPLITK": 0, "MF16": 1, "MF16_MIN": 1}
SPLIT_MIN_K = 64                                 # rn_fp32_split_min_k() without RN_FP32_SPLIT_MIN_K (the host test asserts it)


def plan_name(p):
    """A plan (conv.igemm_plan's dict) as the string the case tables hold."""
    fam = ("tile", "split", "mf16", "splitk")[p["family"]]
    if p["family"] == 3:
        kind = "relu" if p["relu"] else "plain"
    else:
        kind = "raw" if p["raw"] else ("relu" if p["relu"] else ("general" if p["general"] else "dense"))
        assert not p["relu"] or p["general"]
    s = "%s %dx%d/%d %s" % (fam, p["rows"], p["cols"], p["waves"], kind)
    s += (" S%d" % p["split"] if p["split"] else "") + (" T%d" % p["terms"] if p["terms"] else "") + (" staged" if p["staged"] else "")
    if p["family"] == 3:
        s += " fin-general" if p["finish"] else " fin-dense"
    else:
        assert p["finish"] == -1 and p["slices"] == p["used"] == p["steps"] == 0
    return s + ("", " grouped", " list")[p["form"]]


def _profile(native, split, split_ik, split3, **more):
    out = {"native": native, "split": split, "split-ik": split_ik, "split3": split3}
    out.update({k.replace("_", "-"): v for k, v in more.items()})
    return out


def narrow(kind):
    """Cout <= 64, packed row >= 64: the 256 x 64 tile in each family."""
    return _profile("tile 256x64/4 " + kind, "split 256x64/4 %s S2 T3" % kind, "split 256x64/4 %s S1 T3" % kind, "split 256x64/4 %s S2 T2" % kind)


def wide_plain(kind):
    """128 x 128 where neither the 16x16x32 kernel nor SPLIT 3 applies (Cin % 16 != 0, div_shift != 0 or more than 24 taps)."""
    return _profile("tile 128x128/4 " + kind, "split 128x128/4 %s S2 T3" % kind, "split 128x128/4 %s S1 T3" % kind, "split 128x128/4 %s S2 T2" % kind)


def wide_once(kind):
    """128 x 128, Cin % 16 == 0, stride-1 addressing, <= 24 taps, but not the 16x16x32 kernel's (Cin % 32, Cout % 4, input ReLU)."""
    return dict(wide_plain(kind), split="split 128x128/4 %s S3 T3" % kind)


def wide_mf16(kind, long_k, batched=False):
    """What csrc/conv_igemm_mf16.hip takes: Cin % 32 == 0, Cout % 4 == 0, Cout > 64, <= 24 taps, div_shift 0, no input ReLU."""
    if not long_k:
        s3 = "mf16 128x128/4 %s T2" % kind
    elif batched:
        s3 = "mf16 128x128/4 %s T2 staged" % kind
    else:
        s3 = "mf16 256x128/8 %s T2 staged" % kind
    return dict(wide_once(kind), split="mf16 128x128/4 %s T3" % kind, **{"split-nomf": "split 128x128/4 %s S3 T3" % kind, "split3": s3,
                                                                        "split3-nomf": "split 128x128/4 %s S2 T2" % kind})


def short_k(tile_kind):
    """Packed row of 32 (K <= 32): no pre-split twin, below rn_fp32_split_min_k -- the fp32 MFMA tile in every mode."""
    return _profile(*["tile " + tile_kind] * 4)


UNREACHABLE = {
    "RN_SPLIT_A_ONCE=0": "SPLIT 2 on a 128 x 128 tile whose geometry qualifies for SPLIT 3 -- the same instances as wide_plain's split column",
    "RN_MF16_WV8_MIN=0 or > tiles": "the four-wave staged two-term tile for ONE weight tensor -- the same instances the batched GEMM reaches",
    "RN_MF16_STG_MIN_K": "moves the K = 256 border between the unstaged and the staged two-term forms; both sides are reached",
    "RN_FP32_SPLIT_MIN_K": "moves the K = 64 border between the fp32 MFMA tile and the split kernels for w_format 0; both sides are reached",
}


# ---------------------------------------------------------------------------------------------- cases
DESC_DEFAULTS = dict(act=0, add_mode=0, Ha=0, Wa=0, mask_mode=0, in_relu=0, os=1, oo_h=0, oo_w=0, add2_mode=0, Ha2=0, Wa2=0,
                     add2_batch_stride=0, w_batch_stride=0)


class Case:
    """d: the rn_conv_desc fields (geometry, strides, modes; mask_mode without RN_MASK_BITS).  scale / shift: per-channel factors exist.
    mask_bits: the mask is passed as sign bits.  sign: sign_out is asked for.  wbatch: per-image weights.  b16: w_format 2.  xgap:
    floats between images beyond the image (x_batch_stride).  conv: ("fprop" | "dgrad", k, stride, pad) when the case is an ordinary
    convolution torch can compute.  zero_taps: weight columns s >= this are zero (the stem's padded tap).  via: how the GPU test launches
    it -- "igemm" conv.conv_igemm, "desc" a hand-filled ConvDesc through ctypes, "fprop" / "dgrad" the allocating wrappers.
    sigmoid: the REAL form uses the sigmoid (the exact form none).  extra: config -> plan words beyond the name (grid, slices, ...)."""

    def __init__(self, name, d, runs, scale=False, shift=False, mask_bits=False, sign=False, wbatch=False, b16=False, xgap=0, conv=None,
                 zero_taps=None, via="igemm", sigmoid=False, extra=None):
        self.name, self.runs, self.scale, self.shift, self.mask_bits, self.sign = name, dict(runs), scale, shift, mask_bits, sign
        self.wbatch, self.b16, self.xgap, self.conv, self.zero_taps, self.via, self.sigmoid = wbatch, b16, xgap, conv, zero_taps, via, sigmoid
        self.extra = extra or {}
        d = dict(DESC_DEFAULTS, **d)
        d.setdefault("Hy", d["Ho"])
        d.setdefault("Wy", d["Wo"])
        d.setdefault("p_w", d["p"])
        d.setdefault("x_batch_stride", d["Hi"] * d["Wi"] * d["Cin"] + xgap)
        d.setdefault("y_batch_stride", d["Hy"] * d["Wy"] * d["Cout"])
        if d["add_mode"] == 1:
            d.setdefault("add_batch_stride", d["y_batch_stride"])
        elif d["add_mode"] == 2:
            d.setdefault("add_batch_stride", d["Ha"] * d["Wa"] * d["Cout"])
        else:
            d.setdefault("add_batch_stride", 0)
        if d["add2_mode"]:
            d["add2_batch_stride"] = d["Ha2"] * d["Wa2"] * d["Cout"]
        self.kpad = (d["kh"] * d["kw"] * d["Cin"] + 31) // 32 * 32
        if wbatch:
            d["w_batch_stride"] = d["Cout"] * self.kpad
        self.d = d
        assert xgap == 0 or via == "desc"
        assert not sign or via == "desc" or (d["os"] == 1 and d["y_batch_stride"] == d["Ho"] * d["Wo"] * d["Cout"])

    @property
    def K(self):
        return self.d["kh"] * self.d["kw"] * self.d["Cin"]

    @property
    def M(self):
        return self.d["N"] * self.d["Ho"] * self.d["Wo"]


def fwd(N, H, W, cin, cout, k, stride=1, pad=None, kw=None, **over):
    """Descriptor of a forward convolution (conv._fprop's geometry); kw > k: padded tap columns."""
    pad = k // 2 if pad is None else pad
    d = dict(N=N, Hi=H, Wi=W, Cin=cin, Ho=(H + 2 * pad - k) // stride + 1, Wo=(W + 2 * pad - k) // stride + 1, Cout=cout, kh=k,
             kw=kw or k, a=stride, b=1, p=-pad, div_shift=0)
    d.update(over)
    return d


def bwd(N, Ho, Wo, cout, Hi, Wi, cin, k, stride, pad, **over):
    """Descriptor of the generic data gradient (conv._dgrad's geometry): dy [N, Ho, Wo, cout] -> dx [N, Hi, Wi, cin]."""
    d = dict(N=N, Hi=Ho, Wi=Wo, Cin=cout, Ho=Hi, Wo=Wi, Cout=cin, kh=k, kw=k, a=1, b=-1, p=pad, div_shift=stride.bit_length() - 1)
    d.update(over)
    return d


def _cases():
    C = []
    add = C.append
    F, D = "fprop", "dgrad"
    # ---- every instance of the plain launch, by tile: narrow dense / general, wide dense / general / raw, input ReLU
    add(Case("narrow-dense-3x3", fwd(2, 9, 7, 16, 64, 3, act=1), narrow("dense"), scale=True, shift=True, conv=(F, 3, 1, 1), sigmoid=True))
    add(Case("narrow-general-head-slice", fwd(2, 9, 7, 16, 36, 3, y_batch_stride=9 * 7 * 36 + 180), narrow("general"), shift=True,
             sigmoid=True))                                                        # a head writing its slice of [B, A, n]
    add(Case("wide-dense-cout65", fwd(2, 9, 8, 16, 65, 3, act=1), wide_once("dense"), scale=True, shift=True, conv=(F, 3, 1, 1)))      # last column tile 1 wide, scalar epilogue
    add(Case("wide-general-cout132-add2up", fwd(2, 9, 7, 48, 132, 3, add_mode=2, Ha=5, Wa=4), wide_once("general"), shift=True,
             conv=(F, 3, 1, 1)))                                                   # last column tile 4 wide; FPN add on odd sizes
    add(Case("wide-raw-gemm", fwd(1, 1, 300, 80, 132, 1), dict(wide_once("raw"), split3="split 128x128/4 dense S2 T2")))      # split3: y_amax is asked for, so not raw
    add(Case("wide-raw-gemm-desc", fwd(1, 1, 300, 80, 132, 1), wide_once("raw"), via="desc"))
    add(Case("wide-raw-gemm-cin72-desc", fwd(1, 1, 300, 72, 132, 1), wide_plain("raw"), via="desc"))            # Cin % 16 != 0: no SPLIT 3
    add(Case("wide-raw-gemm-affine", fwd(1, 1, 300, 80, 132, 1), wide_once("dense"), scale=True))     # a scale alone leaves the raw instance
    add(Case("relu-on-load", fwd(2, 9, 7, 48, 40, 3, in_relu=1, act=1), wide_once("relu"), shift=True))                 # Cout <= 64 is NOT narrow with in_relu
    add(Case("relu-on-load-7x7", fwd(1, 11, 9, 8, 72, 7, in_relu=1), wide_plain("relu"), conv=None))
    add(Case("wide-plain-7x7-pad3", fwd(1, 11, 9, 8, 68, 7, act=1), wide_plain("dense"), scale=True, conv=(F, 7, 1, 3)))
    add(Case("wide-plain-cin20-general", fwd(2, 6, 5, 20, 117, 3, y_batch_stride=6 * 5 * 117 + 39), wide_plain("general"), shift=True))   # 9 * 13 = 117
    # ---- the 16x16x32 kernels: three terms / two terms unstaged (K < 256) / staged eight waves / staged four waves (batched)
    add(Case("mf16-dense-k128", fwd(3, 7, 7, 128, 132, 1, act=1), wide_mf16("dense", False), scale=True, shift=True, conv=(F, 1, 1, 0)))
    add(Case("mf16-general-k288-add2up", fwd(2, 9, 7, 32, 132, 3, add_mode=2, Ha=5, Wa=4), wide_mf16("general", True), shift=True,
             conv=(F, 3, 1, 1), sigmoid=True))
    add(Case("mf16-raw-k64", fwd(1, 1, 300, 64, 128, 1), dict(wide_mf16("raw", False), split3="mf16 128x128/4 dense T2",
                                                             **{"split3-nomf": "split 128x128/4 dense S2 T2"})))       # split3: y_amax is asked for, so not raw
    add(Case("mf16-raw-k256", fwd(1, 1, 300, 256, 128, 1), wide_mf16("raw", True), via="desc"))          # no y_amax: raw in split3 too
    add(Case("mf16-dense-k256-min-tiles", fwd(1, 16, 16, 256, 72, 1), dict(wide_mf16("dense", True), **{
        "split-min3": "split 128x128/4 dense S3 T3", "split3-min3": "split 128x128/4 dense S2 T2"}), scale=True))     # 2 tiles < RN_OPT_MF16_MIN 3
    add(Case("mf16-dense-k256-three-tiles", fwd(1, 16, 17, 256, 72, 1), dict(wide_mf16("dense", True), **{
        "split-min3": "mf16 128x128/4 dense T3", "split3-min3": "mf16 256x128/8 dense T2 staged"}), scale=True))       # 3 tiles of 128 rows (2 of 256)
    # batched GEMMs (per-image weights that differ; Ho*Wo a multiple of 256): raw and with an epilogue
    add(Case("batched-raw-k64", fwd(3, 1, 256, 64, 132, 1), wide_mf16("raw", False, True), wbatch=True))
    add(Case("batched-raw-k256", fwd(3, 1, 256, 256, 72, 1), wide_mf16("raw", True, True), wbatch=True))
    add(Case("batched-dense-k256", fwd(2, 2, 256, 256, 72, 1, act=1), wide_mf16("dense", True, True), wbatch=True, shift=True))
    add(Case("batched-general-k256", fwd(2, 1, 256, 256, 72, 1, y_batch_stride=256 * 72 + 64), wide_mf16("general", True, True), wbatch=True))
    add(Case("batched-narrow", fwd(3, 1, 256, 32, 24, 1), dict(short_k("256x64/4 dense")), wbatch=True, scale=True))
    add(Case("batched-narrow-k96", fwd(3, 1, 256, 96, 24, 1), narrow("dense"), wbatch=True, scale=True))
    # ---- short reductions: the Kpad zero columns, the fp32 MFMA tile in every mode
    add(Case("k-below-32-narrow", fwd(2, 5, 6, 4, 8, 1), short_k("256x64/4 dense"), scale=True, conv=(F, 1, 1, 0)))       # K = 4, Kpad 32
    add(Case("k-below-32-wide", fwd(2, 5, 6, 12, 65, 1, act=1), short_k("128x128/4 dense"), shift=True, conv=(F, 1, 1, 0)))  # K = 12
    add(Case("k36-kpad64", fwd(2, 5, 6, 4, 8, 3), dict(narrow("dense"), **{"split-ik": "tile 256x64/4 dense"}), conv=(F, 3, 1, 1)))   # twin made (Kpad 64), K = 36 < 64 without it
    # ---- the stem: Cin 4, 7 x 7 stride 2 pad 3 packed with kw 8 (the eighth tap column is padding), and its bf16-product form
    add(Case("stem-cin4-kw8", fwd(2, 13, 11, 4, 64, 7, 2, 3, kw=8, act=1), narrow("dense"), scale=True, shift=True, zero_taps=7,
             conv=(F, 7, 2, 3)))
    add(Case("stem-cin4-kw8-full-taps", fwd(2, 13, 11, 4, 64, 7, 2, 3, kw=8), narrow("dense")))      # nonzero weights in column 7: its x must be read like any tap's
    add(Case("stem-b16-dense", fwd(2, 13, 11, 4, 64, 7, 2, 3, kw=8, act=1), {c: "split 256x64/4 dense S2 T1" for c in ("native", "split", "split3")},
             scale=True, shift=True, zero_taps=7, b16=True, sign=True, conv=(F, 7, 2, 3)))
    add(Case("stem-b16-general", fwd(2, 13, 11, 4, 64, 7, 2, 3, kw=8, y_batch_stride=7 * 6 * 64 + 128), {c: "split 256x64/4 general S2 T1" for c in ("native", "split3")},
             shift=True, zero_taps=7, b16=True))
    # ---- geometry: 1 x 1 stride 2, H = 1, W = 1, unequal (p_rows, p_cols)
    add(Case("1x1-stride2-narrow", fwd(2, 9, 7, 64, 32, 1, 2, 0), narrow("dense"), shift=True, conv=(F, 1, 2, 0)))
    add(Case("1x1-stride2-mf16", fwd(2, 9, 7, 64, 128, 1, 2, 0), wide_mf16("dense", False), shift=True, conv=(F, 1, 2, 0)))
    add(Case("h1-narrow", fwd(3, 1, 37, 16, 24, 3), narrow("dense"), conv=(F, 3, 1, 1)))
    add(Case("w1-wide", fwd(3, 37, 1, 16, 68, 3), wide_once("dense"), conv=(F, 3, 1, 1), shift=True))
    add(Case("w1-mf16", fwd(3, 37, 1, 32, 68, 3), wide_mf16("dense", True), conv=(F, 3, 1, 1), scale=True))
    add(Case("p-rows-ne-cols-narrow", dict(fwd(2, 8, 9, 16, 24, 3), p=0, p_w=-2, Ho=7, Wo=10), narrow("dense")))
    add(Case("p-rows-ne-cols-wide", dict(fwd(2, 8, 9, 16, 68, 3), p=-2, p_w=1, Ho=9, Wo=6), wide_once("dense"), shift=True))
    add(Case("p-rows-ne-cols-mf16", dict(fwd(2, 8, 9, 32, 68, 3), p=-2, p_w=1, Ho=9, Wo=6), wide_mf16("dense", True), scale=True))
    # ---- epilogue operands: masks before / after as floats and as sign bits, sign_out, addend strides
    add(Case("mask-before-float-narrow", fwd(2, 9, 7, 16, 64, 3, add_mode=1, mask_mode=1, act=1), narrow("dense"), scale=True))
    add(Case("mask-before-bits-wide", fwd(2, 9, 7, 16, 96, 3, add_mode=1, mask_mode=1), wide_once("dense"), mask_bits=True, shift=True))
    add(Case("mask-before-bits-mf16", fwd(2, 9, 7, 32, 96, 3, add_mode=1, mask_mode=1), wide_mf16("dense", True), mask_bits=True))
    add(Case("mask-after-bits-narrow-sign", fwd(2, 9, 7, 16, 64, 3, add_mode=1, mask_mode=2), narrow("dense"), mask_bits=True, sign=True))
    add(Case("mask-after-float-wide-cout119", fwd(2, 9, 7, 16, 119, 3, add_mode=1, mask_mode=2), wide_once("dense"), shift=True))
    add(Case("mask-after-float-mf16-sign", fwd(2, 9, 7, 32, 96, 3, add_mode=1, mask_mode=2, act=1), wide_mf16("dense", True), sign=True, scale=True))
    add(Case("mask-before-float-mf16-k64", fwd(2, 9, 7, 64, 96, 1, add_mode=1, mask_mode=1), wide_mf16("dense", False)))
    add(Case("cout39-narrow-scalar-epilogue", fwd(2, 9, 7, 16, 39, 3, add_mode=1, mask_mode=2, act=1), narrow("dense"), scale=True, shift=True))
    add(Case("add-stride-ne-y-stride-narrow", fwd(2, 5, 6, 16, 24, 3, add_mode=1, add_batch_stride=5 * 6 * 24 + 48), narrow("general")))
    add(Case("add-stride-ne-y-stride-wide", fwd(2, 5, 6, 16, 68, 3, add_mode=1, add_batch_stride=5 * 6 * 68 + 136, mask_mode=2), wide_once("general")))
    add(Case("add-stride-ne-y-stride-mf16", fwd(2, 5, 6, 32, 68, 3, add_mode=1, add_batch_stride=5 * 6 * 68 + 136, mask_mode=1), wide_mf16("general", True)))
    add(Case("add2up-odd-narrow", fwd(2, 9, 7, 16, 24, 3, add_mode=2, Ha=5, Wa=4, add_batch_stride=5 * 4 * 24 + 24), narrow("general"), shift=True))
    # ---- x_batch_stride larger than an image (NaN between the images), with sign bits through an output map: hand-filled descriptors
    add(Case("x-gap-narrow", fwd(3, 5, 6, 16, 32, 3, act=1), narrow("dense"), xgap=160, via="desc", sign=True, scale=True))
    add(Case("x-gap-wide", fwd(3, 5, 6, 16, 96, 3), wide_once("dense"), xgap=160, via="desc", shift=True))
    add(Case("x-gap-mf16", fwd(3, 5, 6, 32, 96, 3), wide_mf16("dense", True), xgap=96, via="desc", shift=True))
    add(Case("x-gap-mf16-k64", fwd(3, 5, 6, 64, 96, 1, 1, 0), wide_mf16("dense", False), xgap=64, via="desc", scale=True))
    # ---- a 256-row tile across dozens of tiny images (n_first, the per-tile buffer range, the amax note's span)
    add(Case("tiny-1x1-images-narrow", fwd(300, 1, 1, 16, 24, 3, act=1), narrow("dense"), shift=True, conv=(F, 3, 1, 1)))
    add(Case("tiny-2x2-images-narrow", fwd(70, 2, 2, 16, 24, 3), narrow("dense"), conv=(F, 3, 1, 1)))
    add(Case("tiny-3x3-images-narrow-general", fwd(40, 3, 3, 16, 24, 3, y_batch_stride=9 * 24 + 8), narrow("general")))
    add(Case("tiny-1x1-images-mf16", fwd(300, 1, 1, 32, 68, 3), wide_mf16("dense", True), conv=(F, 3, 1, 1), shift=True))
    add(Case("tiny-2x2-images-mf16", fwd(70, 2, 2, 32, 68, 3, add_mode=1, act=1), wide_mf16("dense", True)))
    add(Case("tiny-3x3-images-mf16-general", fwd(40, 3, 3, 32, 68, 3, y_batch_stride=9 * 68 + 4), wide_mf16("general", True)))
    add(Case("tiny-2x2-images-wide", fwd(70, 2, 2, 16, 68, 3), wide_once("dense"), scale=True))
    add(Case("tiny-2x2-images-x-gap-mf16", fwd(70, 2, 2, 32, 68, 3), wide_mf16("dense", True), xgap=32, via="desc", shift=True))
    # ---- the generic stride-2 data gradient (div_shift 1), slow path (Cin % 16 != 0) and fast, with an addend and a mask
    add(Case("dgrad-s2-slow-narrow", bwd(2, 5, 4, 20, 9, 7, 16, 3, 2, 1, add_mode=1, mask_mode=2), narrow("dense"), conv=(D, 3, 2, 1)))
    add(Case("dgrad-s2-slow-wide", bwd(2, 5, 4, 20, 9, 7, 68, 3, 2, 1, add_mode=1, mask_mode=2), wide_plain("dense"), conv=(D, 3, 2, 1)))
    add(Case("dgrad-s2-fast-wide", bwd(2, 5, 4, 32, 10, 8, 68, 3, 2, 1, add_mode=1, mask_mode=1), wide_plain("dense"), conv=(D, 3, 2, 1)))      # div_shift keeps it off the mf16 / SPLIT 3 kernels
    add(Case("dgrad-s2-1x1-even", bwd(2, 5, 4, 64, 10, 8, 32, 1, 2, 0), narrow("dense"), conv=(D, 1, 2, 0)))
    add(Case("dgrad-s2-7x7-odd", bwd(1, 5, 4, 8, 9, 7, 12, 7, 2, 3, add_mode=1), narrow("dense"), conv=(D, 7, 2, 3)))
    add(Case("dgrad-s1-mf16", bwd(2, 9, 7, 32, 9, 7, 68, 3, 1, 1, add_mode=1, mask_mode=2), wide_mf16("dense", True), conv=(D, 3, 1, 1)))
    # ---- output maps with os = 2 at the four offsets, with add2 (the shortcut's gradient at even stored positions) and a mask
    for oh, ow in ((0, 0), (0, 1), (1, 0), (1, 1)):
        gh, gw = (9 - oh + 1) // 2, (7 - ow + 1) // 2
        m = dict(os=2, oo_h=oh, oo_w=ow, Hy=9, Wy=7, add2_mode=3, Ha2=5, Wa2=4, add_mode=1, mask_mode=2)
        add(Case("outmap-%d%d-narrow" % (oh, ow), dict(fwd(2, gh, gw, 16, 24, 3), **m), narrow("general"), shift=True))
        add(Case("outmap-%d%d-wide" % (oh, ow), dict(fwd(2, gh, gw, 16, 68, 3), **m), wide_once("general")))
        add(Case("outmap-%d%d-mf16" % (oh, ow), dict(fwd(2, gh, gw, 32, 96, 3), **m), wide_mf16("general", True), mask_bits=True))
    add(Case("outmap-11-mf16-sign", dict(fwd(2, 4, 3, 32, 96, 3), os=2, oo_h=1, oo_w=1, Hy=9, Wy=7), wide_mf16("general", True), sign=True, via="desc"))
    # ---- the allocating wrappers
    add(Case("fprop-wrapper", fwd(2, 9, 7, 32, 72, 3, 2, 1, act=1), wide_mf16("dense", True), scale=True, shift=True, conv=(F, 3, 2, 1), via="fprop"))
    add(Case("dgrad-wrapper", bwd(2, 5, 4, 24, 9, 7, 16, 3, 2, 1, add_mode=1, mask_mode=2), narrow("dense"), conv=(D, 3, 2, 1), via="dgrad"))
    # ---- split-K (RN_OPT_SPLITK 1; fp32 MFMA in every mode): the three partial kernels x the two finish kernels
    sk = lambda part, fin: {"native-sk": "splitk %s %s fin-%s" % (part, "relu" if "relu" in fin else "plain", fin.replace("relu-", "")),
                            "split3-sk": "splitk %s %s fin-%s" % (part, "relu" if "relu" in fin else "plain", fin.replace("relu-", ""))}
    # 3 x 3 x 64: 36 K-steps in 2 slices of 18 -- slice 1 starts in the middle of tap 4 (18 = 4 taps x 4 steps + 2)
    add(Case("splitk-mid-tap-narrow-dense", fwd(2, 9, 7, 64, 24, 3, act=1, add_mode=1, mask_mode=2), sk("256x64/4", "dense"), scale=True, shift=True,
             conv=(F, 3, 1, 1), extra={"native-sk": dict(grid=1, slices=2, used=2, steps=18)}))
    add(Case("splitk-mid-tap-narrow-general", fwd(2, 9, 7, 64, 39, 3, add_mode=2, Ha=5, Wa=4), sk("256x64/4", "general"), shift=True,
             extra={"native-sk": dict(grid=1, slices=2, used=2, steps=18)}))
    add(Case("splitk-wide-dense-cout67", fwd(2, 9, 7, 64, 67, 3), sk("128x128/4", "dense"), scale=True, extra={"native-sk": dict(grid=1, slices=2, used=2, steps=18)}))
    add(Case("splitk-wide-general-cout132", fwd(2, 9, 8, 48, 132, 5, y_batch_stride=9 * 8 * 132 + 132, act=1), sk("128x128/4", "general"), shift=True,
             extra={"native-sk": dict(grid=4, slices=4, used=4, steps=19)}))       # 5 x 5 x 48: 76 steps, 3 per tap, 19 per slice
    add(Case("splitk-relu-dense", fwd(2, 9, 7, 64, 40, 3, in_relu=1), sk("128x128/4", "relu-dense"), shift=True))
    add(Case("splitk-relu-general", fwd(2, 9, 7, 64, 40, 3, in_relu=1, add_mode=2, Ha=5, Wa=4), sk("128x128/4", "relu-general")))
    # 7 x 1 x 736: K = 5152, 322 K-steps, 20 slices asked, 17 steps each -> only 19 get work (used < slices)
    add(Case("splitk-used-below-slices", dict(fwd(1, 9, 3, 736, 8, 7), kw=1, p_w=0), sk("256x64/4", "dense"), shift=True,
             extra={"native-sk": dict(grid=1, slices=20, used=19, steps=17)}))
    add(Case("splitk-stride2-dgrad", bwd(1, 5, 4, 64, 9, 7, 16, 3, 2, 1, add_mode=1), sk("256x64/4", "dense"), conv=(D, 3, 2, 1)))
    # the tile-count border: 159 tiles split, 160 do not
    add(Case("splitk-159-tiles", fwd(1, 201, 202, 64, 8, 3), dict(sk("256x64/4", "dense"), native="tile 256x64/4 dense"),
             extra={"native-sk": dict(grid=159, slices=2, used=2, steps=18)}))
    add(Case("splitk-160-tiles-no-split", fwd(1, 202, 202, 64, 8, 3), {"native-sk": "tile 256x64/4 dense", "split3-sk": "split 256x64/4 dense S2 T2"}))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- grouped launches (conv.conv_igemm_grouped: shared weights, add_mode 1 and mask per member, optional y_batch_stride)
class Group:
    """members: [(N, H, W, features)] forward 3 x 3 / 1 x 1 problems sharing cin, cout, k; features: add, mask (mask_mode), ybs_extra."""

    def __init__(self, name, cin, cout, k, members, runs, act=0, scale=False, shift=False, sigmoid=False):
        self.name, self.runs, self.act, self.scale, self.shift, self.sigmoid = name, dict(runs), act, scale, shift, sigmoid
        self.cases = []
        for i, (N, H, W, f) in enumerate(members):
            over = dict(act=act, add_mode=1 if f.get("add") else 0, mask_mode=f.get("mask", 0))
            if f.get("ybs_extra"):
                over["y_batch_stride"] = H * W * cout + f["ybs_extra"]
            self.cases.append(Case("%s/%d" % (name, i), fwd(N, H, W, cin, cout, k, **over), {}, scale=scale, shift=shift, sigmoid=sigmoid))
        self.kpad = self.cases[0].kpad


def grouped(p):
    return {k: v + " grouped" for k, v in p.items()}


def _groups():
    G = []
    five = [(2, 9, 7, {}), (1, 16, 17, {"add": 1}), (1, 5, 5, {"mask": 2}), (2, 12, 11, {"add": 1, "mask": 1}), (1, 3, 3, {"ybs_extra": 72})]
    # 128-row tiles: 126 / 272 / 25 / 264 / 9 rows -> 1, 3, 1, 3, 1 tiles: one-tile problems at both ends and in the middle
    G.append(Group("g5-narrow", 16, 24, 3, five, grouped(narrow("general")), act=1, scale=True, shift=True))
    G.append(Group("g5-wide-cout65", 16, 65, 3, five[:4], grouped(wide_once("general")), shift=True))
    mf = wide_mf16("general", True)
    mf["split3"] = "mf16 128x128/4 general T2 staged"              # the grouped two-term form: four waves, staged
    G.append(Group("g5-mf16", 32, 72, 3, five, grouped(mf), act=1, scale=True, sigmoid=True))
    G.append(Group("g2-mf16-cout132", 32, 132, 3, [(2, 9, 7, {"add": 1}), (1, 16, 17, {"mask": 2})], grouped(mf), shift=True))
    G.append(Group("g1-narrow", 16, 24, 3, [(2, 9, 7, {"add": 1, "mask": 2})], grouped(narrow("general"))))
    G.append(Group("g1-mf16", 64, 68, 1, [(3, 9, 7, {})], grouped(dict(mf, split3="mf16 128x128/4 general T2 staged")), shift=True))
    G.append(Group("g2-wide-7x7", 8, 68, 7, [(1, 9, 7, {}), (1, 5, 6, {"add": 1})], grouped(wide_plain("general"))))
    G.append(Group("g2-short-k", 4, 8, 1, [(2, 9, 7, {}), (1, 5, 6, {"mask": 2})], grouped(short_k("256x64/4 general")), scale=True))
    G.append(Group("g2-short-k-wide", 8, 68, 1, [(2, 9, 7, {}), (1, 5, 6, {"add": 1})], grouped(short_k("128x128/4 general"))))
    return G


GROUPS = _groups()

# ---- stride-2 data gradients by output-parity class (conv.dgrad_s2_classes): (name, N, Ho, Wo, cout, Hi, Wi, cin, k, pad, add, mask, add2)
S2Case = collections.namedtuple("S2Case", "name N Ho Wo cout Hi Wi cin k pad add mask add2 runs")



def _per_class(*profiles):
    """config -> [plan of class 0, 1, ...] from one profile per class."""
    return {cfg: [p[cfg] for p in profiles] for cfg in profiles[0] if all(cfg in p for p in profiles)}


_NG, _SG = narrow("general"), short_k("256x64/4 general")
_MU, _ML = wide_mf16("general", False), wide_mf16("general", True)
S2 = [
    S2Case("s2-k1-even", 2, 5, 4, 64, 10, 8, 32, 1, 0, False, 0, False, _per_class(_NG)),     # one class: the other three stay zero
    # 3 x 3, pad 1: classes of 1 x 1, 1 x 2, 2 x 1 and 2 x 2 taps -- K = 16, 32, 32 (packed rows of 32) and 64
    S2Case("s2-k3-odd", 2, 5, 4, 16, 9, 7, 24, 3, 1, True, 2, True, _per_class(_SG, _SG, _SG, _NG)),
    S2Case("s2-k3-even-mf16", 2, 5, 4, 64, 10, 8, 68, 3, 1, True, 1, False, _per_class(_MU, _MU, _MU, _ML)),      # K = 64, 128, 128, 256
    S2Case("s2-k7-odd", 1, 5, 4, 8, 9, 7, 12, 7, 3, True, 2, False, _per_class(_NG, _NG, _NG, _NG)),
    S2Case("s2-k7-even", 1, 5, 4, 8, 10, 8, 12, 7, 3, True, 0, False, _per_class(_NG, _NG, _NG, _NG)),
]


# ---------------------------------------------------------------------------------------------- operands
def _seed(name, i):
    return (zlib.crc32(name.encode()) + 7919 * i) % (1 << 30)


def _ints(shape, seed, lo, hi):
    return (synth.randint(shape, seed, hi - lo + 1) + lo).astype(np.float32)


def _bf16_round(a):
    """Round to the nearest bf16 value (ties to even), as fp32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


class Operands:
    """Flat fp32 buffers of one case in the C ABI's layouts.  x: N images at x_batch_stride, NaN between them.  w: [Nb][Cout][Kpad], zero
    padded.  mask / add / add2 as the descriptor addresses them; ysize: floats the launch may address (last image's extent)."""


def operands(c, exact, name=None, w_from=None):
    d, o = c.d, Operands()
    name = name or c.name
    ex = "x" if exact else "r"
    draw = (lambda shape, i, std=1.0: _ints(shape, _seed(name + ex, i), -4, 4)) if exact else \
        (lambda shape, i, std=1.0: synth.normal(shape, _seed(name + ex, i), std))
    N, Cin, Cout = d["N"], d["Cin"], d["Cout"]
    img = d["Hi"] * d["Wi"] * Cin
    o.x4 = draw((N, d["Hi"], d["Wi"], Cin), 1)
    nb = N if c.wbatch else 1
    if w_from is not None:
        o.w5 = w_from.w5
    else:
        o.w5 = draw((nb, Cout, d["kh"], d["kw"], Cin), 2, (2.0 / max(c.K, 1)) ** 0.5)
        if c.zero_taps is not None:
            o.w5[:, :, :, c.zero_taps:, :] = 0.0
    if c.b16 and not exact:                      # products from the first bf16 terms: the fp32 convolution of bf16-rounded operands
        o.x4, o.w5 = _bf16_round(o.x4), _bf16_round(o.w5)
    o.x = np.full((N - 1) * d["x_batch_stride"] + img, np.nan, dtype=np.float32)
    for n in range(N):
        o.x[n * d["x_batch_stride"]:n * d["x_batch_stride"] + img] = o.x4[n].reshape(-1)
    o.w = np.zeros((nb, Cout, c.kpad), dtype=np.float32)
    o.w[:, :, :c.K] = o.w5.reshape(nb, Cout, c.K)
    if exact:
        o.scale = (np.float32(2.0) ** synth.randint((Cout,), _seed(name, 3), 3).astype(np.float32)) * \
            np.where(synth.randint((Cout,), _seed(name, 4), 3) == 0, np.float32(-1), np.float32(1)) if c.scale else None
        o.shift = _ints((Cout,), _seed(name, 5), -3, 3) if c.shift else None
    else:
        o.scale = synth.normal((Cout,), _seed(name, 3), 0.3, 1.0) if c.scale else None
        o.shift = synth.normal((Cout,), _seed(name, 5), 0.2) if c.shift else None
    if w_from is not None:                       # a member of a group: the group's weights and factors
        o.scale, o.shift = w_from.scale, w_from.shift
    o.ysize = (N - 1) * d["y_batch_stride"] + d["Hy"] * d["Wy"] * Cout
    o.mask = _ints((o.ysize,), _seed(name, 6), -2, 2) if d["mask_mode"] else None
    if d["add_mode"] == 1:
        o.add = draw(((N - 1) * d["add_batch_stride"] + d["Hy"] * d["Wy"] * Cout,), 7)
    elif d["add_mode"] == 2:
        o.add = draw(((N - 1) * d["add_batch_stride"] + d["Ha"] * d["Wa"] * Cout,), 7)
    else:
        o.add = None
    o.add2 = draw((N * d["Ha2"] * d["Wa2"] * Cout,), 8) if d["add2_mode"] else None
    o.act = d["act"] if (exact or not c.sigmoid) else 2
    return o


def sign_words(values):
    """RN_MASK_BITS layout of a flat fp32 buffer whose length is a multiple of 32: bit (e & 31) of word (e >> 5) = values[e] > 0."""
    b = (np.asarray(values).reshape(-1, 32) > 0).astype(np.uint32)
    return (b << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- the reference
def owned_offsets(d):
    """Float offset of channel 0 of every output pixel in the y buffer: [N, Ho, Wo] int64."""
    n = np.arange(d["N"], dtype=np.int64)[:, None, None]
    ph = (np.arange(d["Ho"], dtype=np.int64) * d["os"] + d["oo_h"])[None, :, None]
    pw = (np.arange(d["Wo"], dtype=np.int64) * d["os"] + d["oo_w"])[None, None, :]
    return n * d["y_batch_stride"] + (ph * d["Wy"] + pw) * d["Cout"], ph + 0 * pw + 0 * n, pw + 0 * ph + 0 * n


def reference(c, o):
    """-> (values [N, Ho, Wo, Cout] float64, offsets [N, Ho, Wo] of their channel 0 in the y buffer)."""
    d = c.d
    N, Hi, Wi, Cin, Ho, Wo, Cout = (d[k] for k in ("N", "Hi", "Wi", "Cin", "Ho", "Wo", "Cout"))
    x = o.x4.astype(np.float64)
    if d["in_relu"]:
        x = np.maximum(x, 0.0)
    w = o.w5.astype(np.float64)
    dm = (1 << d["div_shift"]) - 1
    acc = np.zeros((N, Ho, Wo, Cout))
    for r in range(d["kh"]):
        nh = np.arange(Ho) * d["a"] + d["p"] + r * d["b"]
        okh = (nh >= 0) & ((nh & dm) == 0) & ((nh >> d["div_shift"]) < Hi)
        ih = np.where(okh, nh >> d["div_shift"], 0)
        for s in range(d["kw"]):
            nw = np.arange(Wo) * d["a"] + d["p_w"] + s * d["b"]
            okw = (nw >= 0) & ((nw & dm) == 0) & ((nw >> d["div_shift"]) < Wi)
            iw = np.where(okw, nw >> d["div_shift"], 0)
            if not okh.any() or not okw.any():
                continue
            g = x[:, ih][:, :, iw] * (okh[:, None] & okw[None, :])[None, :, :, None]
            acc += np.einsum("nhwc,noc->nhwo", g, w[:, :, r, s, :] if c.wbatch else np.broadcast_to(w[0, :, r, s, :], (N, Cout, Cin)))
    off, ph, pw = owned_offsets(d)
    ch = np.arange(Cout)
    v = acc
    if o.scale is not None:
        v = v * o.scale.astype(np.float64)
    if o.shift is not None:
        v = v + o.shift.astype(np.float64)
    keep = None if o.mask is None else o.mask[off[..., None] + ch] > 0
    if d["mask_mode"] == 1:
        v = np.where(keep, v, 0.0)
    if d["add_mode"] == 1:
        aoff = np.arange(N)[:, None, None] * d["add_batch_stride"] + (ph * d["Wy"] + pw) * Cout
        v = v + o.add[aoff[..., None] + ch].astype(np.float64)
    elif d["add_mode"] == 2:
        aoff = np.arange(N)[:, None, None] * d["add_batch_stride"] + \
            ((np.arange(Ho)[None, :, None] >> 1) * d["Wa"] + (np.arange(Wo)[None, None, :] >> 1)) * Cout
        v = v + o.add[aoff[..., None] + ch].astype(np.float64)
    if d["add2_mode"] == 3:
        even = ((ph | pw) & 1) == 0
        a2 = np.arange(N)[:, None, None] * d["add2_batch_stride"] + ((ph >> 1) * d["Wa2"] + (pw >> 1)) * Cout
        a2 = np.where(even, a2, 0)
        v = v + np.where(even[..., None], o.add2[a2[..., None] + ch].astype(np.float64), 0.0)
    if o.act == 1:
        v = np.maximum(v, 0.0)
    elif o.act == 2:
        v = 1.0 / (1.0 + np.exp(-v))
    if d["mask_mode"] == 2:
        v = np.where(keep, v, 0.0)
    return v, off


def expected_buffer(c, o, values, off):
    """The whole y buffer after the launch as float64: the reference where the launch owns an element, NaN (the poison) elsewhere."""
    buf = np.full(o.ysize, np.nan)
    buf[(off[..., None] + np.arange(c.d["Cout"])).reshape(-1)] = values.reshape(-1)
    return buf


# ---------------------------------------------------------------------------------------------- what a launch of the wrappers looks like
def w_format(c, config):
    """rn_conv_desc.w_format conv.conv_igemm passes for this case under this configuration (conv._w_operand / _maybe_split): the twin exists
    for packed rows of at least rn_fp32_split_min_k floats when conv.PRESPLIT is on."""
    mode, presplit, opts = CONFIGS[config]
    if c.b16:
        return 2
    if mode == "native" or not presplit or c.kpad < SPLIT_MIN_K:
        return 0
    return 3 if mode == "split3" else 1


def wants_y_amax(c, config):
    """conv.conv_igemm leaves amax words for a dense single-weight result in split3 mode (which rules out the raw instance)."""
    d = c.d
    return c.via != "desc" and CONFIGS[config][0] == "split3" and not c.wbatch and d["os"] == 1 and d["y_batch_stride"] == d["Ho"] * d["Wo"] * d["Cout"] and \
        d["Hy"] == d["Ho"] and d["Wy"] == d["Wo"]


def desc_of(c, conv, fmt=0, sign_out=None, x_amax=None, y_amax=None, w_unscale=None):
    """The ConvDesc of case c with the weight form and the pointer fields given (addresses; only NULL or not matters to the plan query)."""
    d = conv.ConvDesc()
    for k, v in c.d.items():
        setattr(d, k, v)
    if c.mask_bits and c.d["mask_mode"]:
        d.mask_mode = c.d["mask_mode"] | MASK_BITS
    d.w_format, d.sign_out, d.x_amax, d.y_amax, d.w_unscale = fmt, sign_out, x_amax, y_amax, w_unscale
    d.x_amax_img_stride, d.x_amax_row_stride = (1, 0) if fmt == 3 else (0, 0)
    return d


def takes_splitk(config):
    return CONFIGS[config][2].get("SPLITK", 0) == 1


def plan_keys():
    """Every plan name the tables expect."""
    return {p for c in CASES for p in c.runs.values()} | {p for g in GROUPS for p in g.runs.values()} | \
        {p for s in S2 for ps in s.runs.values() for p in ps}


def _reachable():
    """Every plan the launchers can report for a non-listed launch, from the instances their source files name."""
    R = set()
    for tile in ("256x64/4", "128x128/4"):
        kinds = ("dense", "general") if tile[0] == "2" else ("dense", "general", "raw", "relu")
        for k in kinds:
            R.add("tile %s %s" % (tile, k))
            for st in ("S1 T3", "S2 T3", "S2 T2") + (("S3 T3",) if tile[0] == "1" else ("S2 T1",)):
                R.add("split %s %s %s" % (tile, k, st))
        R.add("tile %s general grouped" % tile)
        for st in ("S1 T3", "S2 T3", "S2 T2") + (("S3 T3",) if tile[0] == "1" else ()):
            R.add("split %s general %s grouped" % (tile, st))
    for k in ("dense", "general", "raw"):
        R |= {"mf16 128x128/4 %s T3" % k, "mf16 128x128/4 %s T2" % k, "mf16 128x128/4 %s T2 staged" % k, "mf16 256x128/8 %s T2 staged" % k}
    R |= {"mf16 128x128/4 general T3 grouped", "mf16 128x128/4 general T2 staged grouped"}
    for part in ("256x64/4 plain", "128x128/4 plain", "128x128/4 relu"):
        R |= {"splitk %s fin-dense" % part, "splitk %s fin-general" % part}
    return R


REACHABLE = _reachable()


# ---------------------------------------------------------------------------------------------- stride-2 data gradients by parity class
def s2_build(s, exact):
    """-> (dy4, w OIHW, [(Case, Operands)] per class of conv.s2_classes, expected dx [N, Hi, Wi, cin] float64): every class is a stride-1
    convolution of dy with its tap subset, stored at its parity positions of dx; positions of classes without taps stay zero."""
    from retinanet_mi355x import conv
    ex = "x" if exact else "r"
    draw = (lambda shape, i, std=1.0: _ints(shape, _seed(s.name + ex, i), -4, 4)) if exact else \
        (lambda shape, i, std=1.0: synth.normal(shape, _seed(s.name + ex, i), std))
    dy4 = draw((s.N, s.Ho, s.Wo, s.cout), 1)
    w = draw((s.cout, s.cin, s.k, s.k), 2, (2.0 / (s.k * s.k * s.cout)) ** 0.5)
    n_out = s.N * s.Hi * s.Wi * s.cin
    addb = draw((n_out,), 7) if s.add else None
    maskb = _ints((n_out,), _seed(s.name, 6), -2, 2) if s.mask else None
    Ha2, Wa2 = (s.Hi + 1) // 2, (s.Wi + 1) // 2
    add2b = draw((s.N * Ha2 * Wa2 * s.cin,), 8) if s.add2 else None
    dx = np.zeros(n_out)
    out = []
    for ci, (ph, pw, (r0, nr, s0, ns), (dh0, dw0)) in enumerate(conv.s2_classes(s.k, s.pad)):
        gh, gw = (s.Hi - ph + 1) // 2, (s.Wi - pw + 1) // 2
        d = dict(N=s.N, Hi=s.Ho, Wi=s.Wo, Cin=s.cout, Ho=gh, Wo=gw, Cout=s.cin, kh=nr, kw=ns, a=1, b=-1, p=dh0, p_w=dw0, div_shift=0,
                 os=2, oo_h=ph, oo_w=pw, Hy=s.Hi, Wy=s.Wi, add_mode=1 if s.add else 0, mask_mode=s.mask)
        if s.add2:
            d.update(add2_mode=3, Ha2=Ha2, Wa2=Wa2)
        c = Case("%s/class%d%d" % (s.name, ph, pw), d, {})
        o = Operands()
        o.x4, o.act, o.scale, o.shift, o.add, o.mask, o.add2 = dy4, 0, None, None, addb, maskb, add2b
        o.w5 = np.ascontiguousarray(w[:, :, r0::2, s0::2][:, :, :nr, :ns].transpose(1, 2, 3, 0))[None]     # [1][cin][i][j][cout]
        o.w = np.zeros((1, s.cin, c.kpad), dtype=np.float32)
        o.w[0, :, :c.K] = o.w5.reshape(s.cin, c.K)
        o.ysize = n_out
        v, off = reference(c, o)
        dx[(off[..., None] + np.arange(s.cin)).reshape(-1)] = v.reshape(-1)
        out.append((c, o))
    return dy4, w, out, dx.reshape(s.N, s.Hi, s.Wi, s.cin)


# ---------------------------------------------------------------------------------------------- configurations, applied
def apply_config(conv, config):
    """Product mode, conv.PRESPLIT and the run-time options of CONFIGS[config]; -> the state to hand to restore_config."""
    mode, presplit, opts = CONFIGS[config]
    ids = {"SPLITK": conv.OPT_SPLITK, "MF16": conv.OPT_MF16, "MF16_MIN": conv.OPT_MF16_MIN}
    before = (conv.get_fp32_mfma(), conv.PRESPLIT, {i: conv.get_option(i) for i in ids.values()})
    conv.set_fp32_mfma(mode)
    conv.PRESPLIT = presplit
    for name, i in ids.items():
        conv.set_option(i, opts.get(name, OPTION_DEFAULTS[name]))
    return before


def restore_config(conv, before):
    conv.set_fp32_mfma(before[0])
    conv.PRESPLIT = before[1]
    for i, v in before[2].items():
        conv.set_option(i, v)


def group_of(g, conv, fmt=0, word=None):
    """The ConvGroup of Group g as conv.conv_igemm_grouped fills it, with `word` (an address) for every pointer that only has to be there."""
    cg = conv._hip.ConvGroup()
    cg.n = len(g.cases)
    for i, c in enumerate(g.cases):
        d = desc_of(c, conv, fmt, x_amax=word if fmt == 3 else None, w_unscale=word if fmt == 3 else None)
        cg.d[i] = d
        cg.x[i], cg.y[i] = word, word
        cg.add[i], cg.mask[i] = (word if c.d["add_mode"] else None), (word if c.d["mask_mode"] else None)
    conv._tile_ends(cg, *((256, 64) if g.cases[0].d["Cout"] <= 64 else (128, 128)))
    return cg

"""Cases of tests/test_conv_launch_host.py: what the convolution launchers of csrc/conv_*.hip choose and refuse, on the host.

  desc(**over)        one legal rn_conv_desc as a dict of its fields (a 3x3 stride-1 pad-1 convolution 64 -> 256 on 2 x 24 x 40),
                      with the properties in `over` changed and the dense strides derived from the result
  TILE_CASES          (name, desc overrides, y_is_f32): the detector's own layer shapes (ResNet-50 at 8 x 1080 x 1920: bottlenecks,
                      pyramid, heads) and the base descriptor with one property changed at a time
  TILE_GROUPS         (name, list of desc overrides, y_is_f32): groups for the *_tile_rows queries
  TILE_EXPECTED       the recorded answers (see its comment)
  refusals(form)      per launcher the cases it must answer with RN_EINVAL: a legal call with exactly ONE rule of the launcher's checks
                      broken.  Every one of them is refused before the launcher's first HIP call (read off csrc/conv_launch.h and the
                      launchers), so they need no GPU -- and must never reach one: the pointers are made-up integers.
"""
RN_EINVAL = 10001
RN_MAX_GROUP = 5
RN_OPT_SPLITK, RN_OPT_BF16_P8, RN_OPT_FP8_P8 = 0, 5, 6
FP32_NATIVE, FP32_SPLIT, FP32_SPLIT3 = 0, 1, 2

# made-up device addresses (256-byte aligned); a launcher that refuses never looks behind them
PTR = dict(x=0x10000, w=0x20000, y=0x30000, add=0x40000, mask=0x50000, add2=0x60000)
SIGN, XAMAX, WUNSCALE = 0x70000, 0x80000, 0x90000


def desc(**over):
    d = dict(N=2, Hi=24, Wi=40, Cin=64, Ho=24, Wo=40, Cout=256, kh=3, kw=3, a=1, b=1, p=-1, p_w=-1, div_shift=0, act=1,
             add_mode=0, Ha=0, Wa=0, mask_mode=0, in_relu=0, os=1, oo_h=0, oo_w=0, Hy=None, Wy=None,
             add2_mode=0, Ha2=0, Wa2=0, add2_batch_stride=0, x_batch_stride=None, y_batch_stride=None, add_batch_stride=None,
             w_batch_stride=0, w_format=0, sign_out=0, x_amax=0, y_amax=0, w_unscale=0, x_amax_img_stride=0, x_amax_row_stride=0)
    d.update(over)
    if d["Hy"] is None:
        d["Hy"] = d["Ho"] * d["os"] if d["os"] > 0 else d["Ho"]
    if d["Wy"] is None:
        d["Wy"] = d["Wo"] * d["os"] if d["os"] > 0 else d["Wo"]
    if d["x_batch_stride"] is None:
        d["x_batch_stride"] = d["Hi"] * d["Wi"] * d["Cin"]
    if d["y_batch_stride"] is None:
        d["y_batch_stride"] = d["Hy"] * d["Wy"] * d["Cout"]
    if d["add_batch_stride"] is None:
        d["add_batch_stride"] = d["Ha"] * d["Wa"] * d["Cout"] if d["add_mode"] == 2 else d["y_batch_stride"]
    return d


def conv(N, H, W, cin, cout, k, stride=1, **over):
    """A forward convolution of the detector: k x k, pad k // 2."""
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    return dict(dict(N=N, Hi=H, Wi=W, Cin=cin, Ho=Ho, Wo=Wo, Cout=cout, kh=k, kw=k, a=stride, p=-(k // 2), p_w=-(k // 2)), **over)


LEVELS = [(135, 240), (68, 120), (34, 60), (17, 30), (9, 15)]                     # P3 .. P7 of a 1080 x 1920 frame
ANCHORS = sum(9 * h * w for h, w in LEVELS)

TILE_CASES = [
    # ---- ResNet-50 bottlenecks (D/utils.py:46-80) at 8 x 1080 x 1920
    ("l1_1x1_64_64", conv(8, 270, 480, 64, 64, 1), 0),
    ("l1_3x3_64_64", conv(8, 270, 480, 64, 64, 3), 0),
    ("l1_1x1_64_256_res", conv(8, 270, 480, 64, 256, 1, add_mode=1), 0),
    ("l1_1x1_256_64", conv(8, 270, 480, 256, 64, 1), 0),
    ("l2_1x1_256_128", conv(8, 270, 480, 256, 128, 1), 0),
    ("l2_3x3_128_128_s2", conv(8, 270, 480, 128, 128, 3, 2), 0),
    ("l2_1x1_256_512_s2", conv(8, 270, 480, 256, 512, 1, 2, act=0), 0),
    ("l2_1x1_128_512_res", conv(8, 135, 240, 128, 512, 1, add_mode=1), 0),
    ("l2_3x3_128_128", conv(8, 135, 240, 128, 128, 3), 0),
    ("l3_3x3_256_256_s2", conv(8, 135, 240, 256, 256, 3, 2), 0),
    ("l3_1x1_256_1024_res", conv(8, 68, 120, 256, 1024, 1, add_mode=1), 0),
    ("l3_1x1_1024_256", conv(8, 68, 120, 1024, 256, 1), 0),
    ("l3_3x3_256_256", conv(8, 68, 120, 256, 256, 3), 0),
    ("l4_3x3_512_512_s2", conv(8, 68, 120, 512, 512, 3, 2), 0),
    ("l4_1x1_512_2048_res", conv(8, 34, 60, 512, 2048, 1, add_mode=1), 0),
    ("l4_1x1_2048_512", conv(8, 34, 60, 2048, 512, 1), 0),
    ("l4_3x3_512_512", conv(8, 34, 60, 512, 512, 3), 0),
    # ---- a data gradient of a 3x3 (b = -1, p = +1) with the ReLU mask of its input
    ("l3_3x3_256_256_dgrad", conv(8, 68, 120, 256, 256, 3, b=-1, p=1, p_w=1, act=0, mask_mode=2), 0),
    # ---- pyramid (D/model.py:59-117)
    ("p5_1x1_2048_256", conv(8, 34, 60, 2048, 256, 1, act=0), 0),
    ("p4_1x1_1024_256_up", conv(8, 68, 120, 1024, 256, 1, act=0, add_mode=2, Ha=34, Wa=60), 0),
    ("p3_1x1_512_256_up", conv(8, 135, 240, 512, 256, 1, act=0, add_mode=2, Ha=68, Wa=120), 0),
    ("p3_3x3_256_256", conv(8, 135, 240, 256, 256, 3, act=0), 0),
    ("p6_3x3_2048_256_s2", conv(8, 34, 60, 2048, 256, 3, 2, act=0), 0),
    ("p7_3x3_256_256_s2", conv(8, 17, 30, 256, 256, 3, 2, act=0), 0),
    # ---- heads (D/model.py:120-205): tower layers per level, outputs into their slice of [B, A, n] as fp32
    ("head_p3", conv(8, 135, 240, 256, 256, 3), 0),
    ("head_p5", conv(8, 34, 60, 256, 256, 3), 0),
    ("head_p7", conv(8, 9, 15, 256, 256, 3), 0),
    ("head_reg_out_p3", conv(8, 135, 240, 256, 108, 3, act=0, y_batch_stride=ANCHORS * 12), 1),
    ("head_cls_out_p3", conv(8, 135, 240, 256, 72, 3, act=2, y_batch_stride=ANCHORS * 8), 1),
    ("head_cls_out_p7", conv(8, 9, 15, 256, 72, 3, act=2, y_batch_stride=ANCHORS * 8), 1),
    # ---- the base descriptor, one property changed at a time
    ("base", {}, 0),
    ("base_big", dict(N=8, Hi=135, Wi=240, Ho=135, Wo=240), 0),
    ("cin_96", dict(Cin=96), 0),
    ("cin_128", dict(Cin=128), 0),
    ("cout_8", dict(Cout=8), 0),
    ("cout_64", dict(Cout=64), 0),
    ("cout_264", dict(Cout=264), 0),
    ("big_cout_64", dict(N=8, Hi=135, Wi=240, Ho=135, Wo=240, Cout=64), 0),
    ("big_cout_264", dict(N=8, Hi=135, Wi=240, Ho=135, Wo=240, Cout=264), 0),
    ("big_cin_256", dict(N=8, Hi=135, Wi=240, Ho=135, Wo=240, Cin=256), 0),
    ("k4", dict(kh=4, kw=4, Ho=23, Wo=39), 0),
    ("k4_same", dict(kh=4, kw=4, p=-2, p_w=-2, Ho=25, Wo=41, Hi=25, Wi=41), 0),
    ("k5", dict(kh=5, kw=5, p=-2, p_w=-2), 0),
    ("stride_2", dict(a=2, Ho=12, Wo=20), 0),
    ("plane_differs", dict(p=0, p_w=0, Ho=22, Wo=38), 0),
    ("sparse_y", dict(y_batch_stride=24 * 40 * 256 + 512), 0),
    ("add_upsampled", dict(add_mode=2, Ha=12, Wa=20), 0),
    ("add_same", dict(add_mode=1), 0),
    ("mask_and_sign", dict(mask_mode=2, sign_out=SIGN), 0),
    ("mask_only", dict(mask_mode=2), 0),
    ("sign_only", dict(sign_out=SIGN), 0),
    ("sigmoid", dict(act=2), 0),
    ("y_is_f32", {}, 1),
    ("long_k_few_tiles", dict(N=1, Hi=9, Wi=15, Ho=9, Wo=15, Cin=2048), 0),
    ("long_k_narrow", dict(N=1, Hi=9, Wi=15, Ho=9, Wo=15, Cin=2048, Cout=64), 0),
]

_HEAD = [conv(8, h, w, 256, 256, 3) for h, w in LEVELS]
TILE_GROUPS = [
    ("head_tower", _HEAD, 0),
    ("head_tower_3_levels", _HEAD[2:], 0),
    ("head_tower_masked", [dict(d, mask_mode=2, act=0) for d in _HEAD], 0),
    ("head_reg_out", [conv(8, h, w, 256, 108, 3, act=0, y_batch_stride=ANCHORS * 12) for h, w in LEVELS], 1),
    ("head_cin_64", [conv(8, h, w, 64, 256, 3) for h, w in LEVELS], 0),
    ("head_cout_128", [conv(8, h, w, 256, 128, 3) for h, w in LEVELS], 0),
    ("head_one_strided", [conv(8, h, w, 256, 256, 3) for h, w in LEVELS[:2]] + [conv(8, 34, 60, 256, 256, 3, 2)], 0),
    ("small_planes", [conv(1, h, w, 64, 64, 3) for h, w in [(16, 16), (16, 24), (8, 8), (24, 24), (4, 4)]], 0),
]

# Recorded at the commit before the launch helpers were shared (tests/test_conv_launch_host.py: observe_tiles prints them).
#   TILE_EXPECTED[name]  = (by_mode, splitk_bytes, wants_f16) with by_mode[m] = (rn_conv_igemm_bf16_tile, rn_conv_igemm_bf16_tile_rows of the
#                          one-problem group, rn_conv_igemm_fp8_tile, rn_conv_igemm_fp8_tile_rows) under RN_OPT_BF16_P8 = RN_OPT_FP8_P8 = m,
#                          splitk_bytes = rn_conv_splitk_workspace_bytes with RN_OPT_SPLITK on, wants_f16 = rn_conv_igemm_wants_f16 in the
#                          (native, split, split3) product modes
#   GROUP_EXPECTED[name] = by_mode[m] = (rn_conv_igemm_bf16_tile_rows, rn_conv_igemm_fp8_tile_rows)
TILE_EXPECTED = {
    'l1_1x1_64_64': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l1_3x3_64_64': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l1_1x1_64_256_res': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l1_1x1_256_64': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l2_1x1_256_128': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l2_3x3_128_128_s2': (((128128, 256128, 128128, 128128), (128128, 256128, 256256, 128128), (128128, 256128, 256256, 128128)), 0, (0, 0, 1)),
    'l2_1x1_256_512_s2': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 0, (0, 0, 1)),
    'l2_1x1_128_512_res': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l2_3x3_128_128': (((128128, 256128, 128128, 128128), (128128, 256128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l3_3x3_256_256_s2': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 0, (0, 0, 1)),
    'l3_1x1_256_1024_res': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l3_1x1_1024_256': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l3_3x3_256_256': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l4_3x3_512_512_s2': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 0, (0, 0, 1)),
    'l4_1x1_512_2048_res': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l4_1x1_2048_512': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l4_3x3_512_512': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'l3_3x3_256_256_dgrad': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'p5_1x1_2048_256': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'p4_1x1_1024_256_up': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 0, (0, 0, 1)),
    'p3_1x1_512_256_up': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 0, (0, 0, 1)),
    'p3_3x3_256_256': (((128128, 256128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'p6_3x3_2048_256_s2': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 33423360, (0, 0, 1)),
    'p7_3x3_256_256_s2': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 9953280, (0, 0, 1)),
    'head_p3': (((128128, 256128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'head_p5': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'head_p7': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 9953280, (0, 0, 1)),
    'head_reg_out_p3': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 0, (0, 0, 1)),
    'head_cls_out_p3': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 0, (0, 0, 1)),
    'head_cls_out_p7': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 2799360, (0, 0, 1)),
    'base': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 3932160, (0, 0, 1)),
    'base_big': (((128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'cin_96': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 5898240, (0, 0, 1)),
    'cin_128': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 7864320, (0, 0, 1)),
    'cout_8': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (1256256, 256256, 128128, 128128)), 122880, (0, 0, 1)),
    'cout_64': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256)), 983040, (0, 0, 1)),
    'cout_264': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (1256256, 256256, 128128, 128128)), 4055040, (0, 0, 1)),
    'big_cout_64': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'big_cout_264': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (1256256, 256256, 128128, 128128)), 0, (0, 0, 1)),
    'big_cin_256': (((128128, 256128, 128128, 128128), (1256256, 256256, 256256, 256256), (1256256, 256256, 256256, 256256)), 0, (0, 0, 1)),
    'k4': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 7348224, (0, 0, 1)),
    'k4_same': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 8396800, (0, 0, 1)),
    'k5': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 11796480, (0, 0, 1)),
    'stride_2': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 983040, (0, 0, 1)),
    'plane_differs': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 128128), (128128, 128128, 256256, 128128)), 3424256, (0, 0, 1)),
    'sparse_y': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 3932160, (0, 0, 1)),
    'add_upsampled': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 3932160, (0, 0, 1)),
    'add_same': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 3932160, (0, 0, 1)),
    'mask_and_sign': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (128128, 128128, 256256, 256256)), 3932160, (0, 0, 1)),
    'mask_only': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 3932160, (0, 0, 1)),
    'sign_only': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 3932160, (0, 0, 1)),
    'sigmoid': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 3932160, (0, 0, 1)),
    'y_is_f32': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128)), 3932160, (0, 0, 1)),
    'long_k_few_tiles': (((128128, 128128, 128128, 128128), (128128, 128128, 256256, 256256), (1256256, 256256, 256256, 256256)), 4423680, (0, 0, 1)),
    'long_k_narrow': (((128128, 128128, 128128, 128128), (128128, 128128, 128128, 128128), (1256256, 256256, 256256, 256256)), 1105920, (0, 0, 1)),
}
GROUP_EXPECTED = {
    'head_tower': ((256128, 128128), (256256, 256256), (256256, 256256)),
    'head_tower_3_levels': ((128128, 128128), (128128, 256256), (256256, 256256)),
    'head_tower_masked': ((256128, 128128), (256256, 256256), (256256, 256256)),
    'head_reg_out': ((128128, 128128), (128128, 128128), (128128, 128128)),
    'head_cin_64': ((128128, 128128), (256256, 256256), (256256, 256256)),
    'head_cout_128': ((256128, 128128), (256128, 256256), (256256, 256256)),
    'head_one_strided': ((256128, 128128), (256128, 128128), (256128, 128128)),
    'small_planes': ((128128, 128128), (128128, 128128), (256256, 256256)),
}


# ------------------------------------------------------------------------------------------------ refusals
def _case(name, d=None, yf32=0, mode=FP32_SPLIT3, **ptrs):
    """One single-launch refusal: desc overrides, pointer overrides (add / mask / add2 default to present exactly when their mode asks)."""
    return dict(name=name, d=desc(**(d or {})), yf32=yf32, mode=mode, ptrs=ptrs)


def pointers(d, ptrs):
    """The pointer arguments of a case: PTR's, the optional operands present exactly when the descriptor asks, then the overrides."""
    p = dict(PTR)
    if d["add_mode"] == 0:
        p["add"] = 0
    if d["mask_mode"] == 0:
        p["mask"] = 0
    if d["add2_mode"] == 0:
        p["add2"] = 0
    p.update(ptrs)
    return p


def _desc_rules(form):
    """The descriptor rules every form shares (csrc/conv_launch.h: rn_check_desc_core), one case each; eb = bytes per element."""
    eb = {"fp32": 4, "bf16": 2, "fp8": 1}[form]
    c = [_case("N_0", dict(N=0)), _case("Hi_0", dict(Hi=0)), _case("Wi_0", dict(Wi=0)), _case("Ho_0", dict(Ho=0)),
         _case("Wo_negative", dict(Wo=-1)), _case("Cout_0", dict(Cout=0)),
         _case("Cin_0", dict(Cin=0)), _case("Cin_below_a_chunk", dict(Cin=8 // eb)),
         _case("Cin_not_whole_chunks", dict(Cin=64 + 8 // eb)),
         _case("image_past_2GiB", dict(Hi=16384, Wi=16384, Ho=16384, Wo=16384, Cin=16, Cout=16, N=1)),
         _case("x_batch_stride_negative", dict(x_batch_stride=-1)),
         _case("tile_span_past_2GiB", dict(x_batch_stride=1 << 31)),
         _case("weights_past_2GiB", dict(Cout=1 << 22)),
         _case("rows_past_2_31", dict(N=1 << 22)),
         _case("kh_0", dict(kh=0)), _case("kw_0", dict(kw=0)),
         _case("div_shift_negative", dict(div_shift=-1)), _case("div_shift_3", dict(div_shift=3)),
         _case("add_mode_negative", dict(add_mode=-1)), _case("add_mode_3", dict(add_mode=3)),
         _case("act_negative", dict(act=-1)), _case("act_3", dict(act=3)),
         _case("os_0", dict(os=0)), _case("oo_h_negative", dict(oo_h=-1, Hy=25)), _case("oo_w_negative", dict(oo_w=-1, Wy=41)),
         _case("rows_outside_Hy", dict(Hy=23)), _case("columns_outside_Wy", dict(Wy=39)),
         _case("offset_rows_outside_Hy", dict(os=2, oo_h=2)), _case("offset_columns_outside_Wy", dict(os=2, oo_w=2)),
         _case("strided_store_with_upsampled_add", dict(os=2, add_mode=2, Ha=12, Wa=20))]
    return c


def _mask_rules():
    """The mask / sign-bit rules of the fp32 and bf16 forms (the fp8 form has no mask at all)."""
    return [_case("mask_mode_negative", dict(mask_mode=-1)), _case("mask_mode_8", dict(mask_mode=8)),
            _case("mask_mode_3", dict(mask_mode=3)), _case("mask_mode_7", dict(mask_mode=7)),
            _case("mask_mode_bits_alone", dict(mask_mode=4)),
            _case("mask_bits_Cout_48", dict(mask_mode=6, Cout=48)),
            _case("mask_bits_y_stride_16", dict(mask_mode=5, y_batch_stride=24 * 40 * 256 + 16)),
            _case("sign_out_Cout_48", dict(sign_out=SIGN, Cout=48)),
            _case("sign_out_y_stride_16", dict(sign_out=SIGN, y_batch_stride=24 * 40 * 256 + 16))]


def _single_fp32():
    c = _desc_rules("fp32") + _mask_rules() + [
        _case("add2_mode_1", dict(add2_mode=1)), _case("add2_mode_2", dict(add2_mode=2)),
        _case("w_format_negative", dict(w_format=-1)), _case("w_format_4", dict(w_format=4)),
        _case("w_format_3_without_x_amax", dict(w_format=3, w_unscale=WUNSCALE)),
        _case("w_format_3_without_w_unscale", dict(w_format=3, x_amax=XAMAX)),
        _case("w_batch_stride_negative", dict(w_batch_stride=-1)),
        _case("w_batch_stride_plane_no_multiple_of_256", dict(w_batch_stride=256 * 576)),
        _case("add_without_add_mode", add=PTR["add"]), _case("add_mode_without_add", dict(add_mode=1), add=0),
        _case("mask_without_mask_mode", mask=PTR["mask"]), _case("mask_mode_without_mask", dict(mask_mode=2), mask=0),
        _case("add2_without_add2_mode", add2=PTR["add2"]),
        _case("add2_mode_without_add2", dict(add2_mode=3, Ha2=12, Wa2=20, add2_batch_stride=12 * 20 * 256), add2=0),
        _case("tiles_past_2_31", dict(N=(1 << 20) - 1, Hi=32, Wi=64, Ho=32, Wo=64, Cin=4, Cout=1 << 15, kh=1, kw=1, p=0, p_w=0)),
        _case("one_term_weights_wide", dict(w_format=2)),
        _case("one_term_weights_in_relu", dict(w_format=2, Cout=64, in_relu=1)),
        _case("presplit_weights_native_mode", dict(w_format=1), mode=FP32_NATIVE),
        _case("f16_weights_native_mode", dict(w_format=3, x_amax=XAMAX, w_unscale=WUNSCALE), mode=FP32_NATIVE)]
    return c


def _single_bf16():
    c = _desc_rules("bf16") + _mask_rules() + [
        _case("Cout_no_multiple_of_4", dict(Cout=254), yf32=1), _case("w_format_1", dict(w_format=1)),
        _case("in_relu", dict(in_relu=1)),
        _case("add2", dict(add2_mode=3, Ha2=12, Wa2=20, add2_batch_stride=12 * 20 * 256)),
        _case("w_batch_stride", dict(w_batch_stride=256 * 576, Hi=16, Wi=16, Ho=16, Wo=16)),
        _case("add_without_add_mode", add=PTR["add"]), _case("add_mode_without_add", dict(add_mode=1), add=0),
        _case("mask_without_mask_mode", mask=PTR["mask"]), _case("mask_mode_without_mask", dict(mask_mode=2), mask=0),
        _case("bf16_result_Cout_260", dict(Cout=260)),
        _case("add_at_8_bytes", dict(add_mode=1), add=PTR["add"] + 8),
        _case("add_at_4_bytes_f32_result", dict(add_mode=1), yf32=1, add=PTR["add"] + 4),
        _case("mask_at_8_bytes", dict(mask_mode=2), mask=PTR["mask"] + 8),
        _case("mask_at_4_bytes_f32_result", dict(mask_mode=2), yf32=1, mask=PTR["mask"] + 4),
        _case("mask_bits_at_2_bytes", dict(mask_mode=6), mask=PTR["mask"] + 2),
        _case("sign_out_f32_result", dict(sign_out=SIGN), yf32=1),
        _case("sign_out_at_2_bytes", dict(sign_out=SIGN + 2)),
        _case("x_at_8_bytes", x=PTR["x"] + 8), _case("y_at_8_bytes", y=PTR["y"] + 8), _case("w_at_8_bytes", w=PTR["w"] + 8),
        _case("y_batch_stride_no_multiple_of_8", dict(y_batch_stride=24 * 40 * 256 + 4)),
        _case("add_batch_stride_no_multiple_of_8", dict(add_mode=1, add_batch_stride=24 * 40 * 256 + 4)),
        _case("tiles_past_2_31", dict(N=(1 << 20) - 1, Hi=32, Wi=64, Ho=32, Wo=64, Cin=8, Cout=1 << 15, kh=1, kw=1, p=0, p_w=0))]
    return c


def _single_fp8():
    c = _desc_rules("fp8") + [
        _case("e4m3_result_Cout_264", dict(Cout=264)), _case("Cout_no_multiple_of_4", dict(Cout=254), yf32=1),
        _case("w_format_1", dict(w_format=1)), _case("mask", dict(mask_mode=2)), _case("in_relu", dict(in_relu=1)),
        _case("add2", dict(add2_mode=3, Ha2=12, Wa2=20, add2_batch_stride=12 * 20 * 256)),
        _case("w_batch_stride", dict(w_batch_stride=256 * 576, Hi=16, Wi=16, Ho=16, Wo=16)),
        _case("y_batch_stride_no_multiple_of_16", dict(y_batch_stride=24 * 40 * 256 + 8)),
        _case("add_batch_stride_no_multiple_of_4", dict(add_mode=1, add_batch_stride=24 * 40 * 256 + 2)),
        _case("add_without_add_mode", add=PTR["add"]), _case("add_mode_without_add", dict(add_mode=1), add=0),
        _case("x_at_8_bytes", x=PTR["x"] + 8), _case("w_at_8_bytes", w=PTR["w"] + 8), _case("y_at_8_bytes", y=PTR["y"] + 8),
        _case("add_at_2_bytes", dict(add_mode=1), add=PTR["add"] + 2),
        _case("tiles_past_2_31", dict(N=(1 << 20) - 1, Hi=32, Wi=64, Ho=32, Wo=64, Cin=16, Cout=1 << 15, kh=1, kw=1, p=0, p_w=0))]
    return c


# ---- groups: five pyramid levels of one layer (3x3, 64 -> 256, 2 images), then one thing wrong
GROUP_PLANES = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]


def _tiles(d, form):
    M = d["N"] * d["Ho"] * d["Wo"]
    if form == "fp32" and d["Cout"] <= 64:
        return (M + 255) // 256
    return ((M + 127) // 128) * ((d["Cout"] + 127) // 128)


def _group(name, form, change=None, all_=None, n=None, tile_end=None, yf32=0, mode=FP32_SPLIT3, w=None, **ptrs1):
    """A group refusal: `all_` overrides every problem's descriptor, `change` = (index, overrides) one problem's, ptrs1 the pointers of
    problem 1; tile_end follows the launcher's own tile for the (changed) descriptors unless given."""
    ds = [desc(**dict(dict(Hi=h, Wi=w_, Ho=h, Wo=w_), **(all_ or {}))) for h, w_ in GROUP_PLANES]
    if change is not None:
        i, over = change
        ds[i] = desc(**dict(dict(Hi=GROUP_PLANES[i][0], Wi=GROUP_PLANES[i][1], Ho=GROUP_PLANES[i][0], Wo=GROUP_PLANES[i][1]),
                            **dict(all_ or {}, **over)))
    ps = [pointers(d, ptrs1 if i == 1 else {}) for i, d in enumerate(ds)]
    ends, t = [], 0
    for d in ds:
        t += max(_tiles(d, form), 0) if d["Cout"] > 0 and d["N"] > 0 and d["Ho"] > 0 and d["Wo"] > 0 else 1
        ends.append(min(t, (1 << 31) - 1))
    if tile_end is not None:
        ends = tile_end(ends)
    return dict(name=name, ds=ds, ps=ps, n=len(ds) if n is None else n, tile_end=ends, yf32=yf32, mode=mode,
                w=PTR["w"] if w is None else w)


def _group_common(form):
    g = [_group("n_0", form, n=0), _group("n_6", form, n=RN_MAX_GROUP + 1), _group("n_negative", form, n=-1),
         _group("bad_descriptor_in_problem_1", form, change=(1, dict(kh=0))),
         _group("Cin_differs", form, change=(2, dict(Cin=128))),
         _group("Cout_differs", form, change=(2, dict(Cout=128))),
         _group("kh_differs", form, change=(3, dict(kh=1, p=0, Ho=GROUP_PLANES[3][0]))),
         _group("kw_differs", form, change=(3, dict(kw=1, p_w=0))),
         _group("add_without_add_mode", form, add=PTR["add"]),
         _group("add_mode_without_add", form, change=(1, dict(add_mode=1)), add=0),
         _group("tile_end_first_short", form, tile_end=lambda e: [e[0] - 1] + e[1:]),
         _group("tile_end_last_long", form, tile_end=lambda e: e[:-1] + [e[-1] + 1]),
         _group("tile_end_of_another_tile", form, tile_end=lambda e: [2 * v for v in e]),
         _group("tile_end_not_running", form, tile_end=lambda e: [e[0]] + [b - a for a, b in zip(e, e[1:])])]
    return g


def _grouped_fp32():
    return _group_common("fp32") + [
        _group("narrow_tile_end_of_the_wide_tile", "fp32", all_=dict(Cout=64),
               tile_end=lambda e: [15, 19, 20, 21, 22]),                       # running ceil(M / 128): e is [8, 10, 11, 12, 13]
        _group("add2", "fp32", change=(0, dict(add2_mode=3, Ha2=12, Wa2=20, add2_batch_stride=12 * 20 * 256))),
        _group("in_relu", "fp32", change=(4, dict(in_relu=1))),
        _group("mask_without_mask_mode", "fp32", mask=PTR["mask"]),
        _group("mask_mode_without_mask", "fp32", change=(1, dict(mask_mode=2)), mask=0),
        _group("w_format_differs", "fp32", change=(1, dict(w_format=1)), mode=FP32_SPLIT),
        _group("one_term_weights", "fp32", all_=dict(w_format=2, Cout=64)),
        _group("presplit_weights_native_mode", "fp32", all_=dict(w_format=1), mode=FP32_NATIVE)]


def _grouped_bf16():
    return _group_common("bf16") + [
        _group("act_differs", "bf16", change=(2, dict(act=0))),
        _group("w_at_8_bytes", "bf16", w=PTR["w"] + 8),
        _group("x_at_8_bytes", "bf16", x=PTR["x"] + 8), _group("y_at_8_bytes", "bf16", y=PTR["y"] + 8),
        _group("add_at_8_bytes", "bf16", change=(1, dict(add_mode=1)), add=PTR["add"] + 8),
        _group("mask_without_mask_mode", "bf16", mask=PTR["mask"]),
        _group("mask_mode_without_mask", "bf16", change=(1, dict(mask_mode=2)), mask=0),
        _group("sign_out_f32_result", "bf16", change=(1, dict(sign_out=SIGN)), yf32=1)]


def _grouped_fp8():
    return _group_common("fp8") + [
        _group("act_differs", "fp8", change=(2, dict(act=0))),
        _group("w_at_8_bytes", "fp8", w=PTR["w"] + 8),
        _group("x_at_8_bytes", "fp8", x=PTR["x"] + 8), _group("y_at_8_bytes", "fp8", y=PTR["y"] + 8),
        _group("add_at_2_bytes", "fp8", change=(1, dict(add_mode=1)), add=PTR["add"] + 2),
        _group("mask", "fp8", change=(1, dict(mask_mode=2)))]


def refusals(launcher):
    """launcher: rn_conv_igemm, rn_conv_igemm_grouped, rn_conv_igemm_bf16, ..._bf16_grouped, rn_conv_igemm_fp8, ..._fp8_grouped."""
    return {"rn_conv_igemm": _single_fp32, "rn_conv_igemm_grouped": _grouped_fp32,
            "rn_conv_igemm_bf16": _single_bf16, "rn_conv_igemm_bf16_grouped": _grouped_bf16,
            "rn_conv_igemm_fp8": _single_fp8, "rn_conv_igemm_fp8_grouped": _grouped_fp8}[launcher]()

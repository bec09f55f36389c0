"""Training-batch augmentation: the reference's ``Detection_Dataset.__getitem__`` (corrected_3D_dataset.py:296-498, CROP == 0)
split in two.

Host (this module): the random draws and the label transforms, tiny and in the reference's own fp64 torch operations, in the
reference's order -- ``np.random.seed(k)`` reproduces its numpy sequence.  The result per image is one fixed-size parameter
record (PARAMS_DTYPE = ``rn_augment_params`` of include/retinanet_mi355x.h) plus two resampling coefficient tables.

Device (csrc/augment.hip through ``ops.augment_frames``): every pixel -- resize, noise pad, flip, rotation, colour jitter,
normalisation and the tile swap -- byte for byte what torchvision's PIL backend computes.

Parity that is NOT pinned: the colour-jitter draws.  They follow torchvision's published ``RandomApply(p=0.5)`` and
``ColorJitter.get_params`` (one ``torch.rand`` for apply; ``torch.randperm(4)`` for the order, index 3 = hue = no-op; then
``uniform_`` factors for brightness U(0.4, 1.6), contrast U(0.4, 1.6), saturation U(0.5, 1.5)), but torchvision itself is not
available to check against, as for ``roi_align``.  Nor is the noise: the reference fills the pad with ``torch.rand`` on the host;
here the bytes come from a counter-based generator on the device (``noise_bytes`` restates it) unless the caller supplies them.

The crop mode (``CROP > 0``, :501-594, the crop detector's loader) is ``draw_crop`` / ``pack_crop_params`` / ``augment_crop_batch``
and csrc/augment_crop.hip through ``ops.augment_crops``: the same draws up to the rotation, then a window around one object (or
a random one), a second resize to ``crop x crop``, the jitter and sometimes an occluded region.  The device evaluates the window
only.  Two sources are unpinned there: the pad noise as above, and the occluded region's values, which the reference draws with
``torch.normal`` on the host and which here come from the device's generator (mean + std z, Box-Muller) unless the caller
supplies them.
"""
import math

import numpy as np
import torch

PARAMS_DTYPE = np.dtype([("affine", "<f8", 6), ("rh", "<i4"), ("rw", "<i4"), ("flip", "<i4"), ("apply", "<i4"),
                         ("order", "<i4", 4), ("dy", "<i4"), ("dx", "<i4"), ("factors", "<f4", 3), ("reserved", "<i4")])
assert PARAMS_DTYPE.itemsize == 104
CROP_PARAMS_DTYPE = np.dtype([("affine", "<f8", 6), ("rh", "<i4"), ("rw", "<i4"), ("flip", "<i4"), ("apply", "<i4"),
                              ("order", "<i4", 4), ("win", "<i4", 4), ("factors", "<f4", 3), ("occluded", "<i4"),
                              ("occlude", "<i4", 4)])                # rn_augment_crop_params
assert CROP_PARAMS_DTYPE.itemsize == 128
CROP_WIN_LIMIT = 16384         # the largest window edge rn_augment_crops takes
TAPS = 7                       # RN_AUG_TAPS: a table row is (first source index, TAPS coefficients): shrinking by up to 3x
PRECISION_BITS = 22
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
X_COLS = [0, 2, 4, 6, 8, 10, 12, 14, 16, 18]
Y_COLS = [1, 3, 5, 7, 9, 11, 13, 15, 17, 19]
SWAP_X = [2, 0, 6, 4, 10, 8, 14, 12, 18, 16]
SWAP_Y = [3, 1, 7, 5, 11, 9, 15, 13, 19, 17]


# ------------------------------------------------------------------------------------------------ draws
def draw_jitter():
    """transforms.RandomApply([ColorJitter(brightness=0.6, contrast=0.6, saturation=0.5)]) -> (apply, order[4], factors[3]).
    RandomApply returns the image unchanged when ``p < torch.rand(1)``; only an applied ColorJitter draws anything more."""
    if 0.5 < float(torch.rand(1)):
        return 0, [BRIGHTNESS, CONTRAST, SATURATION, HUE], [1.0, 1.0, 1.0]
    order = [int(v) for v in torch.randperm(4)]
    b = float(torch.empty(1).uniform_(0.4, 1.6))
    c = float(torch.empty(1).uniform_(0.4, 1.6))
    s = float(torch.empty(1).uniform_(0.5, 1.5))
    return 1, order, [b, c, s]


def draw_split(occupied, limit):
    """:440-451 (and :453-464): draw a split in [0, limit) until it cuts through no box, at most 10 failures; ``attempts`` counts
    failures only and the last failing draw is kept."""
    attempts, good, split = 0, False, None
    while not good and attempts < 10:
        good = True
        split = np.random.randint(0, limit)
        for lo, hi in occupied:
            if split > lo and split < hi:
                good = False
                attempts += 1
                break
    return split


def affine_coefficients(angle, W, H):
    """The destination -> source matrix of PIL's Image.rotate(angle) for expand=False: angle % 360, centre (W/2, H/2),
    cos / sin rounded to 15 decimals.  The device never evaluates a trigonometric function."""
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    x, y = -cx - 0, -cy - 0
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _vps_tensor(vps):
    """:307: a float32 tensor of the camera's three vanishing points."""
    v = np.asarray(vps, dtype=np.float64).reshape(-1)
    return torch.tensor([float(x) for x in v])


def _draw_common(labels, camera_id, vps, size):
    """:300-402, what both modes share: scale, aspect, FLIP and angle from the global ``np.random`` and the labels resized,
    flipped, rotated and filtered.  -> (params dict without the jitter, y [n,21], vps [6] float32)."""
    W, H = int(size[0]), int(size[1])
    no_labels = False
    y = labels.clone()
    vps = _vps_tensor(vps)
    if y.numel() == 0:                                                     # :311-318
        y = torch.zeros([1, 21]) - 1
        no_labels = True
    elif camera_id in ["p2c2", "p2c3", "p2c4"]:
        new_y = torch.clone(y)
        new_y[:, X_COLS] = y[:, SWAP_X]
        new_y[:, Y_COLS] = y[:, SWAP_Y]
        y = new_y
    scale = max(1, np.random.normal(1, 0.1))                               # :331-334
    aspect_ratio = max(0.75, np.random.normal(1, 0.2))
    rh, rw = int(H * scale * aspect_ratio), int(W * scale)
    y[:, X_COLS] = y[:, X_COLS] * scale                                    # :344-347
    y[:, Y_COLS] = y[:, Y_COLS] * scale * aspect_ratio
    vps[[0, 2, 4]] = vps[[0, 2, 4]] * scale
    vps[[1, 3, 5]] = vps[[1, 3, 5]] * scale * aspect_ratio
    FLIP = np.random.rand()                                                # :350-364
    if FLIP > 0.5:
        new_y = torch.clone(y)
        new_y[:, X_COLS] = W - y[:, SWAP_X]
        new_y[:, Y_COLS] = y[:, SWAP_Y]
        y = new_y
        new_vps = torch.clone(vps)
        vps[[0, 2, 4]] = W - new_vps[[0, 2, 4]]
        if no_labels:
            y = torch.zeros([1, 21]) - 1
    angle = (np.random.rand() * 40) - 20                                   # :368-390
    if not no_labels:
        y_mag = torch.sqrt((y[:, ::2][:, :-1] - W / 2.0) ** 2 + (y[:, 1::2] - H / 2.0) ** 2)
        y_theta = torch.atan2((y[:, 1::2] - H / 2.0), (y[:, ::2][:, :-1] - W / 2.0))
        y_theta -= angle * (np.pi / 180.0)
        y_new = torch.clone(y)
        y_new[:, ::2][:, :-1] = y_mag * torch.cos(y_theta)
        y_new[:, 1::2] = y_mag * torch.sin(y_theta)
        y_new[:, ::2][:, :-1] += W / 2.0
        y_new[:, 1::2] += H / 2.0
        y = y_new
        xmin = torch.min(y[:, ::2][:, :-1], dim=1)[0].unsqueeze(1)
        xmax = torch.max(y[:, ::2][:, :-1], dim=1)[0].unsqueeze(1)
        ymin = torch.min(y[:, 1::2], dim=1)[0].unsqueeze(1)
        ymax = torch.max(y[:, 1::2], dim=1)[0].unsqueeze(1)
        y[:, 16:20] = torch.cat([xmin, ymin, xmax, ymax], dim=1)
    xs_, ys_ = y[:, X_COLS], y[:, Y_COLS]                                  # :394-402
    keep = (xs_.min(1)[0] < W) & (xs_.max(1)[0] >= 0) & (ys_.min(1)[0] < H) & (ys_.max(1)[0] >= 0)
    y = y[keep] if bool(keep.any()) else torch.zeros([1, 21]) - 1
    params = dict(rh=rh, rw=rw, flip=int(FLIP > 0.5), angle=float(angle), affine=affine_coefficients(angle, W, H),
                  scale=float(scale), aspect=float(aspect_ratio))
    return params, y, vps


def draw(labels, camera_id, vps, size):
    """One image's draws and label transform.  labels: the dataset's [n,21] tensor (fp64 rows from the parser, one all-zero
    fp32 row for a frame without boxes, or [0,21]); vps: the camera's three (x, y) pairs; size: (W, H).
    Consumes the global ``np.random`` (scale, aspect, FLIP, angle, then TILE and the split attempts) and torch's global generator
    (the jitter draws, between angle and TILE) in the reference's order.  -> (params dict, labels [n,27] float32)."""
    W, H = int(size[0]), int(size[1])
    common, y, vps = _draw_common(labels, camera_id, vps, size)
    apply, order, factors = draw_jitter()                                  # :425 (self.im_tf)
    TILE = np.random.rand()                                                # :427-492
    dx = dy = 0
    if TILE > 0.25:
        ox0 = torch.min(y[:, 0:16:2], dim=1)[0]
        ox1 = torch.max(y[:, 0:16:2], dim=1)[0]
        oy0 = torch.min(y[:, 1:16:2], dim=1)[0]
        oy1 = torch.max(y[:, 1:16:2], dim=1)[0]
        xsplit = draw_split(list(zip(ox0.tolist(), ox1.tolist())), W)
        ysplit = draw_split(list(zip(oy0.tolist(), oy1.tolist())), H)
        if TILE > 0.25 and TILE < 0.5:
            dx = xsplit
        elif TILE > 0.5 and TILE < 0.75:
            dy, dx = ysplit, xsplit
        elif TILE > 0.75:
            dy = ysplit
        if TILE > 0.25 and TILE < 0.75:
            right = (ox0 > xsplit).unsqueeze(1)
            y[:, X_COLS] = torch.where(right, y[:, X_COLS] - xsplit, y[:, X_COLS] + (W - xsplit))
        if TILE > 0.5:
            below = (oy0 > ysplit).unsqueeze(1)
            y[:, Y_COLS] = torch.where(below, y[:, Y_COLS] - ysplit, y[:, Y_COLS] + (H - ysplit))
    vps = vps.unsqueeze(0).repeat(len(y), 1).float()                       # :495-497
    y = torch.cat((y.float(), vps), dim=1)
    params = dict(rh=common["rh"], rw=common["rw"], flip=common["flip"], angle=common["angle"], affine=common["affine"],
                  apply=apply, order=order, factors=factors, dy=int(dy), dx=int(dx),
                  scale=common["scale"], aspect=common["aspect"], tile=float(TILE))
    return params, y


def draw_crop(labels, camera_id, vps, size, crop):
    """One image's draws and label transform in the crop mode (:501-594), after the common part: with objects
    ``randint(len(y))``, ``normal(0, 20, size=2)`` and ``normal(size / 4, size / 4)`` place a window around one of them, without
    ``normal(300, 25)`` and two ``randint(100, 1000)`` place it anywhere; then the jitter draws (torch's generator), ``rand()`` for
    the occlusion and above 0.9 three ``randint`` for its region.  The reference's rules are restated as they are: "has objects" is
    ``y[0, 0] != -1`` (an all-zero row counts), ``int()`` truncates towards zero, the window is (minx, miny, maxx - minx,
    maxy - miny) -- may be negative, may differ by one in width and height -- the labels are scaled per axis, column 20 is shifted
    and scaled with the x columns and written back at the end.
    -> (params dict: ``draw``'s without dy / dx, plus win = (minx, miny, cw, ch), crop, occlude = (x0, y0, x1, y1) or None;
    labels [n,21]: fp64, or one fp32 -1 row)."""
    crop = int(crop)
    common, y, _ = _draw_common(labels, camera_id, vps, size)
    classes = y[:, 20].clone()                                             # :503
    if y[0, 0] != -1:                                                      # :505-521: one object defines the centre
        idx = np.random.randint(len(y))
        box = y[idx]
        centx = (box[16] + box[18]) / 2.0
        centy = (box[17] + box[19]) / 2.0
        noise = np.random.normal(0, 20, size=2)
        centx += noise[0]
        centy += noise[1]
        extent = max(box[19] - box[17], box[18] - box[16])
        extent_noise = max(-(extent * 1 / 4), np.random.normal(extent * 1 / 4, extent / 4))
        extent += extent_noise
        if extent < 50:
            extent = 50
    else:                                                                  # :522-525
        extent = max(50, np.random.normal(300, 25))
        centx = np.random.randint(100, 1000)
        centy = np.random.randint(100, 1000)
    minx = int(centx - extent / 2)                                         # :527-530
    miny = int(centy - extent / 2)
    maxx = int(centx + extent / 2)
    maxy = int(centy + extent / 2)
    cw, ch = maxx - minx, maxy - miny
    if cw <= 0 or ch <= 0:                                                 # :543-545: the reference raises as well
        raise ValueError("augment: empty crop window %r" % ((minx, miny, cw, ch),))
    if y[0, 0] != -1:                                                      # :549-552
        y[:, ::2] -= minx
        y[:, 1::2] -= miny
    y[:, ::2] *= crop / cw                                                 # :559-560
    y[:, 1::2] *= crop / ch
    if torch.sum(y) != 0:                                                  # :564-570
        keepers = []
        for i, item in enumerate(y):
            if item[16] < crop - 15 and item[18] > 0 + 15 and item[17] < crop - 15 and item[19] > 0 + 15:
                keepers.append(i)
        y = y[keepers]
        classes = classes[keepers]
    if len(y) == 0:                                                        # :572-574
        y = torch.zeros([1, 21]) - 1
        classes = torch.tensor([-1])
    apply, order, factors = draw_jitter()                                  # :577 (self.im_tf)
    OCCLUDE = np.random.rand()                                             # :579-586
    occlude = None
    if OCCLUDE > 0.9:
        yo_min = np.random.randint(crop / 3, crop)
        xo_min = np.random.randint(0, crop / 3)
        xo_max = np.random.randint(crop * 2 / 3, crop)
        occlude = (int(xo_min), int(yo_min), int(xo_max), crop)
    y[:, 20] = classes                                                     # :594
    params = dict(rh=common["rh"], rw=common["rw"], flip=common["flip"], angle=common["angle"], affine=common["affine"],
                  apply=apply, order=order, factors=factors, scale=common["scale"], aspect=common["aspect"],
                  win=(minx, miny, cw, ch), crop=crop, occlude=occlude, occlude_draw=float(OCCLUDE))
    return params, y


def identity_params(W, H):
    """The record that changes nothing: ``ops.augment_frames`` then equals ``ops.frame_ingest``."""
    return dict(rh=H, rw=W, flip=0, affine=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0], apply=0,
                order=[BRIGHTNESS, CONTRAST, SATURATION, HUE], factors=[1.0, 1.0, 1.0], dy=0, dx=0)


# ------------------------------------------------------------------------------------------------ records and tables
def resample_table(in_size, out_size, n_out):
    """PIL's bilinear (triangle) resampling coefficients for the first n_out of out_size outputs (Resample.c:
    precompute_coeffs + normalize_coeffs_8bpc) -> int32 [n_out, 1 + TAPS]: first source index, then the fixed-point taps
    (zero beyond a row's own).  ``weight((x - c + .5) * (1 / fs))``: the library multiplies by the reciprocal."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    if int(math.ceil(support)) * 2 + 1 > TAPS:
        raise ValueError("augment: shrinking %d -> %d needs more than %d taps" % (in_size, out_size, TAPS))
    ss = 1.0 / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    w = np.zeros((n_out, TAPS), np.float64)
    ww = np.zeros(n_out, np.float64)
    for j in range(TAPS):
        wj = np.maximum(0.0, 1.0 - np.abs((j + lo - center + 0.5) * ss))
        wj = np.where(lo + j < hi, wj, 0.0)
        w[:, j] = wj
        ww = ww + wj                                                       # left to right, as the C loop
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    table = np.zeros((n_out, 1 + TAPS), np.int32)
    table[:, 0] = lo
    table[:, 1:] = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)      # the weights are never negative
    return table


def crop_taps(size, crop):
    """The taps Pillow's bilinear filter takes per output when ``size`` pixels become ``crop``."""
    return int(math.ceil(max(size / crop, 1.0))) * 2 + 1


def resample_table_taps(in_size, out_size, n_out, taps):
    """``resample_table`` with a row of ``taps`` coefficients instead of TAPS: any shrink factor.  Equal to it at taps = TAPS."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    if int(math.ceil(support)) * 2 + 1 > taps:
        raise ValueError("augment: shrinking %d -> %d needs more than %d taps" % (in_size, out_size, taps))
    ss = 1.0 / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    w = np.zeros((n_out, taps), np.float64)
    ww = np.zeros(n_out, np.float64)
    for j in range(taps):
        wj = np.maximum(0.0, 1.0 - np.abs((j + lo - center + 0.5) * ss))
        wj = np.where(lo + j < hi, wj, 0.0)
        w[:, j] = wj
        ww = ww + wj                                                       # left to right, as the C loop
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    table = np.zeros((n_out, 1 + taps), np.int32)
    table[:, 0] = lo
    table[:, 1:] = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)      # the weights are never negative
    return table


def _pack_common(rec, i, p, W, H, tx, ty):
    if p["rh"] < 1 or p["rw"] < 1:
        raise ValueError("augment: resized size must be positive, got %r" % ((p["rh"], p["rw"]),))
    if sorted(p["order"]) != [0, 1, 2, 3]:
        raise ValueError("augment: the op order must be a permutation of 0..3, got %r" % (p["order"],))
    for k in ("rh", "rw", "flip", "apply"):
        rec[k][i] = p[k]
    rec["affine"][i] = p["affine"]
    rec["order"][i] = p["order"]
    rec["factors"][i] = p["factors"]
    nx, ny = min(p["rw"], W), min(p["rh"], H)
    tx[i, :nx] = resample_table(W, p["rw"], nx)
    ty[i, :ny] = resample_table(H, p["rh"], ny)


def pack_crop_params(params, W, H, crop):
    """A list of per-image dicts (``draw_crop``) -> (records CROP_PARAMS_DTYPE [B], table_x int32 [B,W,8], table_y int32
    [B,H,8] for the first resize as ``pack_params`` makes them, table_cx and table_cy int32 [B,crop,1+K] for the second resize
    cw -> crop and ch -> crop, K, win_max).  K is the batch's largest tap count and the stride of both second tables; win_max is
    the batch's largest window edge."""
    B, crop = len(params), int(crop)
    if crop < 1 or crop > CROP_WIN_LIMIT:
        raise ValueError("augment: crop must lie in [1, %d], got %d" % (CROP_WIN_LIMIT, crop))
    for p in params:
        minx, miny, cw, ch = (int(v) for v in p["win"])
        if not (1 <= cw <= CROP_WIN_LIMIT and 1 <= ch <= CROP_WIN_LIMIT and abs(minx) < 1 << 30 and abs(miny) < 1 << 30):
            raise ValueError("augment: crop window out of range: %r" % (tuple(p["win"]),))
        if int(p.get("crop", crop)) != crop:
            raise ValueError("augment: a record drawn for crop %r in a batch of crop %d" % (p["crop"], crop))
        if p.get("occlude") is not None:
            x0, y0, x1, y1 = (int(v) for v in p["occlude"])
            if not (0 <= x0 <= x1 <= crop and 0 <= y0 <= y1 <= crop):
                raise ValueError("augment: occlusion region outside the crop: %r" % (tuple(p["occlude"]),))
    K = max([crop_taps(max(int(p["win"][2]), int(p["win"][3])), crop) for p in params] + [3])
    rec = np.zeros(B, CROP_PARAMS_DTYPE)
    tx = np.zeros((B, W, 1 + TAPS), np.int32)
    ty = np.zeros((B, H, 1 + TAPS), np.int32)
    cx = np.zeros((B, crop, 1 + K), np.int32)
    cy = np.zeros((B, crop, 1 + K), np.int32)
    for i, p in enumerate(params):
        _pack_common(rec, i, p, W, H, tx, ty)
        rec["win"][i] = p["win"]
        if p.get("occlude") is not None:
            rec["occluded"][i] = 1
            rec["occlude"][i] = p["occlude"]
        cx[i] = resample_table_taps(int(p["win"][2]), crop, crop, K)
        cy[i] = resample_table_taps(int(p["win"][3]), crop, crop, K)
    win_max = max([max(int(p["win"][2]), int(p["win"][3])) for p in params] + [1])
    return rec, tx, ty, cx, cy, K, win_max


def pack_params(params, W, H):
    """A list of per-image dicts (``draw`` / ``identity_params``) -> (records PARAMS_DTYPE [B], table_x int32 [B,W,8],
    table_y int32 [B,H,8]).  Only the top-left min(h',H) x W of the resized image is ever read (w' >= W always in the
    reference; here any w' >= 1 works: columns past w' are pad)."""
    B = len(params)
    rec = np.zeros(B, PARAMS_DTYPE)
    tx = np.zeros((B, W, 1 + TAPS), np.int32)
    ty = np.zeros((B, H, 1 + TAPS), np.int32)
    for i, p in enumerate(params):
        if p["rh"] < 1 or p["rw"] < 1:
            raise ValueError("augment: resized size must be positive, got %r" % ((p["rh"], p["rw"]),))
        for k in ("rh", "rw", "flip", "apply", "dy", "dx"):
            rec[k][i] = p[k]
        if not (0 <= p["dy"] < H and 0 <= p["dx"] < W):
            raise ValueError("augment: roll offsets out of range: %r" % ((p["dy"], p["dx"]),))
        if sorted(p["order"]) != [0, 1, 2, 3]:
            raise ValueError("augment: the op order must be a permutation of 0..3, got %r" % (p["order"],))
        rec["affine"][i] = p["affine"]
        rec["order"][i] = p["order"]
        rec["factors"][i] = p["factors"]
        nx, ny = min(p["rw"], W), min(p["rh"], H)
        tx[i, :nx] = resample_table(W, p["rw"], nx)
        ty[i, :ny] = resample_table(H, p["rh"], ny)
    return rec, tx, ty


def noise_bytes(seed, B, H, W):
    """The device generator of csrc/augment.hip, restated: byte [b,y,x,c] = floor(fp32(k * 2^-24) * 255), k = the top 24 bits
    of splitmix64 keyed by (seed, element index)."""
    with np.errstate(over="ignore"):
        z = np.arange(B * H * W * 3, dtype=np.uint64) + np.uint64(seed & 0xFFFFFFFFFFFFFFFF) * np.uint64(0x9E3779B97F4A7C15)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u * np.float32(255.0)).astype(np.uint8).reshape(B, H, W, 3)


# ------------------------------------------------------------------------------------------------ batches
def collate(inputs):
    """The reference's collate (:714-741): stack the images, pad the labels with -1 rows to the batch's longest."""
    im = [item[0] for item in inputs]
    label = [item[1] for item in inputs]
    max_labels = max(len(l) for l in label)
    ims = torch.stack(im)
    size = len(label[0][0])
    labels = torch.zeros([len(label), max_labels, size]) - 1
    for idx in range(len(label)):
        labels[idx, :len(label[idx]), :] = label[idx]
    return ims, labels


def _align(n, a=256):
    return (n + a - 1) // a * a


def _upload(parts, device):
    """Several host arrays in ONE packed (pinned where possible) copy -> a function (index, dtype, shape) -> device view."""
    offs, total = [], 0
    for p in parts:
        offs.append(total)
        total = _align(total + p.nbytes)
    host = torch.empty(total, dtype=torch.uint8, pin_memory=torch.device(device).type == "cuda")
    hv = host.numpy()
    for o, p in zip(offs, parts):
        hv[o:o + p.nbytes] = p.reshape(-1).view(np.uint8)
    dev = host.to(device, non_blocking=True)
    return lambda i, dtype, shape: dev[offs[i]:offs[i] + parts[i].nbytes].view(dtype).view(shape)


def augment_batch(frames, labels, cameras, vps, device, noise=None, seed=0):
    """frames: B uint8 [H,W,3] arrays (or one [B,H,W,3]); labels: B label tensors; cameras: B camera ids; vps: B vanishing-point
    triples.  Makes the draws, uploads frames, parameter records, coefficient tables and the padded labels in ONE packed copy, runs
    the device chain and returns (im [B,3,H,W] float32, label [B,N,27] float32) on ``device``."""
    from . import ops
    B = len(frames)
    H, W = frames[0].shape[:2]
    drawn = [draw(labels[i], cameras[i], vps[i], (W, H)) for i in range(B)]
    rec, tx, ty = pack_params([d[0] for d in drawn], W, H)
    _, lab = collate([(torch.zeros(0), d[1]) for d in drawn])
    parts = [np.ascontiguousarray(np.stack([np.asarray(f) for f in frames]), dtype=np.uint8), rec, tx, ty, lab.numpy()]
    view = _upload(parts, device)
    im = ops.augment_frames(view(0, torch.uint8, (B, H, W, 3)), (view(1, torch.uint8, (B, PARAMS_DTYPE.itemsize)),
                                                                  view(2, torch.int32, tx.shape), view(3, torch.int32, ty.shape)),
                            noise=noise, seed=seed)
    return im, view(4, torch.float32, tuple(lab.shape)).clone()


def augment_crop_batch(frames, labels, cameras, vps, crop, device, noise=None, occlusion=None, seed=0):
    """``augment_batch`` for the crop mode: frames B uint8 [H,W,3]; labels, cameras, vps as there; crop: the output edge (the
    reference's CROP).  Makes the draws (``draw_crop``), uploads frames, records, the four coefficient tables and the padded labels
    in ONE packed copy, runs the device chain and returns (im [B,3,crop,crop] float32, label [B,N,21] float32) on ``device``.
    noise: optional uint8 [B,H,W,3] pad bytes; occlusion: optional float32 [B,3,crop,crop] values for the occluded regions (device
    tensors); both come from the device's generator keyed by ``seed`` otherwise."""
    from . import ops
    B, crop = len(frames), int(crop)
    H, W = frames[0].shape[:2]
    drawn = [draw_crop(labels[i], cameras[i], vps[i], (W, H), crop) for i in range(B)]
    rec, tx, ty, cx, cy, K, win_max = pack_crop_params([d[0] for d in drawn], W, H, crop)
    _, lab = collate([(torch.zeros(0), d[1]) for d in drawn])
    parts = [np.ascontiguousarray(np.stack([np.asarray(f) for f in frames]), dtype=np.uint8), rec, tx, ty, cx, cy, lab.numpy()]
    view = _upload(parts, device)
    im = ops.augment_crops(view(0, torch.uint8, (B, H, W, 3)),
                           (view(1, torch.uint8, (B, CROP_PARAMS_DTYPE.itemsize)), view(2, torch.int32, tx.shape),
                            view(3, torch.int32, ty.shape), view(4, torch.int32, cx.shape), view(5, torch.int32, cy.shape)),
                           K, win_max, crop, noise=noise, occlusion=occlusion, seed=seed)
    return im, view(6, torch.float32, tuple(lab.shape)).clone()


class AugmentedBatches:
    """``batches`` for ``trainer.train``: ``AugmentedBatches(frames, labels, cameras, vps, batch, device)(epoch)`` yields
    (im, label) on the device, augmented there.  frames: uint8 [N,H,W,3]; labels: N label tensors [n_i,21]; cameras: N camera ids;
    vps: {camera id: three (x, y) pairs}.  Each epoch visits the frames in a fresh ``np.random`` permutation; a last short batch
    is dropped.  The noise seed advances with every batch.  crop > 0: the crop mode, (im [B,3,crop,crop], label [B,N,21])."""

    def __init__(self, frames, labels, cameras, vps, batch, device, seed=0, crop=0):
        self.frames, self.labels, self.cameras, self.vps = frames, labels, cameras, vps
        self.batch, self.device, self.seed, self.crop = int(batch), device, int(seed), int(crop)

    def __len__(self):
        return len(self.frames) // self.batch

    def __call__(self, epoch):
        order = np.random.permutation(len(self.frames))
        for b in range(len(self)):
            idx = order[b * self.batch:(b + 1) * self.batch]
            if self.crop > 0:
                yield augment_crop_batch([self.frames[i] for i in idx], [self.labels[i] for i in idx],
                                         [self.cameras[i] for i in idx], [self.vps[self.cameras[i]] for i in idx], self.crop,
                                         self.device, seed=self.seed + (epoch * len(self) + b) * 1000003)
                continue
            yield augment_batch([self.frames[i] for i in idx], [self.labels[i] for i in idx], [self.cameras[i] for i in idx],
                                [self.vps[self.cameras[i]] for i in idx], self.device,
                                seed=self.seed + (epoch * len(self) + b) * 1000003)

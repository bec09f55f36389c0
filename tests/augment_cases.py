"""The image chain of the reference's training loader (corrected_3D_dataset.py: Detection_Dataset.__getitem__, :330-478,
CROP == 0), restated in numpy on bytes, and the cases of tests/golden/augment.npz.

What the reference does through torchvision's PIL backend, and what each step is here:
  F.resize (PIL bilinear)          -> resize():  Pillow's ImagingResample, triangle filter, horizontal pass then vertical,
                                      uint8 between them, 22-bit fixed-point coefficients
  to_tensor, torch.rand pad,       -> pad():     resized bytes survive /255 * 255; the rest is floor(fp32(u) * 255)
  to_pil_image (:336-342)
  F.hflip                          -> a mirrored column
  F.rotate(BILINEAR)               -> rotate():  Pillow's AFFINE transform with its bilinear filter, fill 0, in double
  ColorJitter (ImageEnhance)       -> jitter():  Image.blend(degenerate, image, factor) in fp32 per op
  ToTensor, Normalize              -> finish():  (byte / 255 - mean) / std in fp32
  the tile swap (:468-478)         -> a roll of the output index

Every function works on uint8 [H,W,3] arrays.  ``chain`` returns the bytes at every quantisation point, so a test can say
where a difference starts.  The keyword arguments named in MUTATIONS each break one rule; tests/test_augment_host.py
shows that every one of them is caught by the golden cases."""
import math

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
PRECISION_BITS = 22

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ resize
def resample_coeffs(in_size, out_size, support_one=False):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter -> (xmin [out], k [out, ksize] int64,
    zero beyond each row's own taps)."""
    scale = in_size / out_size
    fs = 1.0 if support_one else max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmin = np.zeros(out_size, np.int64)
    k = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [max(0.0, 1.0 - abs((x + lo - center + 0.5) * ss)) for x in range(hi - lo)]
        ww = sum(w)                                                  # left to right, as the C loop adds them
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx] = lo
        k[xx, :len(w)] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return xmin, k


def resize_pass(img, out_size, axis, support_one=False):
    """One pass along ``axis`` (1 = horizontal, 0 = vertical) of a uint8 [H,W,C] image."""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img.copy()
    xmin, k = resample_coeffs(in_size, out_size, support_one)
    shape = list(img.shape)
    shape[axis] = out_size
    acc = np.full(shape, 1 << (PRECISION_BITS - 1), np.int64)
    for j in range(k.shape[1]):
        idx = np.minimum(xmin + j, in_size - 1)
        kj = k[:, j].reshape([-1 if a == axis else 1 for a in range(3)])
        acc += np.take(img, idx, axis=axis).astype(np.int64) * kj
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, rh, rw, support_one=False, vertical_first=False):
    """PIL's img.resize((rw, rh), BILINEAR)."""
    if vertical_first:
        return resize_pass(resize_pass(img, rh, 0, support_one), rw, 1, support_one)
    return resize_pass(resize_pass(img, rw, 1, support_one), rh, 0, support_one)


def noise_bytes(u):
    """torch.rand values (fp32, k * 2^-24) -> the byte to_pil_image makes of them: floor(fp32(u) * 255)."""
    return (np.asarray(u, np.float32) * np.float32(255.0)).astype(np.uint8)


def pad(resized, noise_u8, H, W):
    """:338-342: the top-left min(h',H) x min(w',W) of the resized image over a noise image of the original size."""
    out = noise_u8.copy()
    h, w = min(resized.shape[0], H), min(resized.shape[1], W)
    out[:h, :w] = resized[:h, :w]
    return out


# ------------------------------------------------------------------------------------------------ rotate
def affine(angle, W, H):
    """Image.rotate's matrix (destination -> source) for expand=False, centre (W/2, H/2)."""
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    x, y = -cx - 0, -cy - 0
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def rotate(img, m, rounding=False):
    """ImagingTransform(AFFINE, BILINEAR) with fill 0: affine_transform + bilinear_filter32RGB of Geometry.c."""
    H, W = img.shape[:2]
    xin = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yin = np.arange(H, dtype=np.float64)[:, None] + 0.5
    sx = m[0] * xin + m[1] * yin + m[2]
    sy = m[3] * xin + m[4] * yin + m[5]
    inside = (sx >= 0.0) & (sx < W) & (sy >= 0.0) & (sy < H)
    fx, fy = sx - 0.5, sy - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    dx, dy = (fx - x0)[..., None], (fy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    f = img.astype(np.float64)
    v1, v2, v3, v4 = f[ya, xa], f[ya, xb], f[yb, xa], f[yb, xb]
    a = v1 + (v2 - v1) * dx
    b = v3 + (v4 - v3) * dx
    v = a + (b - a) * dy
    v = np.floor(v + 0.5) if rounding else np.trunc(v)
    return np.where(inside[..., None], v, 0.0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ colour jitter
def luma(img):
    """convert("L"): ITU-R 601-2 in 16-bit fixed point."""
    p = img.astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).astype(np.uint8)


def blend(a, p, f):
    """Image.blend(degenerate a, image p, f): t = a + f (p - a) in fp32; 0 if t <= 0, 255 if t >= 255, else truncated."""
    a32, p32 = a.astype(np.float32), p.astype(np.float32)
    t = a32 + np.float32(f) * (p32 - a32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def contrast_mean(img, no_half=False):
    """int(ImageStat.Stat(L).mean[0] + 0.5), as the integer expression the kernel uses: (2 S + N) // (2 N)."""
    L = luma(img)
    S, N = int(L.sum(dtype=np.int64)), L.size
    m = S // N if no_half else (2 * S + N) // (2 * N)
    assert no_half or m == int(S / N + 0.5)
    return m


def jitter(img, order, factors, mean_no_half=False, mean_before=False):
    """The ImageEnhance passes in the drawn order (HUE is a no-op: hue = 0 draws nothing and changes nothing).
    -> the image after every op, in order."""
    first, steps = img, []
    for op in order:
        if op == BRIGHTNESS:
            img = blend(np.zeros_like(img), img, factors[0])
        elif op == CONTRAST:
            m = contrast_mean(first if mean_before else img, mean_no_half)
            img = blend(np.full_like(img, m), img, factors[1])
        elif op == SATURATION:
            img = blend(np.repeat(luma(img)[..., None], 3, 2), img, factors[2])
        steps.append(img)
    return steps


# ------------------------------------------------------------------------------------------------ finish
def finish(img, dy, dx, reverse_roll=False):
    """ToTensor + Normalize in fp32, then the tile swap: out[:, y, x] = t[:, (y + dy) % H, (x + dx) % W]."""
    t = (img.astype(np.float32) / np.float32(255.0) - MEAN) / STD
    t = np.ascontiguousarray(t.transpose(2, 0, 1))
    s = 1 if reverse_roll else -1
    return np.roll(t, (s * dy, s * dx), axis=(1, 2))


def chain(frame, p, noise_u8, rotate_round=False, support_one=False, vertical_first=False, mean_no_half=False,
          mean_before=False, flip_after_rotate=False, reverse_roll=False):
    """frame uint8 [H,W,3]; p: dict(rh, rw, flip, affine[6], apply, order[4], factors[3], dy, dx); noise_u8 [H,W,3].
    -> dict of the bytes at every quantisation point and ``out`` fp32 [3,H,W]."""
    H, W = frame.shape[:2]
    r = {}
    # only the top-left min(h',H) x W of the resized image is ever read; Pillow computes all of it and so does this
    r["resized"] = resize(frame, p["rh"], p["rw"], support_one, vertical_first)
    r["padded"] = pad(r["resized"], noise_u8, H, W)
    if flip_after_rotate:
        r["flipped"] = r["padded"]
        r["rotated"] = rotate(r["padded"], p["affine"], rotate_round)
        if p["flip"]:
            r["rotated"] = r["rotated"][:, ::-1].copy()
    else:
        r["flipped"] = r["padded"][:, ::-1].copy() if p["flip"] else r["padded"]
        r["rotated"] = rotate(r["flipped"], p["affine"], rotate_round)
    r["jitter_steps"] = jitter(r["rotated"], p["order"], p["factors"], mean_no_half, mean_before) if p["apply"] else []
    r["jittered"] = r["jitter_steps"][-1] if r["jitter_steps"] else r["rotated"]
    r["out"] = finish(r["jittered"], p["dy"], p["dx"], reverse_roll)
    return r


MUTATIONS = {"rotate_round": "rounding instead of truncation in rotate",
             "support_one": "support 1 instead of the filter scale when shrinking",
             "vertical_first": "vertical pass before horizontal",
             "mean_no_half": "the contrast mean without the +.5",
             "mean_before": "the contrast mean taken before the earlier ops",
             "flip_after_rotate": "flip applied after the rotation",
             "reverse_roll": "roll direction reversed"}


# ------------------------------------------------------------------------------------------------ golden cases
SHAPES = {"a": (50, 38), "b": (41, 27), "c": (96, 64)}          # (W, H)
CLASS_NAMES = ["sedan", "midsize", "van", "pickup", "semi", "truck (other)", "motorcycle", "trailer"]
VPS = {"p1c1": [[-310.5, 12.25], [2100.75, -55.5], [48.0, 3000.5]],
       "p1c4": [[820.125, -140.0], [-1500.5, 260.75], [51.5, -2400.0]],
       "p2c3": [[1300.0, 44.5], [-640.25, 18.0], [70.75, 5100.0]]}

# (name, shape key, camera, boxes, seed).  boxes: a count = that many boxes inside the frame; "none" = an empty list
# in labels.cpkl (the parser makes one all-zero row of it); "empty" = a [0,21] label tensor (the no_labels path);
# "corner" = one small box in the top-left corner, which +-20 degrees turns out of the image.
# The seeds were searched for once; tools/make_golden.py (gen_augment) asserts what the set covers.
GOLDEN = [("a0", "a", "p1c1", "3", 71), ("a1", "a", "p2c3", "2", 8), ("a2", "a", "p1c4", "none", 4),
          ("a3", "a", "p1c1", "empty", 20), ("a4", "a", "p1c4", "corner", 9),
          ("b0", "b", "p1c1", "1", 9), ("b1", "b", "p2c3", "4", 0), ("b2", "b", "p1c4", "empty", 1), ("b3", "b", "p1c1", "corner", 10),
          ("c0", "c", "p1c1", "5", 5), ("c1", "c", "p2c3", "2", 6), ("c2", "c", "p1c4", "3", 7)]


def frame_bytes(name, W, H):
    """A deterministic uint8 [H,W,3] frame with edges, gradients and texture (so that every filter tap matters)."""
    rng = np.random.RandomState(sum(map(ord, name)) * 7919 % (1 << 31))
    y, x = np.mgrid[0:H, 0:W]
    f = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x // 5 + y // 3) % 2) * 200 + 20], -1)
    f = f + rng.randint(-40, 41, size=f.shape)
    return np.clip(f, 0, 255).astype(np.uint8)


def boxes_rows(name, kind, W, H):
    """Label rows as labels.cpkl holds them (lists of strings; [3] class, [4:8] 2D box, [11:27] the 8 corners)."""
    if kind in ("none", "empty"):
        return []
    rng = np.random.RandomState(sum(map(ord, name)) * 104729 % (1 << 31))
    rows = []
    n = 1 if kind == "corner" else int(kind)
    for i in range(n):
        if kind == "corner":
            cx, cy, w, h = 2.0, 1.5, 2.0, 1.0
        else:
            w, h = rng.uniform(4, W / 3), rng.uniform(3, H / 3)
            cx, cy = rng.uniform(w, W - w), rng.uniform(h, H - h)
        base = np.array([[cx + w / 2, cy + h / 2], [cx - w / 2, cy + h / 2], [cx + w / 3, cy], [cx - w / 3, cy]])   # right first
        top = base - np.array([0.0, h / 2]) + rng.uniform(-0.5, 0.5, size=(4, 2)) * (kind != "corner")
        pts = np.concatenate([base, top]).round(3)
        row = [""] * 27
        row[3] = CLASS_NAMES[int(rng.randint(len(CLASS_NAMES)))]
        row[4:8] = [repr(float(v)) for v in (pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max())]
        row[11:27] = [repr(float(v)) for v in pts.reshape(-1)]
        rows.append(row)
    return rows


def write_dataset(tmp, frames):
    """A dataset directory in the reference's format for the golden cases, with the frames cached as .npy arrays (the drop-in
    reads those without an image library).  frames: {name: uint8 [H,W,3]} -> {path: name}"""
    import os
    import pickle
    all_data, names = [], {}
    for i, (name, shape, camera, kind, seed) in enumerate(GOLDEN):
        W, H = SHAPES[shape]
        path = os.path.join(str(tmp), "%s_0_%d.npy" % (camera, i))
        np.save(path, frames[name])
        all_data.append([path, boxes_rows(name, kind, W, H)])
        names[path] = name
    with open(os.path.join(str(tmp), "labels.cpkl"), "wb") as f:
        pickle.dump(all_data, f)
    with open(os.path.join(str(tmp), "camera_vps.cpkl"), "wb") as f:
        pickle.dump(VPS, f)
    return names


def unpack_golden(g, name):
    """One item of tests/golden/augment.npz -> dict."""
    d = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    d["params"] = dict(rh=int(d["draws"][0]), rw=int(d["draws"][1]), flip=int(d["draws"][2]), apply=int(d["draws"][3]),
                       order=[int(v) for v in d["order"]], factors=[float(v) for v in d["factors"]],
                       dy=int(d["draws"][4]), dx=int(d["draws"][5]))
    H, W = d["frame"].shape[:2]
    d["params"]["affine"] = affine(float(d["scalars"][2]), W, H)
    return d

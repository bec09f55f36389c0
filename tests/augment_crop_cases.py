"""The crop mode of the reference's training loader (corrected_3D_dataset.py: Detection_Dataset.__getitem__ with CROP > 0,
:330-390 and :501-594), restated in numpy on bytes, and the cases of tests/golden/augment_crop.npz.

Up to the rotation the chain is that of tests/augment_cases.py (resize, pad, flip, rotate).  Then:
  F.crop (PIL crop)                -> window():   the box (minx, miny, minx + cw, miny + ch) of the rotated image; Pillow fills
                                      what lies outside the image with zero
  F.resize(im_crop, (CROP, CROP))  -> ac.resize:  the same two-pass triangle filter, now with as many taps as the shrink needs
  ColorJitter, ToTensor, Normalize -> ac.jitter, ac.finish (no tile swap)
  the occlusion (:579-592)         -> occlude():  raw values replace the NORMALISED ones inside the region
and, for the labels, the window from the drawn centre and size (``window_from``: int() truncates towards zero) and the shift
and per-axis scale (``labels``).  The keyword arguments named in MUTATIONS each break one rule;
tests/test_augment_crop_host.py shows that every one of them is caught by the golden cases."""
import numpy as np

import augment_cases as ac


def window(img, win, clamp=False):
    """PIL's img.crop((minx, miny, minx + cw, miny + ch)) of a uint8 [H,W,3] image: zero outside the image."""
    minx, miny, cw, ch = (int(v) for v in win)
    H, W = img.shape[:2]
    ys, xs = np.arange(miny, miny + ch), np.arange(minx, minx + cw)
    out = img[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)].copy()
    if not clamp:
        inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        out[~inside] = 0
    return out


def occlude(out, region, values, before_normalise=False):
    """:588-592: inside region = (x0, y0, x1, y1) the values [3,cs,cs] replace the normalised image's."""
    x0, y0, x1, y1 = (int(v) for v in region)
    out = out.copy()
    v = np.asarray(values, np.float32)
    if before_normalise:
        v = (v - ac.MEAN[:, None, None]) / ac.STD[:, None, None]
    out[:, y0:y1, x0:x1] = v[:, y0:y1, x0:x1]
    return out


def chain(frame, p, noise_u8, occlusion=None, crop_before_rotate=False, clamp_fill=False, support_one=False,
          occlude_before_normalise=False):
    """frame uint8 [H,W,3]; p: dict(rh, rw, flip, affine[6], apply, order[4], factors[3], win[4], crop, occlude or None);
    noise_u8 [H,W,3]; occlusion fp32 [3,cs,cs] -> dict of the bytes at every quantisation point and ``out`` fp32 [3,cs,cs]."""
    H, W = frame.shape[:2]
    cs = int(p["crop"])
    r = {}
    r["padded"] = ac.pad(ac.resize(frame, p["rh"], p["rw"]), noise_u8, H, W)
    flipped = r["padded"][:, ::-1].copy() if p["flip"] else r["padded"]
    if crop_before_rotate:
        w = window(flipped, p["win"])
        r["window"] = ac.rotate(w, ac.affine(p["angle"], w.shape[1], w.shape[0]))
    else:
        r["rotated"] = ac.rotate(flipped, p["affine"])
        r["window"] = window(r["rotated"], p["win"], clamp_fill)
    r["second"] = ac.resize(r["window"], cs, cs, support_one)
    r["jitter_steps"] = ac.jitter(r["second"], p["order"], p["factors"]) if p["apply"] else []
    r["jittered"] = r["jitter_steps"][-1] if r["jitter_steps"] else r["second"]
    r["out"] = ac.finish(r["jittered"], 0, 0)
    if p.get("occlude") is not None:
        r["out"] = occlude(r["out"], p["occlude"], occlusion, occlude_before_normalise)
    return r


def window_from(center, size, floor=False):
    """:527-530: (minx, miny, cw, ch) from the drawn centre and size; int() truncates towards zero."""
    cut = (lambda v: int(np.floor(v))) if floor else int
    cx, cy = center
    minx, miny, maxx, maxy = cut(cx - size / 2), cut(cy - size / 2), cut(cx + size / 2), cut(cy + size / 2)
    return minx, miny, maxx - minx, maxy - miny


def labels(y_rot, win, cs, swapped=False):
    """:503, :549-574, :594 on the labels as they leave the rotation (numpy [n,21]) -> [m,21], dtype included."""
    y = np.array(y_rot, copy=True)
    minx, miny, cw, ch = (int(v) for v in win)
    classes = y[:, 20].copy()
    if y[0, 0] != -1:
        y[:, ::2] -= minx                                                   # column 20 as well; written back below
        y[:, 1::2] -= miny
    sx, sy = (cs / ch, cs / cw) if swapped else (cs / cw, cs / ch)
    y[:, ::2] *= sx
    y[:, 1::2] *= sy
    if y.sum() != 0:
        keep = [i for i, r in enumerate(y) if r[16] < cs - 15 and r[18] > 15 and r[17] < cs - 15 and r[19] > 15]
        y, classes = y[keep], classes[keep]
    if len(y) == 0:
        y, classes = np.zeros((1, 21), np.float32) - 1, np.array([-1])
    y[:, 20] = classes
    return y


MUTATIONS = {"crop_before_rotate": "the window cut out before the rotation",
             "clamp_fill": "edge pixels instead of zero outside the frame",
             "floor_window": "floor instead of truncation for the window",
             "swapped_label_scale": "width and height swapped in the label scale",
             "support_one": "support 1 instead of the filter scale when shrinking",
             "occlude_before_normalise": "occlusion applied before normalisation"}


def mutation_caught(d, y_rot, mutation):
    """Does golden item d (``unpack_golden``) tell the mutated restatement from the reference?"""
    if mutation == "floor_window":
        return window_from(d["center"], float(d["size"]), floor=True) != tuple(int(v) for v in d["win"])
    if mutation == "swapped_label_scale":
        got = labels(y_rot, d["win"], int(d["cs"]), swapped=True)
        return got.shape != d["y"].shape or not np.array_equal(got, d["y"])
    return not np.array_equal(chain(d["frame"], d["params"], d["noise"], d["occlusion"], **{mutation: True})["out"], d["im_t"])


# ------------------------------------------------------------------------------------------------ golden cases
SHAPES = {"p": (128, 96), "q": (50, 38), "r": (160, 120)}          # (W, H)

# (name, shape key, camera, boxes, seed, cs).  boxes as in tests/augment_cases.py.  The seeds were searched for once;
# tools/make_golden.py (gen_augment_crop) asserts what the set covers.
GOLDEN = [("p0", "p", "p1c1", "3", 16, 24), ("p1", "p", "p2c3", "2", 19, 32), ("p2", "p", "p1c4", "1", 28, 24),
          ("p3", "p", "p1c1", "empty", 0, 32),
          ("q0", "q", "p1c1", "2", 16, 24), ("q1", "q", "p2c3", "1", 0, 32), ("q2", "q", "p1c4", "none", 0, 24),
          ("q3", "q", "p1c1", "empty", 787, 24), ("q4", "q", "p1c4", "empty", 769, 32), ("q5", "q", "p1c4", "corner", 0, 32),
          ("q6", "q", "p1c1", "3", 0, 32), ("q7", "q", "p1c4", "2", 0, 24),
          ("r0", "r", "p1c1", "2", 8, 112)]


def case_golden(case):
    """A case in the form tests/augment_cases.py's helpers take."""
    return case[:5]


def write_dataset(tmp, frames):
    """As augment_cases.write_dataset, for these cases.  -> {path: name}"""
    import os
    import pickle
    all_data, names = [], {}
    for i, (name, shape, camera, kind, seed, cs) in enumerate(GOLDEN):
        W, H = SHAPES[shape]
        path = os.path.join(str(tmp), "%s_0_%d.npy" % (camera, i))
        np.save(path, frames[name])
        all_data.append([path, ac.boxes_rows(name, kind, W, H)])
        names[path] = name
    with open(os.path.join(str(tmp), "labels.cpkl"), "wb") as f:
        pickle.dump(all_data, f)
    with open(os.path.join(str(tmp), "camera_vps.cpkl"), "wb") as f:
        pickle.dump(ac.VPS, f)
    return names


def unpack_golden(g, name):
    """One item of tests/golden/augment_crop.npz -> dict."""
    d = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    H, W = d["frame"].shape[:2]
    region = tuple(int(v) for v in d["region"])
    d["params"] = dict(rh=int(d["draws"][0]), rw=int(d["draws"][1]), flip=int(d["draws"][2]), apply=int(d["draws"][3]),
                       order=[int(v) for v in d["order"]], factors=[float(v) for v in d["factors"]],
                       angle=float(d["scalars"][2]), affine=ac.affine(float(d["scalars"][2]), W, H),
                       win=tuple(int(v) for v in d["win"]), crop=int(d["cs"]), occlude=region if int(d["draws"][4]) else None)
    return d

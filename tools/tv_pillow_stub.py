"""A stand-in for the part of ``torchvision.transforms`` that the reference's training loader uses, as thin Pillow wrappers
(torchvision is not installed; its PIL backend is itself a thin wrapper over Pillow).  Only tools/make_golden.py installs it.

Written from torchvision's published behaviour: ``resize`` / ``crop`` / ``hflip`` / ``rotate`` / ``adjust_*`` call the Pillow method of the
same meaning; ``to_tensor`` is uint8 / 255 in fp32; ``to_pil_image`` is ``mul(255).byte()``; ``Normalize`` is ``sub_(mean).div_(std)``;
``RandomApply`` skips when ``p < torch.rand(1)``; ``ColorJitter.get_params`` draws ``randperm(4)`` and then one ``uniform_`` per
active factor (hue = 0 is inactive: no draw, no pass).  What the draws are is therefore "parity unpinned".

Every call appends (name, payload) to LOG, so that the golden can record the draws and the bytes at every step."""
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageEnhance

LOG = []


def _u8(img):
    return np.array(img, copy=True)


def resize(img, size, interpolation=Image.BILINEAR):
    out = img.resize(tuple(size[::-1]), interpolation)
    LOG.append(("resize", (tuple(int(s) for s in size), _u8(out))))
    return out


def crop(img, top, left, height, width):
    out = img.crop((left, top, left + width, top + height))
    LOG.append(("crop", ((int(left), int(top), int(width), int(height)), _u8(out))))
    return out


def to_tensor(pic):
    a = torch.from_numpy(_u8(pic))
    return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def to_pil_image(pic):
    out = Image.fromarray(np.ascontiguousarray(pic.mul(255).byte().permute(1, 2, 0).numpy()), "RGB")
    LOG.append(("to_pil_image", _u8(out)))
    return out


def hflip(img):
    out = img.transpose(Image.FLIP_LEFT_RIGHT)
    LOG.append(("hflip", _u8(out)))
    return out


def rotate(img, angle, resample=Image.NEAREST, expand=False, center=None, fill=None):
    out = img.rotate(angle, resample, expand, center, fillcolor=fill)
    LOG.append(("rotate", (float(angle), _u8(out))))
    return out


def adjust_brightness(img, f):
    return ImageEnhance.Brightness(img).enhance(f)


def adjust_contrast(img, f):
    return ImageEnhance.Contrast(img).enhance(f)


def adjust_saturation(img, f):
    return ImageEnhance.Color(img).enhance(f)


def normalize(tensor, mean, std):
    tensor = tensor.clone()
    mean = torch.as_tensor(mean, dtype=tensor.dtype)
    std = torch.as_tensor(std, dtype=tensor.dtype)
    return tensor.sub_(mean[:, None, None]).div_(std[:, None, None])


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


class RandomApply:
    def __init__(self, transforms, p=0.5):
        self.transforms, self.p = transforms, p

    def __call__(self, img):
        skip = bool(self.p < torch.rand(1))
        LOG.append(("apply", int(not skip)))
        if skip:
            return img
        for t in self.transforms:
            img = t(img)
        return img


class ColorJitter:
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        def span(v):
            return None if v == 0 else (max(0.0, 1.0 - v), 1.0 + v)
        self.brightness, self.contrast, self.saturation = span(brightness), span(contrast), span(saturation)
        assert hue == 0

    def __call__(self, img):
        fn_idx = torch.randperm(4)
        b, c, s = (None if r is None else float(torch.empty(1).uniform_(r[0], r[1]))
                   for r in (self.brightness, self.contrast, self.saturation))
        LOG.append(("jitter", ([int(i) for i in fn_idx], [b, c, s])))
        for fn_id in fn_idx:
            if fn_id == 0 and b is not None:
                img = adjust_brightness(img, b)
            elif fn_id == 1 and c is not None:
                img = adjust_contrast(img, c)
            elif fn_id == 2 and s is not None:
                img = adjust_saturation(img, s)
            LOG.append(("jitter_step", _u8(img)))
        return img


class ToTensor:
    def __call__(self, pic):
        LOG.append(("to_tensor", _u8(pic)))
        return to_tensor(pic)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, tensor):
        return normalize(tensor, self.mean, self.std)


def install():
    """Put the stand-ins into sys.modules as torchvision.transforms and torchvision.transforms.functional."""
    me = sys.modules[__name__]
    tv = sys.modules.get("torchvision") or types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    for n in ("resize", "crop", "to_tensor", "to_pil_image", "hflip", "rotate", "adjust_brightness", "adjust_contrast",
              "adjust_saturation", "normalize"):
        setattr(tvf, n, getattr(me, n))
    for n in ("Compose", "RandomApply", "ColorJitter", "ToTensor", "Normalize"):
        setattr(tvt, n, getattr(me, n))
    tvt.functional = tvf
    tv.transforms = tvt
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tvt
    sys.modules["torchvision.transforms.functional"] = tvf

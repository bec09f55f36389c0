"""Drop-in for the reference's ``corrected_3D_dataset.py``: ``Detection_Dataset`` and ``collate`` for the detector's trainer
(train_detector_3D_angle.py:298-307), with the augmentation on the device.

    from corrected_3D_dataset import Detection_Dataset, collate          # the same two lines as before
    loader = data.DataLoader(Detection_Dataset(dir, CROP=0), batch_size=8, shuffle=True, collate_fn=collate)

What stays as in the reference (:169-294): ``labels.cpkl`` parsing, ``camera_vps.cpkl`` from the working directory, the
``random.shuffle`` and the 90/10 split.  What moves: ``__getitem__`` returns the undecorated uint8 frame with its labels, camera
id and vanishing points, and ``collate`` makes the reference's draws (retinanet_mi355x.augment.draw, in its order), uploads the
batch in one packed copy and runs the image chain on the device (csrc/augment.hip).  It returns ``(im [B,3,H,W], label [B,N,27])``
on the device, so the trainer's ``.to(device)`` is a no-op.

The crop detector's trainer (train_crop_detector.py) changes one line:

    from corrected_3D_dataset import Crop_Dataset as Detection_Dataset, collate
    loader = data.DataLoader(Detection_Dataset(dir, label_format="8_corners", mode="train", CROP=112), batch_size=12, ...)

``Crop_Dataset`` parses, shuffles and splits as ``Detection_Dataset`` does; its items carry CROP as a fifth entry, by which
``collate`` tells the two modes apart, and ``collate`` returns ``(im [B,3,CROP,CROP], label [B,N,21])`` on the device (the crop
mode of the reference, :501-594: retinanet_mi355x.augment.draw_crop, csrc/augment_crop.hip).  ``Detection_Dataset(CROP > 0)``
still raises NotImplementedError: its items have no fifth entry, so a trainer that passed CROP to it would silently get full
frames from ``collate``; the error names ``Crop_Dataset`` instead.

Limits.  The colour-jitter draws follow torchvision's published rules but are not pinned against torchvision.  Two sources come
from the device's own counter-based generator, not from torch's host generator: the pad noise
(``torch.rand`` in the reference) and, in the crop mode, the occluded region's values (``torch.normal`` in the reference).  A frame
one of whose boxes has unreadable corners is left out, as in the reference (EXCLUDE)."""
import os
import random
import _pickle as pickle

import numpy as np
import torch
from torch.utils import data

from retinanet_mi355x import augment

DEVICE = "cuda"              # where collate puts the batch
CLASSES = {"sedan": 0, "midsize": 1, "van": 2, "pickup": 3, "semi": 4, "truck (other)": 5, "truck": 5, "motorcycle": 6, "trailer": 7}


class _Frames(data.Dataset):
    """What both datasets share: the reference's parsing, shuffle and 90/10 split (:169-294) and undecorated items."""

    def __init__(self, dataset_dir, label_format, mode, CROP):
        self.mode, self.label_format, self.CROP = mode, label_format, CROP
        self.classes = dict(CLASSES)
        self.classes.update({v: k for k, v in CLASSES.items() if k != "truck"})
        with open("camera_vps.cpkl", "rb") as f:
            self.vps = pickle.load(f)
        with open(os.path.join(dataset_dir, "labels.cpkl"), "rb") as f:
            all_labels = pickle.load(f)
        random.shuffle(all_labels)
        self.data, self.labels = [], []
        for path, boxes in all_labels:
            rows, exclude = [], False
            if len(boxes) == 0:
                rows = [torch.zeros(21)]                                    # :238-239: one all-zero float32 row
            for box in boxes:
                cls = np.ones([1]) * self.classes[box[3]] if box[3] in self.classes else np.zeros([1])
                try:
                    bbox3d = np.array(box[11:27]).astype(float)
                except (ValueError, TypeError):
                    exclude = True
                    break
                try:
                    bbox2d = np.array(box[4:8]).astype(float)
                except (ValueError, TypeError):
                    bbox2d = np.array([np.min(bbox3d[::2]), np.min(bbox3d[1::2]), np.max(bbox3d[::2]), np.max(bbox3d[1::2])])
                rows.append(torch.from_numpy(np.concatenate((bbox3d, bbox2d, cls), axis=0).astype(float)))
            if not exclude:
                self.data.append(path)
                self.labels.append(torch.stack(rows))
        cut = int(len(self.data) * 0.9)
        if self.mode == "train":
            self.data, self.labels = self.data[:cut], self.labels[:cut]
        else:
            self.data, self.labels = self.data[cut:], self.labels[cut:]

    def __len__(self):
        return len(self.labels)

    def _item(self, index):
        path = self.data[index]
        if path.endswith(".npy"):                                           # frames cached as arrays are read as they are
            frame = np.load(path)
        else:
            from PIL import Image
            frame = np.array(Image.open(path).convert("RGB"))
        camera_id = path.split("/")[-1].split("_")[0]
        return frame, self.labels[index].clone(), camera_id, self.vps[camera_id]


class Detection_Dataset(_Frames):
    """Returns undecorated frames and 3D labels for 3D detector training; ``collate`` augments them on the device."""

    def __init__(self, dataset_dir, label_format="tailed_footprint", mode="train", CROP=0):
        if CROP != 0:
            raise NotImplementedError("Detection_Dataset: only the full-frame mode (CROP == 0); the crop mode (CROP > 0, "
                                      "corrected_3D_dataset.py:501-594) is Crop_Dataset")
        _Frames.__init__(self, dataset_dir, label_format, mode, CROP)

    def __getitem__(self, index):
        """-> (frame uint8 [H,W,3], labels [n,21], camera id, the camera's vanishing points)."""
        return self._item(index)


class Crop_Dataset(_Frames):
    """The same frames and labels for the crop detector's training (the reference's Detection_Dataset with CROP > 0)."""

    def __init__(self, dataset_dir, label_format="tailed_footprint", mode="train", CROP=112):
        if int(CROP) <= 0:
            raise ValueError("Crop_Dataset: CROP must be positive, got %r (CROP == 0 is Detection_Dataset)" % (CROP,))
        _Frames.__init__(self, dataset_dir, label_format, mode, int(CROP))

    def __getitem__(self, index):
        """-> (frame uint8 [H,W,3], labels [n,21], camera id, the camera's vanishing points, CROP)."""
        return self._item(index) + (self.CROP,)


_calls = [0]


def collate(inputs, noise=None, seed=None, occlusion=None):
    """Receives a list of ``__getitem__`` results; makes the draws, augments on the device and returns
    (im [B,3,H,W], label [B,N,27]) there, or (im [B,3,CROP,CROP], label [B,N,21]) for ``Crop_Dataset``'s five-entry items.
    noise / seed (/ occlusion): see ops.augment_frames (ops.augment_crops); by default every call takes a fresh seed derived
    from torch's initial seed."""
    if seed is None:
        seed = torch.initial_seed() + 1000003 * _calls[0]
        _calls[0] += 1
    if len(inputs[0]) == 5:
        frames, labels, cameras, vps, crops = zip(*inputs)
        if len(set(crops)) != 1:
            raise ValueError("collate: items of different CROP in one batch: %r" % (sorted(set(crops)),))
        return augment.augment_crop_batch(list(frames), list(labels), list(cameras), list(vps), crops[0], DEVICE, noise=noise,
                                          occlusion=occlusion, seed=seed)
    if occlusion is not None:
        raise ValueError("collate: occlusion values belong to the crop mode")
    frames, labels, cameras, vps = zip(*inputs)
    return augment.augment_batch(list(frames), list(labels), list(cameras), list(vps), DEVICE, noise=noise, seed=seed)

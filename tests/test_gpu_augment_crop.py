"""GPU: crop-detector training batches on the device (csrc/augment_crop.hip: rn_augment_crops; ops.augment_crops;
torch.ops.retinanet_mi355x.augment_crops; augment.augment_crop_batch / AugmentedBatches(crop=); the corrected_3D_dataset drop-in's
Crop_Dataset) against the numpy restatement in tests/augment_crop_cases.py and the reference's own results in
tests/golden/augment_crop.npz.

Everything but the device's own occlusion generator is compared for equality: the output is a function of bytes that are fixed
by integer, fp64 and single-rounded fp32 operations on both sides, so every output float must have the same bits.

Shapes.  The window stage takes one window pixel per lane in blocks of 256 over the flattened cw * ch pixels of an image's own
window, in a grid sized by the batch's largest window edge squared (image in blockIdx.y); the two resize stages do the same over
ch * crop and crop * crop.  A 300x5 and a 3x300 window are the two ways in which the lane -> (row, column) split can go wrong
(rows longer than a block; more rows than a block has lanes), a 1x1 window is the smallest, and one batch holds them all, so the
per-image windows, the shared grid and the shared table stride (the batch's largest tap count) all differ from every image's own."""
import numpy as np
import pytest
import torch

import augment_cases as ac
import augment_crop_cases as cc

pytestmark = pytest.mark.gpu

GROUPS = sorted({(c[1], c[5]) for c in cc.GOLDEN})


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(dev, frames, params, cs, noise=None, occlusion=None, seed=0, custom=False):
    from retinanet_mi355x import augment, ops, torch_ops  # noqa: F401  (torch_ops registers the operator)
    H, W = frames[0].shape[:2]
    f = torch.from_numpy(np.stack(frames)).to(dev)
    n = None if noise is None else torch.from_numpy(np.stack(noise)).to(dev)
    o = None if occlusion is None else torch.from_numpy(np.stack(occlusion)).to(dev)
    rec, tx, ty, cx, cy, K, win_max = augment.pack_crop_params(params, W, H, cs)
    if custom:
        rec = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), -1)).to(dev)
        tables = [torch.from_numpy(t).to(dev) for t in (tx, ty, cx, cy)]
        return torch.ops.retinanet_mi355x.augment_crops(f, rec, *tables, K, win_max, cs, n, o, seed).cpu().numpy()
    return ops.augment_crops(f, (rec, tx, ty, cx, cy), K, win_max, cs, noise=n, occlusion=o, seed=seed).cpu().numpy()


@pytest.fixture(scope="module")
def items(golden):
    g = golden("augment_crop")
    return {c[0]: cc.unpack_golden(g, c[0]) for c in cc.GOLDEN}


@pytest.mark.parametrize("shape,cs", GROUPS)
def test_golden_batches(dev, items, shape, cs):
    """The reference's own frames, draws, noise and occlusion values, one batch per (shape, crop) with mixed records."""
    names = [c[0] for c in cc.GOLDEN if (c[1], c[5]) == (shape, cs)]
    got = _run(dev, [items[n]["frame"] for n in names], [items[n]["params"] for n in names], cs,
               [items[n]["noise"] for n in names], [items[n]["occlusion"] for n in names])
    for i, n in enumerate(names):
        assert np.array_equal(_bits(got[i]), _bits(items[n]["im_t"])), n


W0, H0 = 70, 52                  # the hand-built records' frame


def _base(win, cs, **kw):
    from retinanet_mi355x import augment
    p = augment.identity_params(W0, H0)
    del p["dy"], p["dx"]
    p.update(angle=0.0, win=tuple(win), crop=cs, occlude=None)
    p.update(kw)
    if "angle" in kw:
        p["affine"] = ac.affine(kw["angle"], W0, H0)
    return p


def _hand_cases(cs):
    """Records built by hand: every window form, with rotation, flip, both resizes, pad noise, jitter and occlusion among them."""
    f32 = lambda *v: [float(np.float32(x)) for x in v]
    return [_base((-100, -20, 300, 5), cs, angle=7.5, rh=int(H0 * 0.8)),                          # 300x5: rows longer than a block
            _base((30, -120, 3, 300), cs, angle=-12.0, flip=1, rw=int(W0 * 1.2), rh=int(H0 * 1.2 * 1.3)),   # 3x300
            _base((33, 21, 1, 1), cs, angle=3.0),                                                 # 1x1
            _base((200, 10, 40, 41), cs, angle=20.0),                                             # wholly outside
            _base((-9, 10, 30, 29), cs, angle=-20.0, rw=int(W0 * 1.1), rh=int(H0 * 1.1)),         # crosses the left edge
            _base((15, -11, 31, 30), cs, angle=5.0, flip=1),                                      # ... the top edge
            _base((50, 12, 33, 33), cs, angle=-5.0, rh=int(H0 * 0.76), apply=1, order=[2, 1, 0, 3], factors=f32(0.7, 1.4, 0.6)),  # right
            _base((20, 30, 36, 37), cs, angle=11.0, rh=int(H0 * 0.9), apply=1, order=[1, 3, 0, 2], factors=f32(1.5, 0.5, 1.3),
                  occlude=(2, 9, cs - 3, cs)),                                                    # bottom, into the pad noise
            _base((10, 8, cs, cs), cs, angle=-3.3, apply=1, order=[0, 2, 3, 1], factors=f32(1.2, 0.8, 1.45)),   # both second passes skipped
            _base((12, 9, cs, 40), cs, angle=1.0), _base((12, 9, 40, cs), cs, angle=1.0, occlude=(0, cs // 3, cs - 1, cs)),  # one skipped
            _base((-15, -25, int(4.2 * cs), int(4.2 * cs) + 1), cs, angle=-8.0, flip=1, rw=int(W0 * 1.05), rh=int(H0 * 1.05 * 0.85))]  # 4.2x


@pytest.fixture(scope="module")
def hand_inputs():
    rng = np.random.RandomState(7)
    n = len(_hand_cases(24))
    frames = [ac.frame_bytes("crop%d" % i, W0, H0) for i in range(n)]
    noise = [rng.randint(0, 256, size=(H0, W0, 3)).astype(np.uint8) for _ in range(n)]
    return frames, noise


@pytest.mark.parametrize("cs", [24, 33])
def test_hand_cases_equal_the_restatement(dev, hand_inputs, cs):
    """One batch whose windows and tap counts all differ, through ops and through torch.ops."""
    from retinanet_mi355x import augment
    frames, noise = hand_inputs
    params = _hand_cases(cs)
    rng = np.random.RandomState(cs)
    occ = [rng.standard_normal((3, cs, cs)).astype(np.float32) for _ in params]
    assert len({augment.crop_taps(max(p["win"][2:]), cs) for p in params}) >= 4
    got = _run(dev, frames, params, cs, noise, occ)
    via_op = _run(dev, frames, params, cs, noise, occ, custom=True)
    for i, p in enumerate(params):
        want = cc.chain(frames[i], p, noise[i], occ[i])["out"]
        assert np.array_equal(_bits(got[i]), _bits(want)), (i, p)
    assert np.array_equal(_bits(got), _bits(via_op))


@pytest.mark.parametrize("i", [0, 1, 2, 3, 8])
def test_hand_cases_alone(dev, hand_inputs, i):
    """The same records in a batch of one: the grid and the table stride are then the image's own."""
    frames, noise = hand_inputs
    p = _hand_cases(24)[i]
    got = _run(dev, [frames[i]], [p], 24, [noise[i]])
    assert np.array_equal(_bits(got[0]), _bits(cc.chain(frames[i], p, noise[i])["out"]))


def test_dropin_end_to_end(dev, items, tmp_path, monkeypatch):
    """corrected_3D_dataset.Crop_Dataset + collate on the golden's frames, under the golden's seeds and with its noise and
    occlusion values, equal the reference's im_t and y."""
    import random
    import corrected_3D_dataset as dd
    rows_of = cc.write_dataset(tmp_path, {n: d["frame"] for n, d in items.items()})
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dd, "DEVICE", dev)
    seen = 0
    for mode in ("train", "test"):
        random.seed(0)
        ds = dd.Crop_Dataset(str(tmp_path), label_format="8_corners", mode=mode, CROP=24)
        for idx in range(len(ds)):
            d = items[rows_of[ds.data[idx]]]
            ds.CROP = int(d["cs"])
            if d["labels_in"].shape[0] == 0:
                ds.labels[idx] = torch.zeros([0, 21], dtype=torch.float64)
            H, W = d["frame"].shape[:2]
            np.random.seed(int(d["seed"]))
            torch.manual_seed(int(d["seed"]))
            torch.rand([3, H, W])                                          # the reference's noise image is torch's first draw
            im, label = dd.collate([ds[idx]], noise=torch.from_numpy(d["noise"][None]).to(dev),
                                   occlusion=torch.from_numpy(d["occlusion"][None]).to(dev))
            assert im.device.type == "cuda" and label.device.type == "cuda" and tuple(im.shape) == (1, 3, ds.CROP, ds.CROP)
            assert np.array_equal(_bits(im[0].cpu().numpy()), _bits(d["im_t"]))
            assert label.dtype == torch.float32 and np.array_equal(_bits(label[0].cpu().numpy()), _bits(d["y"].astype(np.float32)))
            seen += 1
    assert seen == len(cc.GOLDEN)


def test_device_occlusion_generator(dev):
    """mean + std z from the device's generator on a hand-set 64x64 region: 4096 samples per channel."""
    cs = 96
    region = (20, 30, 84, 94)
    frames = [ac.frame_bytes("occl%d" % i, W0, H0) for i in range(2)]
    noise = [np.zeros((H0, W0, 3), np.uint8)] * 2
    params = [_base((5, 4, 50, 44), cs, angle=4.0, occlude=region)] * 2
    plain = _run(dev, frames, [dict(p, occlude=None) for p in params], cs, noise, seed=11)
    a = _run(dev, frames, params, cs, noise, seed=11)
    assert np.array_equal(_bits(a), _bits(_run(dev, frames, params, cs, noise, seed=11)))        # repeats for a seed
    b = _run(dev, frames, params, cs, noise, seed=12)
    x0, y0, x1, y1 = region
    inside = np.zeros((cs, cs), bool)
    inside[y0:y1, x0:x1] = True
    for got in (a, b):                                                                          # nothing outside the region
        assert np.array_equal(_bits(got[:, :, ~inside]), _bits(plain[:, :, ~inside]))
    va, vb = a[:, :, inside], b[:, :, inside]                                                   # [2, 3, 4096]
    assert not np.array_equal(va, vb) and not np.array_equal(va[0], va[1])                      # differs between seeds and images
    assert np.isfinite(va).all()
    for img in range(2):
        for c in range(3):
            v = va[img, c].astype(np.float64)
            assert v.size == 4096
            assert abs(v.mean() - float(ac.MEAN[c])) <= 5 * float(ac.STD[c]) / np.sqrt(4096), (img, c, v.mean())
            assert abs(v.std(ddof=1) - float(ac.STD[c])) <= 0.1 * float(ac.STD[c]), (img, c, v.std(ddof=1))


def test_ops_refuse_bad_arguments(dev):
    from retinanet_mi355x import augment, ops
    cs = 24
    f = torch.zeros((1, H0, W0, 3), dtype=torch.uint8, device=dev)
    rec, tx, ty, cx, cy, K, win_max = augment.pack_crop_params([_base((-15, -25, 100, 101), cs)], W0, H0, cs)
    good = (rec, tx, ty, cx, cy)
    assert K > 7 and tuple(ops.augment_crops(f, good, K, win_max, cs).shape) == (1, 3, cs, cs)
    for frames, params, k, kw in ((f.float(), good, K, {}), (f.cpu(), good, K, {}),
                                  (f, (rec, tx, ty, cx[:, :, :-2], cy[:, :, :-2]), K, {}),      # a table too narrow for K
                                  (f, (rec, tx, ty, cx, cy[:, :-1]), K, {}), (f, (rec, tx[:, :, :-1], ty, cx, cy), K, {}),
                                  (f, good, K + 2, {}),
                                  (f, good, K, dict(occlusion=torch.zeros((1, 3, cs, cs + 1), device=dev))),
                                  (f, good, K, dict(occlusion=torch.zeros((1, 3, cs, cs), dtype=torch.float64, device=dev))),
                                  (f, good, K, dict(occlusion=torch.zeros((1, 3, cs, cs)))),
                                  (f, good, K, dict(noise=torch.zeros((1, H0, W0, 1), dtype=torch.uint8, device=dev)))):
        with pytest.raises(RuntimeError):
            ops.augment_crops(frames, params, k, win_max, cs, **kw)
    with pytest.raises(RuntimeError):
        ops.augment_crops(f, good, K, 0, cs)


def test_augmented_batches_crop(dev, items):
    """AugmentedBatches(..., crop=24) as trainer.train's ``batches``: device tensors of the crop's shape, repeatable."""
    from retinanet_mi355x import augment
    names = [c[0] for c in cc.GOLDEN if c[1] == "q"][:6]
    frames = np.stack([items[n]["frame"] for n in names])
    labels = [torch.from_numpy(items[n]["labels_in"]) for n in names]
    cameras = [str(items[n]["camera"]) for n in names]

    def run():
        np.random.seed(3)
        torch.manual_seed(3)
        return list(augment.AugmentedBatches(frames, labels, cameras, ac.VPS, 3, dev, seed=5, crop=24)(0))
    got = run()
    assert len(got) == 2
    for im, label in got:
        assert im.device.type == "cuda" and im.dtype == torch.float32 and tuple(im.shape) == (3, 3, 24, 24)
        assert label.device.type == "cuda" and label.dtype == torch.float32 and label.shape[0] == 3 and label.shape[2] == 21
        assert bool(torch.isfinite(im).all())
    for (a, la), (b, lb) in zip(got, run()):
        assert torch.equal(a, b) and torch.equal(la, lb)

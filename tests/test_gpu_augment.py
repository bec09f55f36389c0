"""GPU: training-batch augmentation on the device (csrc/augment.hip: rn_augment_frames; ops.augment_frames;
torch.ops.retinanet_mi355x.augment_frames; augment.AugmentedBatches; the corrected_3D_dataset drop-in) against the numpy
restatement in tests/augment_cases.py and the reference's own results in tests/golden/augment.npz.

Everything is compared for equality: the output is a function of bytes that are fixed by integer, fp64 and single-rounded fp32
operations on both sides, so every output float must have the same bits.

Shapes.  The kernels take one pixel per lane in blocks of 256 lanes over the flattened H*W pixels of an image (image in
blockIdx.y); there is no two-dimensional tile.  50x38 and 41x27 are odd sizes whose widths are no multiple of 4 and that take
several blocks with a partial last one; 96x64 runs as a batch of 3 with mixed records.  CROSS_W = 300x5 has rows longer than
a block (a block lies inside one row, the row index changes inside a block only once) and CROSS_H = 3x300 has 85 rows per
block and more rows than a block has lanes: the two ways in which the pixel -> (row, column) split can go wrong."""
import numpy as np
import pytest
import torch

import augment_cases as ac

pytestmark = pytest.mark.gpu

CROSS_W, CROSS_H = (300, 5), (3, 300)
SHAPES = [(50, 38), (41, 27), CROSS_W, CROSS_H]
ORDERS = [[0, 1, 2, 3], [2, 1, 0, 3], [1, 3, 0, 2], [3, 2, 0, 1], [1, 0, 3, 2], [2, 3, 1, 0]]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(dev, frames, params, noise=None, seed=0, custom=False):
    from retinanet_mi355x import augment, ops, torch_ops  # noqa: F401  (torch_ops registers the operator)
    H, W = frames[0].shape[:2]
    f = torch.from_numpy(np.stack(frames)).to(dev)
    n = None if noise is None else torch.from_numpy(np.stack(noise)).to(dev)
    rec, tx, ty = augment.pack_params(params, W, H)
    if custom:
        rec = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), -1)).to(dev)
        return torch.ops.retinanet_mi355x.augment_frames(f, rec, torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev), n, seed).cpu().numpy()
    return ops.augment_frames(f, (rec, tx, ty), noise=n, seed=seed).cpu().numpy()


def _hand_cases(W, H):
    """Records built by hand: rotation both ways, shrinking and stretching, every roll form, several op orders."""
    from retinanet_mi355x import augment
    base = augment.identity_params(W, H)
    out = [dict(base, affine=ac.affine(20.0, W, H)), dict(base, affine=ac.affine(-20.0, W, H), flip=1),
           dict(base, rh=int(H * 0.75)), dict(base, rh=int(H * 1.13 * 1.4), rw=int(W * 1.13)),
           dict(base, rh=int(H * 1.07 * 0.93), rw=int(W * 1.07), flip=1, affine=ac.affine(3.7, W, H)),
           dict(base, dx=W // 3), dict(base, dy=H // 2, dx=W - 1), dict(base, dy=H - 1), dict(base, flip=1, dx=1)]
    for i, order in enumerate(ORDERS):
        out.append(dict(base, apply=1, order=order, factors=[float(np.float32(v)) for v in (0.4 + 0.2 * i, 1.6 - 0.21 * i, 0.5 + 0.19 * i)],
                        affine=ac.affine(-11.3 + 4 * i, W, H), rh=int(H * (0.8 + 0.1 * i)), dy=i % H, dx=(7 * i) % W, flip=i & 1))
    return out


@pytest.fixture(scope="module")
def items(golden):
    g = golden("augment")
    return {c[0]: ac.unpack_golden(g, c[0]) for c in ac.GOLDEN}


@pytest.mark.parametrize("shape", sorted(ac.SHAPES))
def test_golden_batches(dev, items, shape):
    """The reference's own frames, draws and noise, one batch per shape (96x64: a batch of 3 with mixed records)."""
    names = [c[0] for c in ac.GOLDEN if c[1] == shape]
    got = _run(dev, [items[n]["frame"] for n in names], [items[n]["params"] for n in names], [items[n]["noise"] for n in names])
    for i, n in enumerate(names):
        assert np.array_equal(_bits(got[i]), _bits(items[n]["im_t"])), n


@pytest.mark.parametrize("W,H", SHAPES)
def test_hand_cases_equal_the_restatement(dev, W, H):
    params = _hand_cases(W, H)
    rng = np.random.RandomState(W * 1000 + H)
    frames = [ac.frame_bytes("hand%d" % i, W, H) for i in range(len(params))]
    noise = [rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in params]
    got = _run(dev, frames, params, noise)
    via_op = _run(dev, frames, params, noise, custom=True)
    for i, p in enumerate(params):
        want = ac.chain(frames[i], p, noise[i])["out"]
        assert np.array_equal(_bits(got[i]), _bits(want)), (i, p)
    assert np.array_equal(_bits(got), _bits(via_op))


@pytest.mark.parametrize("W,H", SHAPES)
def test_identity_equals_frame_ingest(dev, W, H):
    from retinanet_mi355x import augment, ops
    frames = [ac.frame_bytes("id%d" % i, W, H) for i in range(2)]
    got = _run(dev, frames, [augment.identity_params(W, H)] * 2)
    want = ops.frame_ingest(torch.from_numpy(np.stack(frames)).to(dev)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))


def _bytes_of(out):
    """The byte behind every output float (the finish stage is injective on bytes)."""
    table = ((np.arange(256, dtype=np.float32) / np.float32(255.0))[:, None] - ac.MEAN) / ac.STD          # [256,3]
    b = np.zeros(out.shape, np.int64)
    for c in range(3):
        idx = np.searchsorted(table[:, c], out[:, c])
        assert np.array_equal(table[idx.clip(0, 255), c], out[:, c])
        b[:, c] = idx
    assert b.min() >= 0 and b.max() <= 255
    return b.transpose(0, 2, 3, 1).astype(np.uint8)


def test_device_noise_generator(dev):
    from retinanet_mi355x import augment
    W, H = 41, 27
    base = augment.identity_params(W, H)
    params = [dict(base, rh=int(H * 0.75)), dict(base, rh=int(H * 0.75)), dict(base, rh=H - 1, rw=W + 5)]
    frames = [ac.frame_bytes("noise", W, H)] * 3
    a = _run(dev, frames, params, seed=11)
    assert np.array_equal(_bits(a), _bits(_run(dev, frames, params, seed=11)))                   # repeats for a seed
    b = _run(dev, frames, params, seed=12)
    ba, bb = _bytes_of(a), _bytes_of(b)                                                         # bytes, so in [0, 255]
    want_noise = augment.noise_bytes(11, 3, H, W)
    for i, p in enumerate(params):
        rows = min(p["rh"], H)
        inside = ac.resize(frames[i], p["rh"], p["rw"])[:rows, :W]
        assert np.array_equal(ba[i, :rows], inside) and np.array_equal(bb[i, :rows], inside)     # noise touches the pad only
        assert np.array_equal(ba[i, rows:], want_noise[i, rows:])                                # ... and is the stated generator
        assert not np.array_equal(ba[i, rows:], bb[i, rows:])                                    # differs between seeds
    assert not np.array_equal(ba[0, int(H * 0.75):], ba[1, int(H * 0.75):])                      # and between images
    # before the rotation: a rotated record moves the same bytes
    rot = [dict(p, affine=ac.affine(20.0, W, H)) for p in params]
    got = _run(dev, frames, rot, seed=11)
    for i, p in enumerate(rot):
        assert np.array_equal(_bits(got[i]), _bits(ac.chain(frames[i], p, want_noise[i])["out"]))


def test_ops_refuse_bad_arguments(dev):
    from retinanet_mi355x import augment, ops
    W, H = 41, 27
    f = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev)
    rec, tx, ty = augment.pack_params([augment.identity_params(W, H)], W, H)
    with pytest.raises(RuntimeError):
        ops.augment_frames(f.float(), (rec, tx, ty))
    with pytest.raises(RuntimeError):
        ops.augment_frames(f, (rec, tx[:, :-1], ty))
    with pytest.raises(RuntimeError):
        ops.augment_frames(f, (rec, tx, ty), noise=torch.zeros((1, H, W, 1), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError):
        ops.augment_frames(f.cpu(), (rec, tx, ty))


def test_dropin_end_to_end(dev, items, tmp_path, monkeypatch):
    """corrected_3D_dataset.Detection_Dataset + collate on the golden's frames, under the golden's seeds and with its noise,
    equal the reference's im_t and y."""
    import random
    import corrected_3D_dataset as dd
    rows_of = ac.write_dataset(tmp_path, {n: d["frame"] for n, d in items.items()})
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dd, "DEVICE", dev)
    with pytest.raises(NotImplementedError):
        dd.Detection_Dataset(str(tmp_path), CROP=112)
    seen = 0
    for mode in ("train", "test"):
        random.seed(0)
        ds = dd.Detection_Dataset(str(tmp_path), mode=mode, CROP=0)
        for idx in range(len(ds)):
            d = items[rows_of[ds.data[idx]]]
            if d["labels_in"].shape[0] == 0:
                ds.labels[idx] = torch.zeros([0, 21], dtype=torch.float64)
            assert np.array_equal(ds.labels[idx].numpy(), d["labels_in"]) and ds.labels[idx].numpy().dtype == d["labels_in"].dtype
            H, W = d["frame"].shape[:2]
            np.random.seed(int(d["seed"]))
            torch.manual_seed(int(d["seed"]))
            torch.rand([3, H, W])                                          # the reference's noise image is torch's first draw
            im, label = dd.collate([ds[idx]], noise=torch.from_numpy(d["noise"][None]).to(dev))
            assert im.device.type == "cuda" and label.device.type == "cuda"
            assert np.array_equal(_bits(im[0].cpu().numpy()), _bits(d["im_t"]))
            assert np.array_equal(_bits(label[0].cpu().numpy()), _bits(d["y"]))
            seen += 1
    assert seen == len(ac.GOLDEN)


def test_augmented_batches(dev, items):
    """AugmentedBatches as trainer.train's ``batches``: device tensors, labels padded with -1 rows, frames of unequal label counts."""
    from retinanet_mi355x import augment
    names = [c[0] for c in ac.GOLDEN if c[1] == "a"]
    frames = np.stack([items[n]["frame"] for n in names])
    labels = [torch.from_numpy(items[n]["labels_in"]) for n in names]
    cameras = [str(items[n]["camera"]) for n in names]
    np.random.seed(3)
    torch.manual_seed(3)
    batches = augment.AugmentedBatches(frames, labels, cameras, ac.VPS, 2, dev, seed=5)
    got = list(batches(0))
    assert len(got) == len(batches) == len(names) // 2
    for im, label in got:
        assert im.device.type == "cuda" and im.dtype == torch.float32 and tuple(im.shape) == (2, 3) + frames.shape[1:3]
        assert label.dtype == torch.float32 and label.shape[0] == 2 and label.shape[2] == 27
        assert bool(torch.isfinite(im).all())
    # the same seeds give the same batches
    np.random.seed(3)
    torch.manual_seed(3)
    again = list(augment.AugmentedBatches(frames, labels, cameras, ac.VPS, 2, dev, seed=5)(0))
    for (a, la), (b, lb) in zip(got, again):
        assert torch.equal(a, b) and torch.equal(la, lb)

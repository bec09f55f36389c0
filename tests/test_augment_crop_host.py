"""Host side of the crop mode of the training-batch augmentation: tests/augment_crop_cases.py (the numpy restatement of the
reference's crop branch) against tests/golden/augment_crop.npz -- the reference's own __getitem__ with CROP > 0 and collate --
and, where Pillow imports, against Pillow; retinanet_mi355x.augment (draw_crop, pack_crop_params, the general-tap table) and the
drop-in's Crop_Dataset against the same golden.  Everything is compared for equality: bytes, fp32 bits, labels from the same fp64
torch operations.  The GPU tests compare the kernels with the restatement, so this file is what ties them to the reference."""
import numpy as np
import pytest
import torch

import augment_cases as ac
import augment_crop_cases as cc
from retinanet_mi355x import augment

NAMES = [c[0] for c in cc.GOLDEN]
GROUPS = sorted({(c[1], c[5]) for c in cc.GOLDEN})


@pytest.fixture(scope="module")
def items(golden):
    g = golden("augment_crop")
    return {n: cc.unpack_golden(g, n) for n in NAMES}


def _seeded(d):
    """The golden's seeds; the reference's noise image is torch's first draw."""
    H, W = d["frame"].shape[:2]
    np.random.seed(int(d["seed"]))
    torch.manual_seed(int(d["seed"]))
    return torch.rand([3, H, W]), (W, H)


@pytest.fixture(scope="module")
def rotated_labels(items):
    """The labels as they leave the common part (pinned by tests/test_augment_host.py), under the golden's seeds."""
    out = {}
    for n, d in items.items():
        _, size = _seeded(d)
        out[n] = augment._draw_common(torch.from_numpy(d["labels_in"]), str(d["camera"]), d["vps"].tolist(), size)[1].numpy()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(items, rotated_labels, name):
    d = items[name]
    r = cc.chain(d["frame"], d["params"], d["noise"], d["occlusion"])
    assert np.array_equal(r["window"], d["window"])
    assert np.array_equal(r["second"], d["second"])
    assert len(r["jitter_steps"]) == len(d["jitter_steps"]) == (4 if d["params"]["apply"] else 0)
    for got, want in zip(r["jitter_steps"], d["jitter_steps"]):
        assert np.array_equal(got, want)
    assert r["out"].dtype == np.float32 and np.array_equal(r["out"].view(np.uint32), d["im_t"].view(np.uint32))
    assert cc.window_from(d["center"], float(d["size"])) == d["params"]["win"]
    y = cc.labels(rotated_labels[name], d["win"], int(d["cs"]))
    assert y.dtype == d["y"].dtype and y.shape == d["y"].shape and np.array_equal(y, d["y"])


@pytest.mark.parametrize("mutation", sorted(cc.MUTATIONS))
def test_mutation_is_caught(items, rotated_labels, mutation):
    caught = [n for n, d in items.items() if cc.mutation_caught(d, rotated_labels[n], mutation)]
    assert caught, cc.MUTATIONS[mutation]


class _Recorded:
    """np.random.normal / rand / randint wrapped: the values they return, in order (an array's values one by one)."""
    def __enter__(self):
        self.values = []
        self.saved = (np.random.normal, np.random.rand, np.random.randint)

        def wrap(fn):
            def inner(*a, **k):
                v = fn(*a, **k)
                self.values.extend(float(x) for x in np.atleast_1d(v))
                return v
            return inner
        np.random.normal, np.random.rand, np.random.randint = (wrap(f) for f in self.saved)
        return self

    def __exit__(self, *exc):
        np.random.normal, np.random.rand, np.random.randint = self.saved


@pytest.mark.parametrize("name", NAMES)
def test_draw_crop_reproduces_draws_window_and_labels(items, name):
    d = items[name]
    noise, size = _seeded(d)
    with _Recorded() as rec:
        p, y = augment.draw_crop(torch.from_numpy(d["labels_in"]), str(d["camera"]), d["vps"].tolist(), size, int(d["cs"]))
    assert rec.values == d["np_draws"].tolist()                              # the same numpy draws in the same order
    assert np.array_equal(ac.noise_bytes(noise.numpy().transpose(1, 2, 0)), d["noise"])
    want = d["params"]
    for k in ("rh", "rw", "flip", "apply", "order", "affine", "win", "crop", "occlude"):
        assert p[k] == want[k], k
    assert "dy" not in p and "dx" not in p
    if want["apply"]:
        assert p["factors"] == want["factors"]
    assert [p["scale"], p["aspect"], p["angle"], p["occlude_draw"]] == d["scalars"].tolist()
    assert y.numpy().dtype == d["y"].dtype and tuple(y.shape) == d["y"].shape and y.shape[1] == 21
    assert np.array_equal(y.numpy(), d["y"])


def test_draw_is_unmoved_by_the_shared_part(golden):
    """``draw`` and ``draw_crop`` consume the same draws up to the rotation."""
    g = golden("augment")
    d = ac.unpack_golden(g, "a0")
    H, W = d["frame"].shape[:2]
    args = (torch.from_numpy(d["labels_in"]), str(d["camera"]), d["vps"].tolist(), (W, H))
    np.random.seed(5)
    p, _ = augment.draw(*args)
    np.random.seed(5)
    q, _ = augment.draw_crop(*args, 24)
    for k in ("rh", "rw", "flip", "angle", "affine", "scale", "aspect"):
        assert p[k] == q[k]


def test_golden_set_covers_what_it_must(items):
    def feature(fn):
        return any(fn(d, *[int(v) for v in d["win"]], d["frame"].shape[1], d["frame"].shape[0]) for d in items.values())
    assert {d["params"]["flip"] for d in items.values()} == {0, 1}
    assert feature(lambda d, x, y, w, h, W, H: x >= 0 and y >= 0 and x + w <= W and y + h <= H)          # inside
    assert feature(lambda d, x, y, w, h, W, H: x < 0 < x + w) and feature(lambda d, x, y, w, h, W, H: y < 0 < y + h)
    assert feature(lambda d, x, y, w, h, W, H: x < W < x + w) and feature(lambda d, x, y, w, h, W, H: y < H < y + h)
    assert feature(lambda d, x, y, w, h, W, H: x >= W or y >= H or x + w <= 0 or y + h <= 0)           # wholly outside
    assert feature(lambda d, x, y, w, h, W, H: w != h)
    assert feature(lambda d, x, y, w, h, W, H: max(w, h) > 3 * int(d["cs"]) and d["window"].any())
    assert feature(lambda d, x, y, w, h, W, H: max(w, h) < int(d["cs"]))
    assert feature(lambda d, x, y, w, h, W, H: d["params"]["occlude"] is not None)
    assert feature(lambda d, x, y, w, h, W, H: d["params"]["occlude"] is None)
    assert feature(lambda d, x, y, w, h, W, H: d["params"]["apply"]) and feature(lambda d, x, y, w, h, W, H: not d["params"]["apply"])
    assert {d["y"].dtype for d in items.values()} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any(str(d["camera"]) == "p2c3" for d in items.values())
    assert any(d["labels_in"].shape[0] == 0 and d["params"]["flip"] for d in items.values())
    assert any(d["labels_in"].shape[0] == 0 and not d["params"]["flip"] for d in items.values())


@pytest.mark.parametrize("shape,cs", GROUPS)
def test_collate_pads_exactly(golden, items, shape, cs):
    names = [c[0] for c in cc.GOLDEN if (c[1], c[5]) == (shape, cs)]
    ims, ys = augment.collate([(torch.from_numpy(items[n]["im_t"]), torch.from_numpy(items[n]["y"])) for n in names])
    want = golden("augment_crop")["collate_%s%d_y" % (shape, cs)]
    assert ys.dtype == torch.float32 and tuple(ys.shape[1:]) == want.shape[1:] and ys.shape[2] == 21
    assert np.array_equal(ys.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ims.numpy(), np.stack([items[n]["im_t"] for n in names]))


@pytest.mark.parametrize("n_in,n_out", [(50, 50), (38, 50), (50, 38), (1920, 2100), (1080, 811), (100, 34)])
def test_general_tap_table_equals_resample_table_at_7_taps(n_in, n_out):
    n = min(n_in, n_out)
    assert np.array_equal(augment.resample_table_taps(n_in, n_out, n, augment.TAPS), augment.resample_table(n_in, n_out, n))


@pytest.mark.parametrize("n_in,n_out", [(369, 32), (300, 24), (101, 24), (24, 24), (5, 24), (1, 24), (49, 112), (113, 112)])
def test_general_tap_table_equals_the_restatement(n_in, n_out):
    K = augment.crop_taps(n_in, n_out)
    xmin, k = ac.resample_coeffs(n_in, n_out)
    assert k.shape[1] == K
    for taps in (K, K + 4):                                                  # a wider stride: zero beyond a row's own
        t = augment.resample_table_taps(n_in, n_out, n_out, taps)
        assert t.dtype == np.int32 and np.array_equal(t[:, 0], xmin) and np.array_equal(t[:, 1:1 + K], k) and (t[:, 1 + K:] == 0).all()
    if K > 3:
        with pytest.raises(ValueError):
            augment.resample_table_taps(n_in, n_out, n_out, K - 2)


def test_pack_crop_params_round_trips(items):
    names = [c[0] for c in cc.GOLDEN if (c[1], c[5]) == ("q", 24)]
    W, H = cc.SHAPES["q"]
    ps = [items[n]["params"] for n in names]
    rec, tx, ty, cx, cy, K, win_max = augment.pack_crop_params(ps, W, H, 24)
    assert rec.dtype.itemsize == 128 and len(rec) == len(ps)
    assert K == max(augment.crop_taps(max(p["win"][2:]), 24) for p in ps) and win_max == max(max(p["win"][2:]) for p in ps)
    assert K > augment.TAPS and cx.shape == cy.shape == (len(ps), 24, 1 + K) and cx.dtype == cy.dtype == np.int32
    full, fx, fy = augment.pack_params([dict(p, dy=0, dx=0) for p in ps], W, H)
    assert np.array_equal(tx, fx) and np.array_equal(ty, fy)                # the first resize's tables as today
    for i, p in enumerate(ps):
        for k in ("affine", "rh", "rw", "flip", "apply", "order", "factors"):
            assert np.array_equal(rec[k][i], full[k][i]), k
        assert tuple(rec["win"][i]) == p["win"]
        assert bool(rec["occluded"][i]) == (p["occlude"] is not None)
        assert tuple(rec["occlude"][i]) == (p["occlude"] or (0, 0, 0, 0))
        for table, size in ((cx[i], p["win"][2]), (cy[i], p["win"][3])):
            xmin, k = ac.resample_coeffs(size, 24)
            assert np.array_equal(table[:, 0], xmin) and np.array_equal(table[:, 1:1 + k.shape[1]], k)
            assert (table[:, 1 + k.shape[1]:] == 0).all()


def test_pack_crop_params_refuses_bad_records(items):
    p = items["q0"]["params"]
    W, H = cc.SHAPES["q"]
    for bad in (dict(p, win=(0, 0, 0, 50)), dict(p, win=(0, 0, 50, -1)), dict(p, win=(0, 0, 50, 1 << 20)), dict(p, win=(1 << 31, 0, 50, 50)),
                dict(p, occlude=(0, 8, 25, 24)), dict(p, occlude=(5, 8, 4, 24)), dict(p, occlude=(-1, 8, 20, 24)),
                dict(p, order=[0, 1, 1, 3]), dict(p, rh=0), dict(p, rh=9), dict(p, crop=32)):
        with pytest.raises(ValueError):
            augment.pack_crop_params([bad], W, H, 24)
    with pytest.raises(ValueError):
        augment.pack_crop_params([p], W, H, 0)


def test_crop_dataset_parses_as_detection_dataset(items, tmp_path, monkeypatch):
    """corrected_3D_dataset.Crop_Dataset: the same parsing, shuffle and split; five-entry items; CROP <= 0 refused."""
    import random
    import corrected_3D_dataset as dd
    names = cc.write_dataset(tmp_path, {n: d["frame"] for n, d in items.items()})
    monkeypatch.chdir(tmp_path)
    for bad in (0, -5):
        with pytest.raises(ValueError):
            dd.Crop_Dataset(str(tmp_path), CROP=bad)
    with pytest.raises(NotImplementedError, match="Crop_Dataset"):
        dd.Detection_Dataset(str(tmp_path), CROP=112)
    for mode in ("train", "test"):
        random.seed(0)
        full = dd.Detection_Dataset(str(tmp_path), mode=mode)
        random.seed(0)
        ds = dd.Crop_Dataset(str(tmp_path), label_format="8_corners", mode=mode, CROP=24)
        assert ds.data == full.data and len(ds) == len(full)
        for idx in range(len(ds)):
            item, want = ds[idx], full[idx]
            d = items[names[ds.data[idx]]]
            assert len(item) == 5 and item[4] == 24
            assert np.array_equal(item[0], d["frame"]) and item[2] == str(d["camera"]) and item[3] == want[3]
            assert torch.equal(item[1], want[1])
            if d["labels_in"].shape[0]:
                assert item[1].numpy().dtype == d["labels_in"].dtype and np.array_equal(item[1].numpy(), d["labels_in"])


WINDOWS = [(-7, -5, 30, 31), (10, 8, 12, 12), (30, 20, 60, 40), (-100, -100, 20, 20), (-20, -20, 300, 290), (45, 3, 1, 1)]


@pytest.mark.parametrize("W,H", [(50, 38), (96, 64)])
def test_restatement_against_pillow(W, H):
    Image = pytest.importorskip("PIL.Image")
    f = ac.frame_bytes("pillowcrop%d" % W, W, H)
    im = Image.fromarray(f)
    rng = np.random.RandomState(W)
    wins = WINDOWS + [(int(rng.randint(-40, W)), int(rng.randint(-40, H)), int(rng.randint(1, 300)), int(rng.randint(1, 300)))
                      for _ in range(10)]
    for x, y, w, h in wins:
        cut = im.crop((x, y, x + w, y + h))
        got = cc.window(f, (x, y, w, h))
        assert np.array_equal(np.array(cut), got), (x, y, w, h)
        for cs in (24, 32):                                                  # shrink factors up to 12x, enlargements too
            assert np.array_equal(np.array(cut.resize((cs, cs), Image.BILINEAR)), ac.resize(got, cs, cs)), (x, y, w, h, cs)

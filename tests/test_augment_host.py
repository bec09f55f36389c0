"""Host side of the training-batch augmentation: tests/augment_cases.py (the numpy restatement of the reference's image chain)
against tests/golden/augment.npz -- the reference's own __getitem__ and collate -- and, where Pillow imports, against Pillow;
retinanet_mi355x.augment (draws, labels, parameter records, coefficient tables) against the same golden.  Everything is compared
for equality: bytes, fp32 bits, and labels that come from the same fp64 torch operations.  The GPU tests compare the kernels
with the restatement, so this file is what ties them to the reference."""
import numpy as np
import pytest
import torch

import augment_cases as ac
from retinanet_mi355x import augment

NAMES = [c[0] for c in ac.GOLDEN]


@pytest.fixture(scope="module")
def items(golden):
    g = golden("augment")
    return {n: ac.unpack_golden(g, n) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(items, name):
    d = items[name]
    r = ac.chain(d["frame"], d["params"], d["noise"])
    assert np.array_equal(r["resized"], d["resized"])
    assert np.array_equal(r["padded"], d["padded"])
    assert np.array_equal(r["rotated"], d["rotated"])
    assert len(r["jitter_steps"]) == len(d["jitter_steps"]) == (4 if d["params"]["apply"] else 0)
    for got, want in zip(r["jitter_steps"], d["jitter_steps"]):
        assert np.array_equal(got, want)
    assert r["out"].dtype == np.float32 and np.array_equal(r["out"].view(np.uint32), d["im_t"].view(np.uint32))


class _Recorded:
    """np.random.normal / rand / randint wrapped: the values they return, in order."""
    def __init__(self, script=None):
        self.values, self.script = [], script

    def __enter__(self):
        self.saved = (np.random.normal, np.random.rand, np.random.randint)

        def wrap(fn, scripted):
            def inner(*a, **k):
                v = self.script.pop(0) if scripted and self.script is not None else fn(*a, **k)
                self.values.append(float(v))
                return v
            return inner
        np.random.normal, np.random.rand, np.random.randint = wrap(self.saved[0], False), wrap(self.saved[1], False), wrap(self.saved[2], True)
        return self

    def __exit__(self, *exc):
        np.random.normal, np.random.rand, np.random.randint = self.saved


def _drawn(d):
    """augment.draw under the golden's seeds; the reference's noise image is torch's first draw, so it is drawn here too."""
    H, W = d["frame"].shape[:2]
    seed = int(d["seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    noise = torch.rand([3, H, W])
    with _Recorded() as rec:
        p, y = augment.draw(torch.from_numpy(d["labels_in"]), str(d["camera"]), d["vps"].tolist(), (W, H))
    return p, y, noise, rec.values


@pytest.mark.parametrize("name", NAMES)
def test_draw_reproduces_draws_and_labels(items, name):
    d = items[name]
    p, y, noise, values = _drawn(d)
    assert values == d["np_draws"].tolist()                                  # the same numpy draws in the same order
    assert np.array_equal(ac.noise_bytes(noise.numpy().transpose(1, 2, 0)), d["noise"])
    want = d["params"]
    for k in ("rh", "rw", "flip", "apply", "order", "dy", "dx", "affine"):
        assert p[k] == want[k], k
    if want["apply"]:
        assert p["factors"] == want["factors"]
    assert [p["scale"], p["aspect"], p["angle"], p["tile"]] == d["scalars"].tolist()
    assert y.dtype == torch.float32 and tuple(y.shape) == d["y"].shape
    assert np.array_equal(y.numpy().view(np.uint32), d["y"].view(np.uint32))


def test_golden_set_covers_what_it_must(items):
    flips = {d["params"]["flip"] for d in items.values()}
    tiles = {min(int(d["scalars"][3] * 4), 3) for d in items.values()}
    orders = {tuple(d["params"]["order"]) for d in items.values() if d["params"]["apply"]}
    assert flips == {0, 1} and tiles == {0, 1, 2, 3} and len(orders) >= 3
    assert any(not d["params"]["apply"] for d in items.values())
    assert any(d["scalars"][0] == 1 for d in items.values())
    assert any(d["scalars"][1] < 1 for d in items.values()) and any(d["scalars"][1] > 1 for d in items.values())
    assert any(d["labels_in"].shape[0] == 0 and d["params"]["flip"] for d in items.values())
    assert any(d["labels_in"].shape[0] == 0 and not d["params"]["flip"] for d in items.values())
    assert (items["a4"]["y"][:, 20] == -1).all() and (items["b3"]["y"][:, 20] == -1).all()      # rotated out of the image
    assert str(items["a1"]["camera"]) == "p2c3"


@pytest.mark.parametrize("shape", sorted(ac.SHAPES))
def test_collate_pads_exactly(golden, items, shape):
    names = [c[0] for c in ac.GOLDEN if c[1] == shape]
    ims, ys = augment.collate([(torch.from_numpy(items[n]["im_t"]), torch.from_numpy(items[n]["y"])) for n in names])
    want = golden("augment")["collate_%s_y" % shape]
    assert len({len(items[n]["y"]) for n in names}) > 1
    assert np.array_equal(ys.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ims.numpy(), np.stack([items[n]["im_t"] for n in names]))
    for i, n in enumerate(names):
        assert (ys[i, len(items[n]["y"]):] == -1).all()


# the split loop's exit rule (:440-464): (occupied, scripted draws, split kept, draws consumed)
SPLIT_CASES = {
    "first_is_good": ([(2.0, 8.0)], [9], 9, 1),
    "third_is_good": ([(2.0, 8.0)], [3, 7, 1], 1, 3),
    "edges_are_outside": ([(2.0, 8.0)], [2], 2, 1),                 # strict comparisons on both sides
    "upper_edge": ([(2.0, 8.0)], [8], 8, 1),
    "no_boxes": ([], [4], 4, 1),
    "ten_failures_keep_the_last": ([(0.5, 30.0)], [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13], 12, 10),
    "tenth_is_good": ([(0.5, 30.0)], [3, 4, 5, 6, 7, 8, 9, 10, 11, 0, 13], 0, 10),
    "second_box_blocks": ([(0.0, 1.0), (4.0, 9.0)], [5, 3], 3, 2),
    "fractional_bounds": ([(2.5, 3.5)], [3, 2], 2, 2),
}


@pytest.mark.parametrize("name", sorted(SPLIT_CASES))
def test_split_loop_exit_rule(name):
    occupied, script, want, consumed = SPLIT_CASES[name]
    script = list(script)
    n = len(script)
    with _Recorded(script) as rec:
        got = augment.draw_split(occupied, 40)
    assert got == want and n - len(script) == consumed == len(rec.values)


@pytest.mark.parametrize("mutation", sorted(ac.MUTATIONS))
def test_mutation_is_caught(items, mutation):
    caught = [n for n, d in items.items()
              if not np.array_equal(ac.chain(d["frame"], d["params"], d["noise"], **{mutation: True})["out"], d["im_t"])]
    assert caught, ac.MUTATIONS[mutation]


@pytest.mark.parametrize("name", NAMES)
def test_tables_and_records(items, name):
    d = items[name]
    H, W = d["frame"].shape[:2]
    p = d["params"]
    rec, tx, ty = augment.pack_params([p], W, H)
    assert rec.dtype.itemsize == 104 and rec["affine"][0].tolist() == p["affine"] and rec["order"][0].tolist() == p["order"]
    assert rec["factors"][0].tolist() == [float(np.float32(f)) for f in p["factors"]]
    for table, n_in, n_out in ((tx[0], W, p["rw"]), (ty[0], H, p["rh"])):
        xmin, k = ac.resample_coeffs(n_in, n_out)
        n = min(n_out, n_in)
        assert np.array_equal(table[:n, 0], xmin[:n])
        assert np.array_equal(table[:n, 1:1 + k.shape[1]], k[:n]) and (table[:n, 1 + k.shape[1]:] == 0).all()
        assert (table[n:] == 0).all()


def test_pack_params_rejects_what_the_kernels_cannot_do():
    p = augment.identity_params(50, 38)
    with pytest.raises(ValueError):
        augment.pack_params([dict(p, rh=9)], 50, 38)                  # shrinking by more than 3x: more than 7 taps
    with pytest.raises(ValueError):
        augment.pack_params([dict(p, dx=50)], 50, 38)
    with pytest.raises(ValueError):
        augment.pack_params([dict(p, order=[0, 1, 1, 3])], 50, 38)


def test_identity_record_changes_nothing():
    f = ac.frame_bytes("identity", 41, 27)
    p = augment.identity_params(41, 27)
    r = ac.chain(f, p, np.zeros_like(f))
    assert np.array_equal(r["jittered"], f)
    assert np.array_equal(r["out"], ac.finish(f, 0, 0))


def test_noise_generator_restatement():
    a = augment.noise_bytes(3, 2, 27, 41)
    assert a.dtype == np.uint8 and a.shape == (2, 27, 41, 3)
    assert np.array_equal(a, augment.noise_bytes(3, 2, 27, 41))
    assert not np.array_equal(a, augment.noise_bytes(4, 2, 27, 41)) and not np.array_equal(a[0], a[1])
    assert np.array_equal(a[0], augment.noise_bytes(3, 1, 27, 41)[0])          # keyed by the element, not by the batch size
    hist = np.bincount(augment.noise_bytes(1, 4, 64, 96).reshape(-1), minlength=256)
    assert hist[255] == 0 and hist[:255].min() > 0 and abs(hist[:255].mean() - hist.sum() / 255) < 1e-9
    for k in range(256):                                                        # byte(fp32(u) / 255 * 255) == u: copied pixels keep their byte
        assert int(np.float32(k) / np.float32(255.0) * np.float32(255.0)) == k


def test_jitter_draws_follow_the_published_order():
    """Parity unpinned (torchvision is absent): the draws are what RandomApply(p=.5) / ColorJitter.get_params document."""
    torch.manual_seed(5)
    seen = set()
    for _ in range(40):
        state = torch.get_rng_state()
        apply, order, factors = augment.draw_jitter()
        after = torch.get_rng_state()
        torch.set_rng_state(state)
        skip = bool(0.5 < torch.rand(1))
        assert apply == (not skip)
        if apply:
            assert order == torch.randperm(4).tolist()
            want = [float(torch.empty(1).uniform_(lo, hi)) for lo, hi in ((0.4, 1.6), (0.4, 1.6), (0.5, 1.5))]
            assert factors == want and 0.4 <= factors[0] <= 1.6 and 0.5 <= factors[2] <= 1.5
            seen.add(tuple(order))
        assert torch.equal(torch.get_rng_state(), after)
    assert len(seen) >= 3


def test_dropin_dataset_parses_as_the_reference(items, tmp_path, monkeypatch):
    """corrected_3D_dataset.Detection_Dataset: the reference's parsing, shuffle and 90/10 split; undecorated items; no crop mode."""
    import random
    import corrected_3D_dataset as dd
    names = ac.write_dataset(tmp_path, {n: d["frame"] for n, d in items.items()})
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError):
        dd.Detection_Dataset(str(tmp_path), CROP=112)
    seen = []
    for mode in ("train", "test"):
        random.seed(0)
        ds = dd.Detection_Dataset(str(tmp_path), mode=mode, CROP=0)
        assert len(ds) == (int(len(names) * 0.9) if mode == "train" else len(names) - int(len(names) * 0.9))
        for idx in range(len(ds)):
            frame, labels, camera, vps = ds[idx]
            d = items[names[ds.data[idx]]]
            seen.append(names[ds.data[idx]])
            assert frame.dtype == np.uint8 and np.array_equal(frame, d["frame"])
            assert camera == str(d["camera"]) and np.array_equal(np.array(vps, np.float64), d["vps"])
            if d["labels_in"].shape[0]:                                     # "empty" is put in by hand on both sides
                assert labels.numpy().dtype == d["labels_in"].dtype and np.array_equal(labels.numpy(), d["labels_in"])
    random.seed(0)
    order = [c[0] for c in ac.GOLDEN]
    random.shuffle(order)
    assert seen == order                                                    # the reference's shuffle, then train | test


PIL_SHAPES = [(50, 38), (41, 27), (96, 64)]


@pytest.mark.parametrize("W,H", PIL_SHAPES)
def test_restatement_against_pillow(W, H):
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    f = ac.frame_bytes("pillow%d" % W, W, H)
    im = Image.fromarray(f)
    for s, a in ((1, .75), (1.13, .8), (1, 1), (1.25, 1.4), (1.07, .93)):
        rh, rw = int(H * s * a), int(W * s)
        assert np.array_equal(np.array(im.resize((rw, rh), Image.BILINEAR)), ac.resize(f, rh, rw)), (s, a)
    for angle in (0, 20, -20, 19.999, 3.7, -11.3, 0.01):
        assert np.array_equal(np.array(im.rotate(angle, Image.BILINEAR)), ac.rotate(f, ac.affine(angle, W, H))), angle
        assert ac.affine(angle, W, H) == augment.affine_coefficients(angle, W, H)
    for fac in (0.4, 0.55, 0.9, 1.0, 1.3, 1.6):
        fac = float(np.float32(fac))
        for op, enh in ((0, ImageEnhance.Brightness), (1, ImageEnhance.Contrast), (2, ImageEnhance.Color)):
            assert np.array_equal(np.array(enh(im).enhance(fac)), ac.jitter(f, [op], [fac] * 3)[0]), (op, fac)

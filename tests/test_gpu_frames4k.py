"""GPU: the 4K frame intake (csrc/ts_parse.hip, csrc/ingest.hip) against the numpy restatement (tests/frames4k_cases.py) and
the reference's own results (tests/golden/frames4k.npz), bit for bit throughout.

Time stamps: cells below and above a wave (5x9 = 45, 7x11 = 77 pixels); n = 10, 11, 13, 16; B = 1, 3, 18; a strip inside a
larger frame at an odd x0 and through a row stride; a strip ending at, and running past, the frame's edge; empty areas; gray
127 / 128 from unequal channels and swap_rb; noise in the point's cell; a doubled table entry; flipped pixels; a second set;
the fall-back; 256 random stamps against float(text); the drop-in against the reference's returns.
Reduction + ingest: against ops.frame_ingest of the numpy-reduced frame and that frame itself; sizes on the pair path and
the byte path, below and past one block of either, B = 1 and 3, a base one byte off alignment."""
import numpy as np
import pytest
import torch

import frames4k_cases as fc
import timestamp_utilities as tsu
from retinanet_mi355x import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.retinanet_mi355x.*)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check(dev, frames, sets, prev=None, swap_rb=False, device_frames=None):
    """ops.parse_frame_timestamps on `frames` (numpy [B,H,W,3], or the device tensor given) against the restatement: every
    output.  -> the restatement's dict."""
    want = fc.parse_frames(list(frames), sets, prev=prev, swap_rb=swap_rb)
    f = torch.from_numpy(np.ascontiguousarray(frames)).to(dev) if device_frames is None else device_frames
    p = None if prev is None else torch.tensor(prev, dtype=torch.float64, device=dev)
    times, status, set_index, digits, fail_cell, mask = ops.parse_frame_timestamps(f, sets, prev=p, swap_rb=swap_rb, want_mask=True)
    assert times.dtype == torch.float64 and digits.dtype == torch.int8 and mask.dtype == torch.uint8
    assert np.array_equal(_bits(times.cpu().numpy()), _bits(want["times"]))
    assert np.array_equal(status.cpu().numpy(), want["status"])
    assert np.array_equal(set_index.cpu().numpy(), want["set_index"])
    assert np.array_equal(digits.cpu().numpy(), want["digits"])
    assert np.array_equal(fail_cell.cpu().numpy(), want["fail_cell"])
    assert np.array_equal(mask.cpu().numpy(), want["mask"])
    return want


@pytest.fixture(scope="module")
def cases():
    return fc.golden_cases()


def test_golden_cases_device_restatement_and_drop_in(dev, golden, cases):
    """Every case the reference ran: the op equals the restatement in every output, and the drop-in returns what the
    reference returned -- the same int or float, or None with the failing cell's mask pixels."""
    g = golden("frames4k")
    for c in cases:
        tag, geom, tab = c["name"] + "_", c["geom"], c["table"]
        r = _check(dev, c["frame"][None], [(geom, tab)])
        assert (r["status"][0] == fc.FAILED) == bool(g[tag + "failed"])
        for kind in ("numpy", "device", "strip"):
            if kind == "numpy":
                got, err = tsu.parse_frame_timestamp(geom, tab, frame_pixels=c["frame"])
            elif kind == "device":
                got, err = tsu.parse_frame_timestamp(geom, tab, frame_pixels=torch.from_numpy(c["frame"]).to(dev))
            else:
                strip = c["frame"][geom["y0"]:geom["y0"] + geom["h"], geom["x0"]:geom["x0"] + geom["n"] * geom["w"]]
                if strip.shape[0] == 0 or strip.shape[1] == 0:
                    continue
                got, err = tsu.parse_frame_timestamp(geom, tab, timestamp_pixels=np.ascontiguousarray(strip))
            if g[tag + "failed"]:
                assert got is None and err.dtype == np.uint8 and np.array_equal(err, g[tag + "err"]), (c["name"], kind)
            else:
                assert err is None and type(got) is (int if g[tag + "is_int"] else float), (c["name"], kind)
                assert float(got).hex() == float(g[tag + "time"]).hex(), (c["name"], kind)


def test_strip_through_strides_and_batches(dev):
    """B = 1, 3, 18 frames with their own stamps, read in place from a view of a larger buffer (a row stride, a frame
    stride, a base offset that is no multiple of 4), for a cell below a wave and one above."""
    for (w, h), n in (((5, 9), 16), ((7, 11), 13)):
        geom = fc.geometry(w, h, n, x0=9, y0=1)
        tab = fc.table(geom)
        H, W = h + 3, 9 + n * w + 2
        digits = fc.random_digits(18, 15, seed=11 + w)
        frames = np.stack([fc.render(fc.stamp_text(d, n), geom, H, W) for d in digits])
        for B in (1, 3, 18):
            big = torch.zeros((B, H + 5, W + 7, 3), dtype=torch.uint8, device=dev)
            view = big[:, 2:2 + H, 3:3 + W]
            view.copy_(torch.from_numpy(frames[:B]).to(dev))
            assert not view.is_contiguous() and view.data_ptr() % 4 != 0
            r = _check(dev, frames[:B], [(geom, tab)], device_frames=view)
            assert (r["status"] == fc.READ).all()
            assert [float(t).hex() for t in r["times"]] == [float(fc.stamp_text(d, n)).hex() for d in digits[:B]]


def test_swap_rb_and_gray_edges(dev, cases):
    """Gray exactly 127 and 128 from unequal channels: B,G,R frames, and the same frames stored R,G,B read with swap_rb; read
    without it they are whatever the restatement says."""
    c = dict((k["name"], k) for k in cases)["gray_127_128"]
    sets = [(c["geom"], c["table"])]
    assert _check(dev, c["frame"][None], sets)["status"][0] == fc.READ
    rgb = np.ascontiguousarray(c["frame"][None, :, :, ::-1])
    assert _check(dev, rgb, sets, swap_rb=True)["status"][0] == fc.READ
    _check(dev, rgb, sets, swap_rb=False)


def test_second_set_and_fall_back(dev):
    """Set 0: font 0 in 7x11 cells; set 1: font 1 in 6x10 cells elsewhere, n = 16, its table in another order.  One launch
    holds a frame either set reads, and one nobody reads: set index, value, and prev + 1/30.0 or NaN."""
    g0, g1 = fc.geometry(7, 11, 13, x0=3, y0=2), fc.geometry(6, 10, 16, x0=1, y0=14)
    t0, t1 = fc.table(g0), fc.table(g1, font=1, order=(3, 1, 4, 5, 9, 2, 6, 8, 7, 0))
    H, W = 26, 110
    a = fc.render(fc.stamp_text(fc.DIGITS, 13), g0, H, W)
    b = fc.render(fc.stamp_text(fc.DIGITS[3:] + fc.DIGITS[:3], 16), g1, H, W, font=1)
    both = a.copy()
    both[14:] = b[14:]                                                       # both stamps: the first set wins
    frames = np.stack([a, b, np.zeros_like(a), both])
    prev = [1.5, 2.5, 1620398457.123456, 4.5]
    r = _check(dev, frames, [(g0, t0), (g1, t1)], prev=prev)
    assert list(r["set_index"]) == [0, 1, -1, 0] and list(r["status"]) == [fc.READ, fc.READ, fc.FELL_BACK, fc.READ]
    assert float(r["times"][1]).hex() == float(fc.stamp_text(fc.DIGITS[3:] + fc.DIGITS[:3], 16)).hex()
    assert float(r["times"][2]).hex() == (1620398457.123456 + 1 / 30.0).hex()
    r = _check(dev, frames, [(g0, t0), (g1, t1)])
    assert np.isnan(r["times"][2]) and r["status"][2] == fc.FAILED and r["fail_cell"][1] >= 0
    r = _check(dev, frames[2:3], [(g1, t1), (g0, t0), (g1, t1), (g0, t0)], prev=[7.0])     # four sets, every one failing
    assert float(r["times"][0]).hex() == (7.0 + 1 / 30.0).hex()


def test_256_random_stamps_equal_the_literal(dev):
    geom = fc.geometry(5, 9, 13)
    tab = fc.table(geom)
    digits = fc.random_digits(256, 12, seed=29)
    texts = [fc.stamp_text(d, 13) for d in digits]
    frames = np.stack([fc.render(t, geom, 9, 65) for t in texts])
    times = ops.parse_frame_timestamps(torch.from_numpy(frames).to(dev), [(geom, tab)])[0].cpu().numpy()
    assert [float(t).hex() for t in times] == [float(t).hex() for t in texts]


def test_reader_keeps_prev_on_the_device(dev):
    geom = fc.geometry(7, 11, 13)
    tab = fc.table(geom)
    reader = tsu.TimestampReader([(geom, tab)], 2, device=dev)
    good = fc.render(fc.stamp_text(fc.DIGITS, 13), geom, 11, 91)
    blank = np.zeros_like(good)
    t, s = reader(torch.from_numpy(np.stack([good, blank])).to(dev))
    want = float(fc.stamp_text(fc.DIGITS, 13))
    assert t.cpu().tolist() == [want, 0.0 + 1 / 30.0] and s.cpu().tolist() == [fc.READ, fc.FELL_BACK]
    t, s = reader(torch.from_numpy(np.stack([blank, blank])).to(dev))
    assert t.cpu().tolist() == [want + 1 / 30.0, 1 / 30.0 + 1 / 30.0] and s.cpu().tolist() == [fc.FELL_BACK] * 2


# ----------------------------------------------------------------------------- reduction + ingest
HALF_SIZES = [(2, 2), (2, 8), (6, 10), (22, 190), (22, 188), (10, 520)]   # input H x W; the last two: past one block of the pair path


def _half_inputs(B, H2, W2):
    return dict(random=fc.rng_bytes((B, H2, W2, 3), seed=H2 * 1000 + W2 + B), white=np.full((B, H2, W2, 3), 255, np.uint8),
                residues=np.repeat(fc.residue_blocks(H2, W2), B, axis=0))


@pytest.mark.parametrize("size", HALF_SIZES)
@pytest.mark.parametrize("B", [1, 3])
def test_half_ingest_equals_ingest_of_the_reduced_frame(dev, size, B):
    H2, W2 = size
    mean, std = (0.1, 0.2, 0.3), (0.5, 0.25, 2.0)
    for name, f in _half_inputs(B, H2, W2).items():
        small = fc.reduce_half(f)
        assert small.shape == (B, H2 // 2, W2 // 2, 3)
        if name == "residues":
            sums = f.astype(np.int64).reshape(B, H2 // 2, 2, W2 // 2, 2, 3).sum(axis=(2, 4))
            assert H2 * W2 < 56 or set(np.unique(sums)) == set(range(7)) | set(range(1014, 1021))
        fd, sd = torch.from_numpy(f).to(dev), torch.from_numpy(small).to(dev)
        shifted = torch.zeros(f.size + 1, dtype=torch.uint8, device=dev)
        shifted[1:].copy_(fd.reshape(-1))
        shifted = shifted[1:].view(fd.shape)
        assert shifted.data_ptr() % 2 == 1 and shifted.is_contiguous()
        for nhwc4 in (False, True):
            for swap in (False, True):
                want = ops.frame_ingest(sd, swap_rb=swap, nhwc4=nhwc4)
                got, u8 = ops.frame_ingest_half(fd, swap_rb=swap, nhwc4=nhwc4, keep_u8=True)
                assert got.shape == want.shape and torch.equal(got, want), (name, nhwc4, swap)
                assert u8.dtype == torch.uint8 and torch.equal(u8, sd), (name, nhwc4, swap)
                assert torch.equal(ops.frame_ingest_half(fd, swap_rb=swap, nhwc4=nhwc4), want)
                got, u8 = ops.frame_ingest_half(shifted, swap_rb=swap, nhwc4=nhwc4, keep_u8=True)
                assert torch.equal(got, want) and torch.equal(u8, sd), (name, nhwc4, swap, "one byte off")
        want = ops.frame_ingest(sd, mean=mean, std=std)
        assert torch.equal(ops.frame_ingest_half(fd, mean=mean, std=std), want)
    with pytest.raises(RuntimeError, match="even"):
        ops.frame_ingest_half(torch.zeros((1, 3, 4, 3), dtype=torch.uint8, device=dev))


def test_load_frames_4k_returns_frames_and_stamps_from_one_call(dev):
    geom = fc.geometry(4, 7, 13, x0=5, y0=1)
    tab = fc.table(geom)
    digits = fc.random_digits(3, 12, seed=41)
    frames = np.stack([fc.render(fc.stamp_text(d, 13), geom, 8, 64) for d in digits])
    frames[2, 1:8, 5 + 12:5 + 16] = 255                                      # the third frame's cell 3 is unreadable
    fd = torch.from_numpy(frames).to(dev)
    reader = tsu.TimestampReader([(geom, tab)], 3, device=dev)
    reader.prev = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device=dev)
    (x, u8), t, s = ops.load_frames_4k(fd, reader, nhwc4=True, keep_u8=True)
    small = torch.from_numpy(fc.reduce_half(frames)).to(dev)
    assert torch.equal(u8, small) and torch.equal(x, ops.frame_ingest(small, nhwc4=True)) and tuple(x.shape) == (3, 4, 32, 4)
    assert t.cpu().tolist() == [float(fc.stamp_text(digits[0], 13)), float(fc.stamp_text(digits[1], 13)), 3.0 + 1 / 30.0]
    assert s.cpu().tolist() == [fc.READ, fc.READ, fc.FELL_BACK]
    got = torch.ops.retinanet_mi355x.parse_frame_timestamps(fd, [int(v) for v in reader.geometry.reshape(-1)], reader.table, None, False)
    assert got[1].cpu().tolist() == [fc.READ, fc.READ, fc.FAILED] and got[4].cpu().tolist() == [-1, -1, 3]
    x2, u2 = torch.ops.retinanet_mi355x.frame_ingest_half(fd, False, True)
    assert torch.equal(x2, x) and torch.equal(u2, u8)

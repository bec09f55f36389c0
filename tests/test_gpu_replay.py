"""GPU: the four kernels of csrc/replay.hip, Camera_Wrapper, test_integrity and Data_Reader.plot_in against the plain
restatement of tests/replay_cases.py.  Bit for bit, except the image corners, which are held to the project's projection bound
(rtol 1e-9, atol 1e-8: the device sums the 3x4 product in the reference's order, the restatement through numpy)."""
import os

import numpy as np
import pytest
import torch

import datareader_cases as dc
import frames4k_cases as fc
import render_cases as rc
import replay_cases as rp

import datareader
import homography
import mc3d_render
import timestamp_utilities as tsu
from retinanet_mi355x import ops

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ replay_boxes
@pytest.mark.parametrize("n", [0, 1, 257])
@pytest.mark.parametrize("wrapper", [False, True])
def test_replay_boxes(dev, n, wrapper):
    all_names, P, P2 = dc.cameras()
    names = ["p1c2", "p2c4", "p1c5"]
    idx = [all_names.index(c) for c in names]
    dts = np.array([-0.0371, 0.0, 0.0519], np.float64)                           # negative, zero, positive
    pad = 5                                                                       # rows in front: the offset is used
    st = rp.boxes_case(n + pad)
    want = rp.boxes(st[pad:], dts, names, all_names, P, P2 if wrapper else None)
    got = ops.replay_boxes(t(st, dev), t(dts, dev), t(P[idx], dev), t(P2[idx], dev) if wrapper else None, pad, n)
    views, im, side, cam = (g.cpu().numpy() for g in got)
    assert views.shape == (3 * n, 7) and im.shape == (3 * n, 8, 2) and side.dtype == cam.dtype == np.int32
    assert views.tobytes() == want[0].tobytes()
    assert np.array_equal(side, want[2]) and np.array_equal(cam, want[3])
    if n:
        finite = np.isfinite(want[1]).all(axis=(1, 2))
        assert np.array_equal(np.isfinite(im).all(axis=(1, 2)), finite)
        assert np.allclose(im[finite], want[1][finite], rtol=rp.RTOL, atol=rp.ATOL)
        print("n=%d wrapper=%s: largest corner deviation %.3e" % (n, wrapper, np.abs(im[finite] - want[1][finite]).max()))
    if n == 257:
        y = st[pad:, 1]
        assert (y == 60).any() and (y > 60).any() and (y < 60).any() and set(st[pad:, 5]) == {-1.0, 1.0}
        assert side[:n][y == 60].tolist() == [0] * int((y == 60).sum())
        assert (views[n:2 * n] == st[pad:]).all() and (views[:n, 0] != st[pad:, 0]).any()      # dt = 0 moves nothing


def test_replay_boxes_refusals(dev):
    st, dt, P = torch.zeros(4, 7, device=dev), torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, 3, 4, dtype=torch.float64, device=dev)
    for bad in (lambda: ops.replay_boxes(st.double(), dt, P), lambda: ops.replay_boxes(st, dt.float(), P),
                lambda: ops.replay_boxes(st, dt, P[:1]), lambda: ops.replay_boxes(st[:, :6].contiguous(), dt, P),
                lambda: ops.replay_boxes(st, dt, P, None, 3, 2), lambda: ops.replay_boxes(st, dt, P, None, -1, 2),
                lambda: ops.replay_boxes(st, dt, P, P.float())):
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------------------------------------------------ replay_compose
@pytest.fixture(scope="module")
def planes():
    """Frames and an all-combinations mask for six cameras of EDGE_SHAPE's 37 x 67; fewer cameras take the first ones."""
    _, H, W = rc.EDGE_SHAPE
    frames = np.random.RandomState(4).randint(0, 256, (6, H, W, 3)).astype(np.uint8)
    frames[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 1], [1, 0, 255]]
    return frames, rc.all_masks(6, H, W, 12)


@pytest.mark.parametrize("C", [1, 2, 3, 5, 6])
def test_replay_compose(dev, planes, C):
    frames, mask = planes[0][:C], planes[1][:C]
    assert C > 1 or len(set((mask[0] & 15).reshape(-1).tolist())) == 16          # every combination of the four bits
    _, H, W = mask.shape
    rows, cols = rp.layout(C)
    CW, CH = cols * W, rows * H
    d_frames = t(frames, dev)
    d_mask = ops.render_mask(C, H, W, dev)
    d_mask.copy_(t(mask, dev))
    sizes = [None, (CW, CH), (CW // 2, CH // 2) if CW % 2 == 0 and CH % 2 == 0 else (CW // 2 + 1, CH // 2), (29, 50), (2 * CW + 3, CH + 11),
             (1, 1), (CW, 7)]
    for swap in (False, True):
        for size in sizes:
            got = ops.replay_compose(d_frames, d_mask, size, swap).cpu().numpy()
            want = rp.compose(frames, mask, size, swap)
            assert got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (C, size, swap, int((got != want).sum()))
    empty = ops.replay_compose(d_frames, ops.render_mask(C, H, W, dev)).cpu().numpy()    # an empty mask gives the frames back
    for i in range(C):
        r, c = rp.tile_of(i, C)
        assert np.array_equal(empty[r * H:(r + 1) * H, c * W:(c + 1) * W], frames[i])


def test_replay_compose_exact_halving_and_aligned_rows(dev):
    """W a multiple of 4 (the vector path of every row) and an exact 2:1 reduction of a 2 x 2 mosaic."""
    C, H, W = 4, 10, 16
    rs = np.random.RandomState(8)
    frames = rs.randint(0, 256, (C, H, W, 3)).astype(np.uint8)
    mask = rs.randint(0, 16, (C, H, W)).astype(np.uint16)
    d_mask = ops.render_mask(C, H, W, dev)
    d_mask.copy_(t(mask, dev))
    for size in (None, (W, H), (3 * W, 3 * H)):
        assert np.array_equal(ops.replay_compose(t(frames, dev), d_mask, size).cpu().numpy(), rp.compose(frames, mask, size))
    with pytest.raises(RuntimeError):
        ops.replay_compose(t(frames, dev)[:3], d_mask)
    with pytest.raises(RuntimeError):
        ops.replay_compose(t(frames, dev), d_mask, (0, 5))
    with pytest.raises(RuntimeError):
        ops.replay_compose(t(frames, dev).float(), d_mask)


# ------------------------------------------------------------------------------------------------ frame_absdiff, running_frame
def test_frame_absdiff(dev):
    rs = np.random.RandomState(6)
    a, b = (rs.randint(0, 256, (12, 20, 3)).astype(np.uint8) for _ in range(2))
    for win in ((3, 9, 4, 15), (5, 40, 7, 90), (0, 12, 0, 20), (9, 9, 2, 8), (6, 3, 2, 8), (100, 500, 100, 500)):    # inner, clipped, whole, empty
        got = ops.frame_absdiff(t(a, dev), t(b, dev), *win)
        assert got.dtype == torch.int64 and int(got) == rp.absdiff(a, b, *win), win
    lo, hi = np.zeros((12, 20, 3), np.uint8), np.full((12, 20, 3), 255, np.uint8)
    assert int(ops.frame_absdiff(t(lo, dev), t(hi, dev), 0, 12, 0, 20)) == int(ops.frame_absdiff(t(hi, dev), t(lo, dev), 0, 12, 0, 20)) == 255 * 720
    a, b = (rs.randint(0, 256, (600, 520, 3)).astype(np.uint8) for _ in range(2))   # the real window: many workgroups
    da, db = t(a, dev), t(b, dev)
    first = int(ops.frame_absdiff(da, db))
    assert first == rp.absdiff(a, b) and all(int(ops.frame_absdiff(da, db)) == first for _ in range(3))
    assert datareader.absdiff_mean(first, 600, 520) == np.mean(np.abs(a[100:500, 100:500, :].astype(float) - b[100:500, 100:500, :].astype(float)))
    assert datareader.absdiff_mean(0, 50, 900) is None
    with pytest.raises(RuntimeError):
        ops.frame_absdiff(da, db[:500])
    with pytest.raises(RuntimeError):
        ops.frame_absdiff(da, db, -1, 5, 0, 5)


def test_running_frame(dev):
    _, H, W = rc.EDGE_SHAPE
    frames = [np.random.RandomState(s).randint(0, 256, (H, W, 3)).astype(np.uint8) for s in (1, 2, 3)]
    frames[1][0, 0] = [0, 255, 1]
    want = rp.running(frames)
    run = torch.full((H, W, 3), np.nan, dtype=torch.float64, device=dev)
    for k, f in enumerate(frames):
        ops.running_frame(run, t(f, dev), k == 0)
        assert run.cpu().numpy().tobytes() == want[k].tobytes(), k
    with pytest.raises(RuntimeError):
        ops.running_frame(run.float(), t(frames[0], dev))


# ------------------------------------------------------------------------------------------------ Camera_Wrapper, test_integrity
class Loader:
    """A source as Camera_Wrapper takes it: an iterator of uint8 [h,w,3] frames with a ``.sequence`` string."""

    def __init__(self, frames, sequence, device=None):
        self.frames, self.sequence, self.device, self.k, self.released = list(frames), sequence, device, 0, False

    def __len__(self):
        return len(self.frames)

    def __next__(self):
        if self.k >= len(self.frames):
            raise StopIteration
        f = self.frames[self.k]
        self.k += 1
        return f if self.device is None else t(f, self.device)

    def release(self):
        self.released = True


G0, G1 = fc.geometry(7, 11, 13, x0=3, y0=2), fc.geometry(6, 10, 16, x0=1, y0=14)


def two_sets():
    return [(G0, fc.table(G0)), (G1, fc.table(G1, font=1, order=(3, 1, 4, 5, 9, 2, 6, 8, 7, 0)))]


@pytest.mark.parametrize("ds", [1, 2])
def test_camera_wrapper(dev, ds, capsys):
    H, W = 26, 110
    first = fc.render(fc.stamp_text(fc.DIGITS, 13), G0, H, W)
    second = fc.render(fc.stamp_text(fc.DIGITS[3:] + fc.DIGITS[:3], 16), G1, H, W, font=1)
    noise = np.random.RandomState(3).randint(0, 100, (H, W, 3)).astype(np.uint8)   # dark: nobody reads it
    frames = [first, second, noise, first, noise]
    sets = two_sets()
    stamps = fc.parse_frames(frames[:1], sets)["times"].tolist()
    cam = datareader.Camera_Wrapper(Loader(frames, "/data/rec_p2c3_0.mp4", dev if ds == 1 else None), ds=ds,
                                    reader=tsu.TimestampReader(sets, 1, device=dev))
    assert cam.name == "p2c3" and cam.ts is None and cam.frame is None and cam.running_frame is None and len(cam) == 5 and cam.ds == ds
    want_ts = [float(fc.stamp_text(fc.DIGITS, 13)), float(fc.stamp_text(fc.DIGITS[3:] + fc.DIGITS[:3], 16))]
    want_ts += [want_ts[1] + 1 / 30.0, want_ts[0], want_ts[0] + 1 / 30.0]
    assert stamps[0] == want_ts[0]
    shown = [fc.reduce_half(f[None])[0] if ds == 2 else f for f in frames]
    want_run = rp.running(shown)
    for k in range(5):
        next(cam)
        assert cam.ts == want_ts[k] and isinstance(cam.ts, float) and cam.all_ts == want_ts[:k + 1]
        assert cam.frame.is_cuda and cam.frame.dtype == torch.uint8 and np.array_equal(cam.frame.cpu().numpy(), shown[k])
        assert cam.running_frame.dtype == torch.float64 and cam.running_frame.cpu().numpy().tobytes() == want_run[k].tobytes()
        out = capsys.readouterr().out
        assert out == ("No timestamp parsed: p2c3\n" if k in (2, 4) else ""), (k, out)
    with pytest.raises(StopIteration):
        next(cam)
    cam.release()
    assert cam.source.released
    skipper = datareader.Camera_Wrapper(Loader(frames, "p1c1", dev), ds=1, reader=tsu.TimestampReader(sets, 1, device=dev))
    skipper.skip(3)                                                              # three frames taken unseen, then one read
    assert skipper.ts == want_ts[0] and skipper.all_ts == [want_ts[0]] and skipper.source.k == 4


def test_integrity_counts(dev, tmp_path, capsys):
    stamps, frames = rp.integrity_case()
    geom = fc.geometry(5, 9, 16, x0=2, y0=1)
    sets = [(geom, fc.table(geom))]
    stamped = []
    for s, f in zip(stamps, frames):
        g = f.copy()
        g[:12, :90] = fc.render("%016.5f" % (1623877000.0 + s), geom, 12, 90)      # outside the window [100:500]^2
        stamped.append(g)
    want = rp.integrity([float("%016.5f" % (1623877000.0 + s)) for s in stamps], stamped)
    assert want["doubled_ts"] == want["doubled_frame"] == want["doubled_both"] == want["skipped_ts"] == 1 and want["correct"] > 5
    save = os.path.join(str(tmp_path), "flagged")
    got = datareader.test_integrity(Loader(stamped, "p3c2", dev), n=1000, save_dir=save, reader=tsu.TimestampReader(sets, 1, device=dev))
    assert got == want
    out = capsys.readouterr().out.splitlines()
    assert out == ["Camera p3c2 results for 1000 frames:", "Doubled timestamps occured 1 times", "Doubled both occured 1 times",
                   "Doubled frames occured 1 times", "Skipped timestamps occurred 1 times"]
    assert len(os.listdir(save)) >= 4 * 3 and all(n.startswith("p3c2_") and n.endswith(".png") for n in os.listdir(save))
    short = datareader.test_integrity(Loader(stamped[:7], "p3c2", dev), n=5, reader=tsu.TimestampReader(sets, 1, device=dev))
    assert short == rp.integrity([float("%016.5f" % (1623877000.0 + s)) for s in stamps[:7]], stamped[:7], n=5)
    small = [f[:60, :100].copy() for f in stamped[:6]]                            # the window is empty: never "doubled frame"
    small[3] = small[2].copy()
    assert datareader.test_integrity(Loader(small, "p3c2", dev), n=6, reader=tsu.TimestampReader(sets, 1, device=dev))["doubled_frame"] == 0


# ------------------------------------------------------------------------------------------------ plot_in
REPLAY_H, REPLAY_W = 108, 192
REPLAY_GEOM = fc.geometry(5, 9, 16, x0=100, y0=2)


def replay_matrices():
    """Three cameras looking straight down on the fixture's road (x 100..400 ft, y 0..120 ft) through 192 x 108 pixels, each
    with its own scale and a little perspective; the second set differs slightly, as a wrapper's does."""
    P, P2 = np.zeros((3, 3, 4)), np.zeros((3, 3, 4))
    for c, (sx, ox, sy, oy) in enumerate(((0.50, -45.0, 0.80, 4.0), (0.45, -30.0, 0.75, 8.0), (0.55, -60.0, 0.78, 2.0))):
        P[c] = [[sx, 0.02, 0.1, ox], [0.01, sy, -1.2, oy], [0.0002, 0.0001, 0.0, 1.0]]
        P2[c] = [[sx * 1.02, 0.02, 0.1, ox - 2.0], [0.01, sy * 0.98, -1.1, oy + 1.0], [0.0002, 0.0001, 0.0, 1.0]]
    return P, P2


def test_plot_in_end_to_end(dev, tmp_path):
    names = list(rp.GOLDEN_CAMERAS)
    text = dc.tracking_csv(**rp.GOLDEN_CSV)
    _, data = dc.load(text)
    script = np.array([[float("%.5f" % s) for s in row] for row in rp.script(data, n=30)])
    sets = [(REPLAY_GEOM, fc.table(REPLAY_GEOM))]
    rs = np.random.RandomState(17)
    base = rs.randint(0, 120, (3, REPLAY_H, REPLAY_W, 3)).astype(np.uint8)

    def frames_of(c):
        out = []
        for k, s in enumerate(script[c]):
            f = base[c].copy()
            f[40 + k % 7, 3 * k % REPLAY_W] = 200                                  # every frame differs
            stamp = fc.render("%.5f" % s, REPLAY_GEOM, 12, REPLAY_W)
            f[:12] = np.where(stamp > 0, stamp, f[:12] // 4)
            out.append(f)
        return out
    per_cam = [frames_of(c) for c in range(3)]
    assert fc.parse_frames([per_cam[1][4]], sets)["times"][0] == script[1][4]
    P, P2 = replay_matrices()

    def one(M):
        hg = homography.Homography()
        hg.correspondence = {n: {"P": M[i]} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    hg = homography.Homography_Wrapper(hg1=one(P), hg2=one(P2))
    path = os.path.join(str(tmp_path), "in.csv")
    with open(path, "w", newline="") as f:
        f.write(text)
    # the restatement: the loop, then per frame boxes, labels and the canvas
    cams = [rp.ScriptedCamera(n, s) for n, s in zip(names, script)]
    for c in cams:
        next(c)
    want_log = rp.walk(data, cams)
    assert len(want_log) >= 6 and want_log[-1][0] == len(data) - 1
    inside = total = 0
    for inst, _, dts in want_log:
        _, im, _, _ = rp.boxes(rp.state7(data[inst]), dts, names, names, P, P2)
        ok = (im[:, :, 0] >= 0) & (im[:, :, 0] < REPLAY_W) & (im[:, :, 1] >= 0) & (im[:, :, 1] < REPLAY_H)
        inside, total = inside + int(ok.all(1).sum()), total + len(im)
    assert 2 * inside >= total, (inside, total)                                   # at least half of the boxes lie in their frame

    out_dir = os.path.join(str(tmp_path), "frames")
    canvases, corners = [], []

    class Keep(mc3d_render.Replayer):
        def replay(self, frames, *a, **kw):
            shown = np.stack([f.cpu().numpy() for f in frames])
            canvas = super().replay(frames, *a, **kw)
            canvases.append((shown, canvas.cpu().numpy()))
            corners.append({k: v.cpu().numpy() for k, v in self.last.items()})
            return canvas
    real, mc3d_render.Replayer = mc3d_render.Replayer, Keep
    try:
        dr = datareader.Data_Reader(path, hg)
        wrappers = [datareader.Camera_Wrapper(Loader(per_cam[c], "cam_%s.mp4" % names[c], dev if c else None), ds=1,
                                              reader=tsu.TimestampReader(sets, 1, device=dev)) for c in range(3)]
        n = dr.plot_in(wrappers, render={"out": out_dir, "size": None, "max_frames": None})
    finally:
        mc3d_render.Replayer = real
    H, W = REPLAY_H, REPLAY_W
    assert n == len(want_log) == len(dr.replay_log) == len(canvases)
    for got, want in zip(dr.replay_log, want_log):
        assert got[0] == want[0] and np.array(got[1]).tobytes() == np.array(want[1]).tobytes()
        assert np.array(got[2]).tobytes() == np.array(want[2]).tobytes()
    font = mc3d_render.FONT
    for (inst, stamps, dts), (shown, canvas), last in zip(want_log, canvases, corners):
        st = rp.state7(data[inst])
        views, im, side, cam = rp.boxes(st, dts, names, names, P, P2)
        assert last["views"].tobytes() == views.tobytes() and np.array_equal(last["side"], side) and np.array_equal(last["cam"], cam)
        assert np.allclose(last["corners"], im, rtol=rp.RTOL, atol=rp.ATOL)
        for c in range(3):
            k = list(script[c]).index(stamps[c])
            assert np.array_equal(shown[c], per_cam[c][k])
        lines = rp.frame_lines(data[inst], st, dc._first_ts(data[inst]), dts)
        want = rp.replay_frame(shown, font, last["corners"], side, cam, lines)    # painted from the device's own corners
        assert canvas.shape == (2 * H, 2 * W, 3) and np.array_equal(canvas, want), int((canvas != want).sum())
        assert (canvas != rp.compose(shown, np.zeros((3, H, W), np.uint16))).any()         # something was drawn
    assert np.array_equal(dr.replayed.cpu().numpy(), canvases[-1][1])
    assert sorted(os.listdir(out_dir)) == ["combined"]
    assert sorted(os.listdir(os.path.join(out_dir, "combined"))) == ["%05d.png" % k for k in range(n)]
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, "combined", "%05d.png" % (n - 1)))), canvases[-1][1])


def test_plot_in_resized_and_limited(dev, tmp_path):
    """max_frames, an output size, loaders wrapped by plot_in itself (ds = 2: the halved frames are shown), a plain Homography,
    B,G,R frames, no directory: nothing is written."""
    names = list(rp.GOLDEN_CAMERAS)
    text = dc.tracking_csv(**rp.GOLDEN_CSV)
    _, data = dc.load(text)
    script = np.array([[float("%.5f" % s) for s in row] for row in rp.script(data, n=12)])
    sets = [(REPLAY_GEOM, fc.table(REPLAY_GEOM))]
    base = np.random.RandomState(18).randint(0, 120, (3, REPLAY_H, REPLAY_W, 3)).astype(np.uint8)
    per_cam = []
    for c in range(3):
        per_cam.append([])
        for s in script[c]:
            f = base[c].copy()
            stamp = fc.render("%.5f" % s, REPLAY_GEOM, 12, REPLAY_W)
            f[:12] = np.where(stamp > 0, stamp, f[:12] // 4)
            per_cam[c].append(f)
    P, _ = replay_matrices()
    hg = homography.Homography()
    hg.correspondence = {n: {"P": P[i]} for i, n in enumerate(names)}
    hg.default_correspondence = names[0]
    path = os.path.join(str(tmp_path), "in.csv")
    with open(path, "w", newline="") as f:
        f.write(text)
    dr = datareader.Data_Reader(path, hg)
    size = (250, 141)
    n = dr.plot_in([Loader(per_cam[c], names[c], dev) for c in range(3)],
                   render={"out": None, "size": size, "max_frames": 3, "swap_rb": True, "sets": sets})
    assert n == 3 and len(dr.replay_log) == 3 and tuple(dr.replayed.shape) == (141, 250, 3) and dr.replayed.is_cuda
    cams = [rp.ScriptedCamera(nm, s) for nm, s in zip(names, script)]
    for c in cams:
        next(c)
    inst, stamps, dts = rp.walk(data, cams, max_frames=3)[-1]
    assert dr.replay_log[-1][0] == inst and dr.replay_log[-1][2] == dts
    shown = np.stack([fc.reduce_half(per_cam[c][list(script[c]).index(stamps[c])][None])[0] for c in range(3)])
    last = {k: v.cpu().numpy() for k, v in dr.replayer.last.items()}
    st = rp.state7(data[inst])
    lines = rp.frame_lines(data[inst], st, dc._first_ts(data[inst]), dts)
    want = rp.replay_frame(shown, mc3d_render.FONT, last["corners"], last["side"], last["cam"], lines, size, True)
    assert np.array_equal(dr.replayed.cpu().numpy(), want)
    assert os.listdir(str(tmp_path)) == ["in.csv"]

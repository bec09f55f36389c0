"""CPU: the restatement of the tracking-CSV replay in tests/replay_cases.py against the reference's own plot_in
(tests/golden/replay.npz, written by tools/make_golden_replay.py), the resampling rule at its edges, and the host side of the
mirror (datareader.py, mc3d_render.Replayer, the four operators of csrc/replay.hip): signatures, registration, refusals.

Bit-equal with the reference: the label instant, the camera stamps and dt of every output frame (Python floats, the loop as
written), the shifted fp32 states (one rounding per operation), the label strings and the tiles.  The image corners go through
the reference's BLAS matrix product: numeric, at the project's projection bound (rtol 1e-9, atol 1e-8)."""
import inspect
import os

import numpy as np
import pytest

import datareader_cases as dc
import render_cases as rc
import replay_cases as rp


@pytest.fixture(scope="module")
def scene(golden):
    g = golden("replay")
    text = g["csv"].tobytes().decode()
    assert text == dc.tracking_csv(**rp.GOLDEN_CSV)                               # the generator is portable: same bytes
    names = [str(n) for n in g["names"]]
    assert tuple(names) == rp.GOLDEN_CAMERAS
    _, data = dc.load(text)
    return g, names, data


def scripted(names, stamps):
    cams = [rp.ScriptedCamera(n, s) for n, s in zip(names, stamps)]
    for c in cams:
        next(c)
    return cams


def test_fixture_covers_what_it_is_for(scene):
    g, names, data = scene
    assert np.array_equal(g["script"], rp.script(data))
    inst = g["inst"]
    assert (np.diff(inst) >= 2).any() and (np.diff(inst) == 0).any() and inst[-1] == len(data) - 1       # a jump, a repeat, the end
    assert (g["stamps"].max(1) - g["stamps"].min(1) < 1 / 25.0).all()            # a lagging camera is caught up, by at most a frame
    assert g["script"][1, 0] + 1 / 60.0 < g["script"][0, 0]                       # camera 1 starts lagging
    assert "p2c1" not in data[0][next(iter(data[0]))]["ts_bias"]                  # the KeyError branch
    y = g["views"][:, 1]
    assert (y > 60).any() and (y < 60).any()
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "replay.npz")) < 200 * 1024


def test_loop_equals_the_reference(scene):
    g, names, data = scene
    got = rp.walk(data, scripted(names, g["script"]))
    assert [w[0] for w in got] == g["inst"].tolist()
    assert np.array([w[1] for w in got], np.float64).tobytes() == g["stamps"].tobytes()
    assert np.array([w[2] for w in got], np.float64).tobytes() == g["dt"].tobytes()
    assert len(rp.walk(data, scripted(names, g["script"]), max_frames=4)) == 4
    short = rp.walk(data, scripted(names, g["script"][:, :6]))                    # a source that ends early ends the loop
    assert 0 < len(short) < len(got) and [w[0] for w in short] == g["inst"].tolist()[:len(short)]


def test_boxes_labels_and_tiles_equal_the_reference(scene):
    g, names, data = scene
    all_names, P, P2 = dc.cameras()
    C, at, worst = len(names), 0, 0.0
    strings = [str(s) for s in g["strings"]]
    rects, texts, lines = g["rects"], g["texts"], g["lines"]
    r_at = t_at = 0
    for f, inst in enumerate(g["inst"].tolist()):
        frame, ts = data[inst], dc._first_ts(data[inst])
        st = rp.state7(frame)
        n = len(st)
        assert n == g["n"][f]
        views, im, side, cam = rp.boxes(st, g["dt"][f], names, all_names, P, P2)
        want_views, want_im = g["views"][at:at + C * n], g["corners"][at:at + C * n]
        at += C * n
        assert views.tobytes() == want_views.tobytes()                            # the shift, bit for bit
        assert np.allclose(im, want_im, rtol=rp.RTOL, atol=rp.ATOL)
        worst = max(worst, float(np.abs(im - want_im).max()))
        want_lines = rp.frame_lines(frame, st, ts, [np.float64(d) for d in g["dt"][f]])
        for c in range(C):
            # boxes: the colour of every line call is the side's (BGR in the reference)
            mine = lines[(lines[:, 0] == f) & (lines[:, 1] == c)]
            assert len(mine) == 14 * n and (mine[:, 9] == rp.THICKNESS).all()
            blue = (mine[:, 6:9] == (255, 0, 0)).all(1)
            assert int(blue.sum()) == 14 * int((side[cam == c] == 0).sum()) and (mine[~blue, 6:9] == (0, 255, 0)).all()
            for i in range(n):
                box = want_im[c * n + i]
                ax, ay = int(box[:, 0].min()), int(box[:, 1].max())          # :276-279; the painters skip one outside +-8192
                ls = want_lines[c][i]
                longest = max(len(line) for line in ls)
                rect = rects[r_at]
                r_at += 1
                assert rect[:6].tolist() == [f, c, ax, ay, ax + 6 * longest + 10, ay + 12 * len(ls)] and rect[9] == -1
                for k, line in enumerate(ls):
                    for copy in range(2):                                         # im and im2
                        assert strings[t_at] == line, (f, c, i, k, strings[t_at], line)
                        assert texts[t_at][:4].tolist() == [f, c, ax, ay + 12 * (k + 1)]
                        t_at += 1
        tiles = np.full(rp.layout(C), -1, np.int64)
        for i in range(C):
            tiles[rp.tile_of(i, C)] = i
        assert np.array_equal(g["tiles"][f], tiles)
    assert r_at == len(rects) and t_at == len(texts) == len(strings)
    print("largest corner deviation restated vs reference %.3e px" % worst)


def test_shift_order_matters():
    """The fp32 order of :345 is not the fp64 product rounded once: the two differ on some rows, so the test above can tell."""
    rs = np.random.RandomState(0)
    st = rp.boxes_case(4096, seed=1)
    dt = rs.uniform(-0.1, 0.1)
    other = (st[:, 6].astype(np.float64) * dt).astype(np.float32) * st[:, 5] + st[:, 0]
    assert (rp.shift(st, dt)[:, 0] != other).any()


def _canvas(CH, CW, seed):
    return np.random.RandomState(seed).randint(0, 256, (CH, CW, 3)).astype(np.int64)


def test_resample_rule():
    cv = _canvas(12, 20, 1)
    assert np.array_equal(rp.resample(cv, 20, 12), cv)                             # canvas size in: the identity
    half = rp.resample(cv, 10, 6)                                                 # exact 2:1: the rounded mean of each 2x2 block
    blocks = cv[0::2, 0::2] + cv[0::2, 1::2] + cv[1::2, 0::2] + cv[1::2, 1::2]
    assert np.array_equal(half, (blocks + 2) // 4)
    flat = np.full((9, 14, 3), 77, np.int64)
    for size in ((5, 7), (14, 4), (31, 23), (1, 1)):                              # non-uniform, upscale: a constant stays constant
        assert (rp.resample(flat, *size) == 77).all()
    up = rp.resample(cv, 40, 24)
    assert np.array_equal(up[0, 0], cv[0, 0]) and np.array_equal(up[-1, -1], cv[-1, -1])       # the border clamps
    assert np.array_equal(up[1, 1], (9 * cv[0, 0] + 3 * cv[0, 1] + 3 * cv[1, 0] + cv[1, 1] + 8) // 16)
    ramp = np.repeat(np.arange(0, 200, 10)[None, :, None], 12, 0).repeat(3, 2).astype(np.int64)
    assert (np.diff(rp.resample(ramp, 33, 5)[:, :, 0].astype(int), axis=1) >= 0).all()         # monotone in, monotone out
    # 7680 x 5400 -> 3840 x 2160, the largest sizes the bench uses: every intermediate of the rule fits int64
    OW, OH, CW, CH = 3840, 2160, 7680, 5400
    assert 4 * OW * OH * 255 + 2 * OW * OH < 2 ** 63 and (2 * OW + 1) * CW < 2 ** 63
    x0, x1, w0, w1 = (np.asarray(v) for v in rp.axis_taps(OW, CW))
    assert (w0 + w1 == 2 * OW).all() and (w0 >= 0).all() and (w1 >= 0).all() and x1.max() == CW - 1 and x0.min() == 0
    assert (x0 == 2 * np.arange(OW)).all() and (w1 == OW).all()                   # exact 2:1 again: equal weights


def test_compose_layers_and_layout():
    frames = np.random.RandomState(2).randint(0, 256, (3, 5, 6, 3)).astype(np.uint8)
    mask = np.zeros((3, 5, 6), np.uint16)
    assert np.array_equal(rp.compose(frames, mask)[:5, :6], frames[0]) and np.array_equal(rp.compose(frames, mask)[5:, :6], frames[1])
    assert np.array_equal(rp.compose(frames, mask)[:5, 6:], frames[2]) and (rp.compose(frames, mask)[5:, 6:] == 0).all()
    assert np.array_equal(rp.compose(frames, mask, swap_rb=True)[:5, :6], frames[0][..., ::-1])
    mask[0, 0, :4] = [1, 2, 4, 8]
    mask[0, 1, :3] = [3, 5, 15]
    px = rp.compose(frames, mask)
    v = frames[0].astype(np.int64)
    assert px[0, 0].tolist() == [0, 0, 255] and px[0, 1].tolist() == [0, 255, 0] and px[0, 3].tolist() == [0, 0, 0]
    assert px[0, 2].tolist() == ((7 * v[0, 2] + 770) // 10).tolist()
    assert px[1, 0].tolist() == [0, 255, 0] and px[1, 1].tolist() == [77, 77, 255] and px[1, 2].tolist() == [0, 0, 0]
    assert [rp.layout(n) for n in (1, 2, 3, 5, 6, 18)] == [(1, 1), (1, 2), (2, 2), (2, 3), (2, 3), (4, 5)]
    assert [rp.tile_of(i, 5) for i in range(5)] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]


def test_window_sum_and_running_frame():
    stamps, frames = rp.integrity_case()
    a, b = frames[0], frames[1]
    y0, y1, x0, x1 = rp.window(*a.shape[:2])
    count = (y1 - y0) * (x1 - x0) * 3
    assert count > 0 and rp.absdiff(a, b) / count == np.mean(np.abs(a[100:500, 100:500].astype(float) - b[100:500, 100:500].astype(float)))
    assert rp.absdiff(a[:50], b[:50]) == 0 and not rp.doubled(a[:50], a[:50])    # an empty window is never doubled
    assert rp.integrity(stamps, frames) == dict(doubled_ts=1, doubled_frame=1, doubled_both=1, skipped_ts=1,
                                                correct=len(stamps) - 1 - 4 - 8)
    r = rp.running(frames[:3])
    assert r[0].dtype == np.float64 and np.array_equal(r[0], frames[0]) and np.array_equal(r[2], 0.95 * (0.95 * r[0] + 0.05 * frames[1]) + 0.05 * frames[2])


def test_interface_without_a_gpu(tmp_path):
    import torch
    import datareader
    import mc3d_render
    from retinanet_mi355x import _hip, ops, torch_ops
    for name in ("replay_boxes", "replay_compose", "frame_absdiff", "running_frame"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
        assert ("rn_" + name) in _hip.SIGNATURES
    assert ops.REPLAY_BITS == rp.BIT and mc3d_render.REPLAY_THICKNESS == rp.THICKNESS
    assert [ops.replay_layout(n) for n in (1, 2, 3, 5, 6, 18)] == [rp.layout(n) for n in (1, 2, 3, 5, 6, 18)]
    assert ops.absdiff_window(600, 520) == 400 * 400 * 3 and ops.absdiff_window(104, 108) == 4 * 8 * 3 and ops.absdiff_window(50, 900) == 0
    st = torch.zeros(3, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.replay_boxes(st, torch.zeros(2, dtype=torch.float64), torch.zeros(2, 3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.replay_compose(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_absdiff(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.running_frame(torch.zeros(4, 4, 3, dtype=torch.float64), torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.retinanet_mi355x.frame_absdiff(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, 3, dtype=torch.uint8), 0, 4, 0, 4)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")         # noqa: E731
        out = torch.ops.retinanet_mi355x.replay_boxes(e(9, 7, dtype=torch.float32), e(3, dtype=torch.float64), e(3, 3, 4, dtype=torch.float64),
                                                      None, 2, 5)
        assert [tuple(t.shape) for t in out] == [(15, 7), (15, 8, 2), (15,), (15,)]
        img = torch.ops.retinanet_mi355x.replay_compose(e(3, 8, 8, 3, dtype=torch.uint8), e(3, 8, 8, dtype=torch.uint16), 10, 6, False)
        assert tuple(img.shape) == (6, 10, 3) and img.dtype == torch.uint8
    # signatures, as the issue's public surface states them
    sig = inspect.signature(datareader.Camera_Wrapper.__init__).parameters
    assert list(sig)[:4] == ["self", "source", "ds", "reader"] and sig["ds"].default == 2 and sig["reader"].default is None
    assert "self" in inspect.signature(datareader.Camera_Wrapper.skip).parameters
    sig = inspect.signature(datareader.test_integrity).parameters
    assert list(sig)[:3] == ["source", "n", "save_dir"] and sig["n"].default == 1000 and sig["save_dir"].default is None
    sig = inspect.signature(datareader.Data_Reader.plot_in).parameters
    assert list(sig) == ["self", "sequences", "framerate", "savefile", "render"] and sig["framerate"].default == 10
    assert "painted by the replay" in datareader.Data_Reader.plot_labels.__doc__
    # refusals: what is cv2 itself, and the replay without a device
    path = os.path.join(str(tmp_path), "in.csv")
    with open(path, "w", newline="") as f:
        f.write(dc.tracking_csv(**rp.GOLDEN_CSV))
    dr = datareader.Data_Reader(path, None)
    render = {"out": None, "size": None, "max_frames": 1}
    with pytest.raises(NotImplementedError, match="cv2"):
        dr.plot_in([], savefile="out.avi", render=render)
    with pytest.raises(NotImplementedError, match="cv2"):
        dr.plot_in([])

    class Loader:
        sequence = "somewhere/p1c1_0.mp4"

        def __next__(self):
            return np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="TimestampReader"):
        datareader.Camera_Wrapper(Loader())
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dr.plot_in([Loader()], render=dict(render, sets=[]))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            datareader.Camera_Wrapper(Loader(), reader=object())
    # the label records carry the replay's bit numbers, the tracker's stay as they were
    labels = [(0, 0, ["ab", "c"]), (1, 1, ["xyz"])]
    rects, runs, text = mc3d_render.label_records(labels, ops.REPLAY_BITS)
    assert (rects[:, 7] == rp.BIT["label"]).all() and (runs[:, 6] == rp.BIT["label_text"]).all()
    rects0, runs0, text0 = mc3d_render.label_records(labels)
    assert (rects0[:, 7] == rc.BIT["label"]).all() and (runs0[:, 6] == rc.BIT["label_text"]).all() and bytes(text) == bytes(text0)
    assert np.array_equal(rects[:, :7], rects0[:, :7])
    assert mc3d_render.replay_label_lines(np.array([1, 2, 17.25, 6.049999, 5.5, 1, 80], np.float32), "van", 104, np.float64(12.5)) == \
        rp.label_lines(np.array([1, 2, 17.25, 6.049999, 5.5, 1, 80], np.float32), "van", 104, np.float64(12.5)) == \
        ["van 104:", "L: 17.2ft", "W: 6.0ft", "H: 5.5ft", "12.5"]

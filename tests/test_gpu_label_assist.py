"""GPU: csrc/label_assist.hip (ops.label_fit_box2d / label_best_anchor / label_crop_windows) and the public label_assist
functions on top of it, against the restatement of tests/label_assist_cases.py and the reference's own output
(tests/golden/label_assist.npz).  Reads nothing of the reference.

Device against restatement is compared BIT FOR BIT -- centre, error, every round's index, the best anchor's box, the crop
window: the kernels' arithmetic is the restatement's, float32 with one rounding per operation (float64 inside state_to_im), so
there is no tolerance to choose.  Device against the reference: tools/make_golden_label_assist.py found the restatement's
errors bit-equal to the reference's on every candidate, so indices, errors and centres are compared exactly too.

Shapes: 0, 1, 4, 5, 63, 64 and 65 boxes (one wave per box, four waves per block), grids of 2 (4 candidates, 60 idle lanes), 8
(exactly one pass), 11 (a second pass with 7 idle lanes) and 16 (four full passes), one round and three; 1, 63, 64, 65 and 2 394
anchors; 255, 256 and 257 crop windows (one thread per box, 256 per block)."""

import numpy as np
import pytest
import torch

import label_assist_cases as ac

pytestmark = pytest.mark.gpu
F32 = np.float32
SCENES = ac.golden_scenes()


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same(a, b):
    """bit_equal, but a NaN is a NaN whatever its bits (a box that was left out)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        bit_equal(np.where(np.isnan(a), F32(0), a), np.where(np.isnan(b), F32(0), b))


def up(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def fit_on_device(dev, tmpl, cam, centre, target, P1, P2, rads, grid, skip=None):
    from retinanet_mi355x import ops
    got = ops.label_fit_box2d(up(dev, tmpl), up(dev, np.asarray(cam, np.int32)), up(dev, centre), up(dev, target), up(dev, P1),
                              up(dev, P2), up(dev, np.array(rads, np.float64)), grid, skip=up(dev, skip))
    return [t.cpu().numpy() for t in got]


def fit_same_as_restatement(dev, tmpl, cam, centre, target, P1, P2, rads=None, grid=ac.GRID, status=0):
    rads = ac.radii() if rads is None else rads
    out, err, idx, st = fit_on_device(dev, tmpl, cam, centre, target, P1, P2, rads, grid)
    w_out, w_err, w_idx, w_status, every = ac.fit_boxes(tmpl, cam, centre, target, P1, P2, rads, grid)
    assert int(st[0]) == status == w_status
    assert out.dtype == err.dtype == np.float32 and bit_equal(idx, w_idx) and same(out, w_out) and same(err, w_err)
    return out, err, idx, every


@pytest.mark.parametrize("grid,rounds", [(11, 3), (2, 3), (8, 1), (16, 3), (11, 1)])
@pytest.mark.parametrize("n", [0, 1, 4, 5, 63, 64, 65])
def test_fit_equals_the_restatement_bit_for_bit(dev, n, grid, rounds):
    args = ac.fuzz_fit(n, seed=10 * n + grid)
    out, err, idx, _ = fit_same_as_restatement(dev, *args, rads=ac.radii()[:rounds], grid=grid)
    assert idx.shape == (n, rounds) and out.shape == (n, 2)
    if n:
        assert idx.min() >= 0 and idx.max() < grid * grid and np.isfinite(err).all()
    if n >= 63:
        assert len(set(args[1].tolist())) == 4 and len(set(idx[:, 0].tolist())) > 1 and (np.abs(out - args[2]) > 0).any()
        assert idx.max() >= 64 or grid <= 8                     # winners of the second pass


def test_fit_at_the_wrapper_switch(dev):
    """Centres at y = 60 +/- 1 and on it: the corner-0 y of the candidates lies on both sides, the two matrices differ."""
    tmpl, cam, centre, target, P1, P2 = ac.fuzz_fit(12, seed=5, near_switch=True)
    centre[:, 1] = np.tile(np.array([59.0, 60.0, 61.0], F32), 4)
    out, _, idx, _ = fit_same_as_restatement(dev, tmpl, cam, centre, target, P1, P2)
    one, _, _, _ = fit_same_as_restatement(dev, tmpl, cam, centre, target, P1, None)
    two, _, _, _ = fit_same_as_restatement(dev, tmpl, cam, centre, target, P2, None)
    assert not bit_equal(P1, P2) and not bit_equal(one, two)
    assert not bit_equal(out, one) and not bit_equal(out, two)                  # the wrapper is neither side alone


def test_equal_errors_go_to_the_lower_index(dev):
    tmpl, cam, centre, target, P1, P2 = ac.fuzz_fit(9, seed=3)
    P1[:, [1, 5, 9]] = 0.0                                      # the image ignores y: the candidates of one ix tie
    out, err, idx, every = fit_same_as_restatement(dev, tmpl, cam, centre, target, P1, None)
    e = every[0][0].reshape(ac.GRID, ac.GRID)
    assert (e == e[:, :1]).all() and (idx % ac.GRID == 0).all()
    assert bit_equal(out[:, 1], ((centre[:, 1] - F32(50)) - F32(10)) - F32(2))


def test_a_bad_camera_and_an_error_that_is_not_finite_leave_their_box_out(dev):
    tmpl, cam, centre, target, P1, P2 = ac.fuzz_fit(11, seed=6)
    clean = fit_same_as_restatement(dev, tmpl, cam, centre, target, P1, P2)
    cam2, target2, centre2 = cam.copy(), target.copy(), centre.copy()
    cam2[2], cam2[7] = -1, 4
    out, err, idx, _ = fit_same_as_restatement(dev, tmpl, cam2, centre, target, P1, P2, status=ac.BAD_CAMERA)
    keep = np.array([i not in (2, 7) for i in range(11)])
    assert np.isnan(out[~keep]).all() and np.isnan(err[~keep]).all() and (idx[~keep] == -1).all()
    assert bit_equal(out[keep], clean[0][keep]) and bit_equal(err[keep], clean[1][keep]) and bit_equal(idx[keep], clean[2][keep])
    target2[4, 1] = np.nan                                      # every candidate's error is NaN
    centre2[9, 0] = np.inf                                      # inf - inf in the grid
    out, err, idx, _ = fit_same_as_restatement(dev, tmpl, cam, centre2, target2, P1, P2, status=ac.BAD_ERROR)
    keep = np.array([i not in (4, 9) for i in range(11)])
    assert np.isnan(out[~keep]).all() and np.isnan(err[~keep]).all() and (idx[~keep] == -1).all()
    assert bit_equal(out[keep], clean[0][keep]) and bit_equal(idx[keep], clean[2][keep])
    out, err, idx, _ = fit_same_as_restatement(dev, tmpl, cam2, centre2, target2, P1, P2, status=ac.BAD_CAMERA | ac.BAD_ERROR)
    # a skipped box is left out without a status bit, whatever it holds
    skip = np.zeros(11, np.uint8)
    skip[[2, 4, 7, 9]] = 1
    out, err, idx, st = fit_on_device(dev, tmpl, cam2, centre2, target2, P1, P2, ac.radii(), ac.GRID, skip=skip)
    keep = skip == 0
    assert int(st[0]) == 0 and np.isnan(out[~keep]).all() and (idx[~keep] == -1).all()
    assert bit_equal(out[keep], clean[0][keep]) and bit_equal(err[keep], clean[1][keep]) and bit_equal(idx[keep], clean[2][keep])


def test_fit_equals_the_reference(dev, golden, monkeypatch):
    """Every search of the golden script, with the inputs the restated replay hands to its own search."""
    g, scene = golden("label_assist"), SCENES["assist"]
    calls, plain = [], ac.fit_boxes

    def recording(*args, **kw):
        calls.append(([np.array(a) for a in args], plain(*args, **kw)))
        return calls[-1][1]
    monkeypatch.setattr(ac, "fit_boxes", recording)
    steps = ac.golden_script(scene)
    ac.replay(ac.Labels(scene), [s for s in steps if s[0] != "automate"], ac.RESTATED)
    n_paste = len(calls)
    ac.replay(ac.Labels(scene), steps, ac.RESTATED)
    calls = calls[:n_paste] + calls[2 * n_paste:]
    assert n_paste == len(g["assist_win"]) == 16 and len(calls) == 20
    for k, (args, want) in enumerate(calls):
        out, err, idx, st = fit_on_device(dev, *args, ac.radii(), ac.GRID)
        assert int(st[0]) == 0 and bit_equal(out, want[0]) and bit_equal(err, want[1]) and bit_equal(idx, want[2])
        if k < n_paste:                                         # the reference's own numbers
            assert bit_equal(idx[0].astype(np.int64), g["assist_win"][k]) and bit_equal(err[0], g["assist_err"][k, -1])
            assert bit_equal(out[0].astype(np.float64), g["assist_centre"][k])


def test_fit_refuses_what_it_cannot_take(dev):
    from retinanet_mi355x import ops
    tmpl, cam, centre, target, P1, P2 = (up(dev, a) for a in ac.fuzz_fit(3, seed=1))
    rads = up(dev, np.array(ac.radii(), np.float64))
    ok = ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads)
    assert int(ok[3]) == 0
    for bad in (lambda: ops.label_fit_box2d(tmpl.double(), cam, centre, target, P1, P2, rads),
                lambda: ops.label_fit_box2d(tmpl, cam.long(), centre, target, P1, P2, rads),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target.long(), P1, P2, rads),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target, P1.float(), P2, rads),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads.float()),
                lambda: ops.label_fit_box2d(tmpl[:, :3].contiguous(), cam, centre, target, P1, P2, rads),
                lambda: ops.label_fit_box2d(tmpl, cam[:2], centre, target, P1, P2, rads),
                lambda: ops.label_fit_box2d(tmpl, cam, centre[:2], target, P1, P2, rads),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2[:2], rads),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads, grid=1),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads, grid=17),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads.repeat(3)),
                lambda: ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads, skip=cam),
                lambda: ops.label_best_anchor(centre.reshape(3, 2, 1).double(), target.reshape(3, 1, 4), tmpl[:, :3].contiguous()),
                lambda: ops.label_best_anchor(centre.reshape(3, 2, 1), target.reshape(3, 1, 4), tmpl[:, :3].contiguous()),
                lambda: ops.label_best_anchor(centre.reshape(3, 2, 1)[:, :0], target.reshape(3, 1, 4)[:, :0], tmpl[:, :3].contiguous()),
                lambda: ops.label_crop_windows(target, cam, P1, P2),
                lambda: ops.label_crop_windows(torch.cat((centre, tmpl), 1).double(), cam, P1, P2),
                lambda: ops.label_crop_windows(torch.cat((centre, tmpl), 1), cam[:1], P1, P2)):
        with pytest.raises(RuntimeError):
            bad()


def test_the_registered_operators_are_the_ops(dev):
    from retinanet_mi355x import ops, torch_ops  # noqa: F401
    t = torch.ops.retinanet_mi355x
    tmpl, cam, centre, target, P1, P2 = (up(dev, a) for a in ac.fuzz_fit(6, seed=2))
    rads = up(dev, np.array(ac.radii(), np.float64))
    state = torch.cat((centre, tmpl), 1).contiguous()
    a, b = t.label_crop_windows(state, cam, P1, P2, 1.2, 1920.0, 1080.0), ops.label_crop_windows(state, cam, P1, P2)
    assert all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:3], b[:3])) and torch.equal(a[3], b[3])
    a = t.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads, 11, a[3])
    b = ops.label_fit_box2d(tmpl, cam, centre, target, P1, P2, rads, skip=b[3])
    assert all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:2], b[:2])) and torch.equal(a[2], b[2]) and int(a[3]) == 0
    cls, reg, win = (up(dev, x) for x in ac.fuzz_detector(3, 70, 8, seed=4))
    assert all(torch.equal(x, y) for x, y in zip(t.label_best_anchor(cls, reg, win, 112.0), ops.label_best_anchor(cls, reg, win)))


# ------------------------------------------------------------------------------------------------ the best anchor
@pytest.mark.parametrize("name", sorted(ac.anchor_edge_cases()))
def test_best_anchor_equals_the_restatement_bit_for_bit(dev, name):
    from retinanet_mi355x import ops
    cls, reg, win = ac.anchor_edge_cases()[name]
    got = [t.cpu().numpy() for t in ops.label_best_anchor(up(dev, cls), up(dev, reg), up(dev, win), 112)]
    want = ac.best_anchor(cls, reg, win, 112)
    assert [g.dtype for g in got] == [np.float32, np.int32, np.float32, np.int32]
    assert bit_equal(got[1], want[1]) and bit_equal(got[3], want[3]) and same(got[0], want[0]) and same(got[2], want[2])
    if name == "edges":
        assert got[1].tolist() == [129, 5, 0, 77, 9] and np.isnan(got[2][3])


# ------------------------------------------------------------------------------------------------ the crop windows
def windows_same_as_restatement(dev, state, cam, P1, P2, status=0, **kw):
    from retinanet_mi355x import ops
    got = [t.cpu().numpy() for t in ops.label_crop_windows(up(dev, state), up(dev, np.asarray(cam, np.int32)), up(dev, P1),
                                                           up(dev, P2), **kw)]
    want = ac.crop_windows(state, cam, P1, P2, **kw)
    assert int(got[4][0]) == status == want[4] and bit_equal(got[3], want[3])
    assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2])
    return got


def test_each_edge_test_on_its_bound_and_one_ulp_past_it(dev):
    """A camera whose pixels are the road's feet (u = x, v = y), so the extent is the state's own float32 numbers."""
    P = np.array([[1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 1.0]], np.float64)
    tiny = np.nextafter(F32(0), F32(-1))
    rows = [(0.0, 10.0, 20.0, 0.0, 5.0, 1.0), (tiny, 10.0, 20.0, 0.0, 5.0, 1.0),                    # x1 = x
            (10.0, 0.0, 20.0, 0.0, 5.0, 1.0), (10.0, tiny, 20.0, 0.0, 5.0, 1.0),                    # y1 = y (no width)
            (1920.0, 10.0, 20.0, 0.0, 5.0, -1.0), (np.nextafter(F32(1920), F32(2000)), 10.0, 20.0, 0.0, 5.0, -1.0),     # x2 = x
            (10.0, 1080.0, 20.0, 0.0, 5.0, 1.0), (10.0, np.nextafter(F32(1080), F32(2000)), 20.0, 0.0, 5.0, 1.0),      # y2 = y
            (100.0, 100.0, 20.0, 30.0, 5.0, 1.0), (100.0, 100.0, 20.0, 10.0, 5.0, -1.0)]            # h > w and w > h
    state = np.array(rows, F32)
    crop, rois, win, skipped, _ = windows_same_as_restatement(dev, state, np.zeros(len(rows), np.int32), P, None)
    assert skipped.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 0]
    assert bit_equal(crop[1], np.array([tiny, 10, 20, 10], F32)) and np.isnan(rois[1]).all() and np.isnan(win[1]).all()
    assert win[8, 2] == F32(30) * F32(1.2) and win[9, 2] == F32(20) * F32(1.2)
    small = windows_same_as_restatement(dev, state, np.zeros(len(rows), np.int32), P, None, ber=1.5, width=96, height=64)
    assert small[3].tolist() == [0, 1, 0, 1, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_crop_windows_equal_the_restatement_bit_for_bit(dev, n):
    rng = np.random.RandomState(n)
    tmpl, cam, centre, _, P1, P2 = ac.fuzz_fit(n, seed=20 + n)
    centre[:, 0] += rng.uniform(-60, 60, n).astype(F32)         # some leave their camera's frame
    state = np.concatenate([centre, tmpl], axis=1).astype(F32)
    got = windows_same_as_restatement(dev, state, cam, P1, P2)
    if n >= 255:
        assert 0 < got[3].sum() < n
        cam2 = cam.copy()
        cam2[[3, n - 1]] = [4, -1]
        bad = windows_same_as_restatement(dev, state, cam2, P1, P2, status=ac.BAD_CAMERA)
        assert bad[3][3] == 1 and bad[3][n - 1] == 1 and np.isnan(bad[0][3]).all()
        windows_same_as_restatement(dev, state, cam, P1, None)


# ------------------------------------------------------------------------------------------------ the public functions
class Scripted():
    """A stand-in for the localiser: hands out the scene's scripted LOCALIZE outputs in the order the crops arrive and keeps
    the crops it was given."""

    def __init__(self, scene, keys, dev):
        self.queue = [scene["script"][k] for k in keys]
        self.dev, self.crops, self.training = dev, [], True

    def eval(self):
        self.training = False

    def __call__(self, crops, LOCALIZE=False):
        assert LOCALIZE and not self.training and crops.dtype == torch.float32 and crops.is_cuda
        n = crops.shape[0]
        take, self.queue = self.queue[:n], self.queue[n:]
        assert len(take) == n
        self.crops.append(crops.cpu().numpy())
        reg, cls = (torch.from_numpy(np.stack([pair[k] for pair in take])).to(self.dev) for k in (0, 1))
        return reg, cls


@pytest.fixture(scope="module")
def Me(dev):
    import label_assist as la

    class Me(ac.Labels, la.LabelAssist):
        pass
    return Me


def test_the_public_functions_equal_the_reference(dev, Me, golden):
    """The golden script through box_to_state, find_box, copy_paste and paste_in_2D_bbox on the device; automate with the
    script's 2D box in place of the detector.  Every array of the golden file, data included, bit for bit."""
    g, scene = golden("label_assist"), SCENES["assist"]

    def automate(me, oid, detect):
        me.crop_detect = lambda frame, crop, ber=1.2, cs=112: torch.from_numpy(detect(None, np.asarray(crop, F32)))
        return me.automate(oid)
    ops = {"box_to_state": lambda me, p: me.box_to_state(p).numpy(), "find_box": lambda me, p: me.find_box(p),
           "copy_paste": lambda me, p: me.copy_paste(p), "paste2d": lambda me, b: me.paste_in_2D_bbox(b), "automate": automate}
    got = ac.replay(Me(scene), ac.golden_script(scene), ops)
    for k in ("b2s", "found", "centre", "auto_box", "auto_skip", "data_idx", "data_val"):
        assert bit_equal(got[k], g["assist_" + k]), k


def test_automate_many_equals_key_by_key_equals_the_restatement(dev, Me):
    from oracle import crop_refine as ocr
    import label_assist as la
    scene = ac.small_scene()
    keys, cs, names = scene["keys"], scene["cs"], scene["names"]
    want_me = ac.Labels(scene)
    want = ac.ref_automate_keys(want_me, scene, keys)
    # key by key: a click copies the box, automate crops, localises and fits it
    one = Me(scene)
    one.detector = Scripted(scene, [k for k in keys if not want[k]["skipped"]], dev)
    one.buffer = [[(scene["frames"][c],) for c in range(3)]]
    single = {}
    for key in keys:
        o = one.data[0][key]
        one.active_cam, one.clicked_camera, one.copied_box = names.index(o["camera"]), o["camera"], None
        p = ac.image_point(one, o["camera"], o["x"], o["y"])
        one.copy_paste(np.array([p[0], p[1], p[0] + 3, p[1] + 2], np.int64))
        assert one.copied_box[0] == o["id"]
        single[key] = one.automate(o["id"], cs=cs)
    # the batch, frames as a dict of host arrays and as one device tensor
    for frames in ({n: scene["frames"][c] for c, n in enumerate(names)}, torch.from_numpy(scene["frames"]).to(dev)):
        many = Me(scene)
        many.detector = Scripted(scene, keys, dev)
        batch = many.automate_many(keys, frames, cs=cs)
        assert many.data == one.data == want_me.data
        for key in keys:
            for res in (batch[key], single[key]):
                assert res["skipped"] == want[key]["skipped"] and bit_equal(res["crop_box"], want[key]["crop_box"])
                assert res["box_2D"] is None if res["skipped"] else bit_equal(res["box_2D"], want[key]["box_2D"])
        assert all(type(d["x"]) is float and type(d["y"]) is float for d in many.data[0].values())
    # the crops the detector saw: to_tensor, roi_align, normalize, against the oracle's restated roi_align
    state = np.array([[scene["data"][0][k][s] for s in ac.STATE_KEYS] for k in keys], F32)
    cam = np.array([names.index(scene["data"][0][k]["camera"]) for k in keys], np.int32)
    P1, P2 = ac.tables(want_me.hg, names)
    _, rois, _, skipped, _ = ac.crop_windows(state, cam, P1, P2)
    tensor = (scene["frames"].astype(F32) / F32(255)).transpose(0, 3, 1, 2)
    crops = ocr.roi_align(np.ascontiguousarray(tensor), np.where(np.isnan(rois), F32(0), rois), (cs, cs))
    mean, std = np.array(la.MEAN, F32).reshape(1, 3, 1, 1), np.array(la.STD, F32).reshape(1, 3, 1, 1)
    crops = ((crops.numpy() if torch.is_tensor(crops) else np.asarray(crops, F32)) - mean) / std
    seen = many.detector.crops
    assert len(seen) == 1 and seen[0].shape == (len(keys), 3, cs, cs)
    keep = skipped == 0
    assert bit_equal(seen[0][keep], crops[keep].astype(F32)) and (seen[0][~keep] == ((0 - mean) / std)).all()
    assert bit_equal(np.concatenate(one.detector.crops), seen[0][keep])


def test_crop_detect_composes_with_the_2d_localiser(dev, Me):
    """The project's own 2D ResNet-50 at cs = 112 on one crop: shapes, finite output, a box inside the frame."""
    from retinanet_mi355x import modules
    torch.manual_seed(0)
    me = Me(SCENES["assist"])
    me.detector = modules.resnet50(num_classes=8, directional=False).to(dev)
    seen = {}
    plain = me.detector.forward

    def forward(x, LOCALIZE=False):
        seen["in"] = tuple(x.shape)
        seen["out"] = plain(x, LOCALIZE=LOCALIZE)
        return seen["out"]
    me.detector.forward = forward
    frame = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (1080, 1920, 3)).astype(np.uint8)).to(dev)
    box = me.crop_detect(frame, np.array([700, 400, 900, 520], F32))
    reg, cls = seen["out"]
    assert seen["in"] == (1, 3, 112, 112) and tuple(reg.shape) == (1, 2394, 4) and tuple(cls.shape) == (1, 2394, 8)
    assert not me.detector.training and box.dtype == torch.float32 and tuple(box.shape) == (4,) and not box.is_cuda
    assert torch.isfinite(box).all() and torch.isfinite(reg).all() and torch.isfinite(cls).all()
    assert 0 <= box[0] <= box[2] <= 1920 and 0 <= box[1] <= box[3] <= 1080
    lo, hi = 800 - 120, 800 + 120                               # the window: 240 square about (800, 460)
    assert lo <= box[0] and box[2] <= hi and 460 - 120 <= box[1] and box[3] <= 460 + 120

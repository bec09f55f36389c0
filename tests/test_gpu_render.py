"""GPU: csrc/render.hip and mc3d_render.py against the plain restatement of tests/render_cases.py -- exact uint16 / uint8
equality everywhere -- and the tracker of tests/tracker_cases.py run with ``params["render"]``."""
import os

import numpy as np
import pytest
import torch

import render_cases as rc
import tracker_cases as trc

pytestmark = pytest.mark.gpu


def _mask(ops, dev, shape):
    return ops.render_mask(*shape, dev)


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _font(dev):
    from mc3d_render import FONT
    return FONT, torch.from_numpy(FONT).to(dev)


def _same(got, want):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_edges(dev, thickness):
    from retinanet_mi355x import ops
    corners, cam = rc.edges_case()
    mask = _mask(ops, dev, rc.EDGE_SHAPE)
    ops.render_edges(_t(corners, dev), _t(cam, dev), thickness, 2, mask)
    ops.render_edges(_t(corners[:3], dev), _t(cam[:3], dev), 1, 11, mask)               # a second layer ORs in
    want = rc.paint_edges(rc.new_mask(*rc.EDGE_SHAPE), corners, cam, thickness, 2)
    want = rc.paint_edges(want, corners[:3], cam[:3], 1, 11)
    assert want[0].any() and want[2].any() and not want[1].any()                       # camera 1 receives nothing
    _same(mask, want)


def test_rects(dev):
    from retinanet_mi355x import ops
    rects, anchors = rc.rects_case()
    mask = _mask(ops, dev, rc.EDGE_SHAPE)
    ops.render_rects(_t(rects, dev), mask, _t(anchors, dev))
    want = rc.paint_rects(rc.new_mask(*rc.EDGE_SHAPE), rects, anchors)
    assert all((want >> b & 1).any() for b in (0, 1, 4, 5, 6, 7, 15)) and not (want >> 3 & 1).any()      # bit 3: no such camera
    _same(mask, want)
    ops.render_rects(_t(rects[:0], dev), mask)                                          # nothing to draw, no anchors
    _same(mask, want)


def test_text(dev):
    from retinanet_mi355x import ops
    font, d_font = _font(dev)
    runs, text, anchors = rc.text_case()
    mask = _mask(ops, dev, rc.TEXT_SHAPE)
    ops.render_text(_t(runs, dev), _t(text, dev), d_font, mask, _t(anchors, dev))
    want = rc.paint_text(rc.new_mask(*rc.TEXT_SHAPE), runs, text, font, anchors)
    assert all((want >> b & 1).any() for b in (6, 7, 8, 9)) and not (want >> 10 & 1).any()
    _same(mask, want)


@pytest.mark.parametrize("shape", [(2, 16, 35), (1, 9, 64), (3, 37, 67)])
@pytest.mark.parametrize("crops_present", [False, True])
def test_compose_every_mask(dev, shape, crops_present):
    from retinanet_mi355x import ops
    from mc3d_render import mosaic_layout
    frames, m = rc.random_frames(*shape, seed=11), rc.all_masks(*shape, seed=12)
    mask = _mask(ops, dev, shape)
    mask.copy_(_t(m, dev))
    cols = mosaic_layout(shape[0])[1]
    _same(ops.render_compose(_t(frames, dev), mask, crops_present, cols), rc.compose(frames, m, crops_present, cols))


def test_compose_empty_mask_gives_the_bytes_back(dev):
    """Three cameras -> a 2x2 canvas whose fourth tile is zero; every byte value in every channel."""
    from retinanet_mi355x import ops
    n, H, W = rc.EDGE_SHAPE
    u8 = np.random.RandomState(5).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    u8[0, 0, :, 0], u8[1, 1, :64, 1], u8[2, 2, :, 2] = np.arange(W), np.arange(64) * 4 + 3, 255 - np.arange(W)
    u8[0, 3:7, :64, :] = np.arange(256, dtype=np.uint8).reshape(4, 64, 1)
    frames = ops.frame_ingest(_t(u8, dev))
    out = ops.render_compose(frames, _mask(ops, dev, rc.EDGE_SHAPE), False, 2).cpu().numpy()
    assert out.shape == (2 * H, 2 * W, 3)
    for i in range(n):
        assert np.array_equal(out[(i // 2) * H:(i // 2 + 1) * H, (i % 2) * W:(i % 2 + 1) * W], u8[i]), i
    assert not out[H:, W:].any()


def _scene(dev, shape, seed):
    """Arguments of Renderer.render for a busy frame, as numpy."""
    n, H, W = shape
    rs = np.random.RandomState(seed)

    def boxes(k):
        c = np.stack((rs.uniform(0, W, k), rs.uniform(0, H, k)), 1)[:, None, :]
        return c + rs.uniform(-9, 9, (k, 8, 2)), rs.randint(0, n, k).astype(np.int32)
    tracks, dets, priors = boxes(5), boxes(4), boxes(2)
    crops = (np.stack((rs.uniform(-5, W - 20, 3), rs.uniform(-5, H - 12, 3), rs.uniform(10, W + 9, 3), rs.uniform(8, H + 9, 3)), 1),
             rs.randint(0, n, 3).astype(np.int64))
    labels = [(i, int(tracks[1][i]), ["car %d:" % i, "61.5mph EB", "L: 16.2ft"][:1 + i % 3]) for i in range(5)]
    banners = ["Estimated time bias: %.4fs (%.1fft)" % (0.01 * c, 0.8 * c) for c in range(n)]
    return dict(frames=rc.random_frames(n, H, W, seed + 1), tracks=tracks, detections=dets, priors=priors, crops=crops, labels=labels,
                banners=banners)


def _render(r, dev, sc, **kw):
    pair = lambda p: None if p is None else (_t(p[0], dev), _t(p[1], dev))               # noqa: E731
    return r.render(_t(sc["frames"], dev), pair(sc["tracks"]), pair(sc["detections"]), pair(sc["priors"]), pair(sc["crops"]),
                    sc["labels"], sc["banners"], **kw)


@pytest.mark.parametrize("fancy_crop", [True, False])
def test_renderer_against_the_restatement_and_itself(dev, fancy_crop):
    from mc3d_render import FONT, Renderer
    shape = (3, 64, 96)
    sc = _scene(dev, shape, seed=21)
    r = Renderer(*shape, dev)
    first = _render(r, dev, sc, fancy_crop=fancy_crop).clone()
    second = _render(r, dev, sc, fancy_crop=fancy_crop)
    assert torch.equal(first, second)                                                   # identical calls, identical bytes
    want, want_mask = rc.render_restated(*shape, FONT, **sc, fancy_crop=fancy_crop)
    _same(r.mask, want_mask)
    _same(second, want)
    assert all((want_mask >> rc.BIT[k] & 1).any() for k in ("prior", "track", "det", "label", "label_text", "banner_edge", "banner_text",
                                                             "in_crop" if fancy_crop else "crop_edge"))
    for view, i in zip(r.views(), range(3)):
        assert torch.equal(view, second[(i // 2) * 64:(i // 2 + 1) * 64, (i % 2) * 96:(i % 2 + 1) * 96])


def test_beyond_one_block(dev):
    """One camera of 130x515: a thickness-3 edge along the whole diagonal and a 300-character run."""
    from retinanet_mi355x import ops
    font, d_font = _font(dev)
    shape = (1, 130, 515)
    box = np.array([[[0.0, 0.0], [514.0, 129.0]] + [[0.0, 0.0]] * 6])
    text = np.frombuffer(bytes(32 + (7 * i) % 95 for i in range(300)), np.uint8)
    runs = np.array([[-700, 70, 0, -1, 1, 1, 6, 0, 300], [3, 120, 0, -1, 2, 0, 8, 0, 300]], np.int32)
    mask = _mask(ops, dev, shape)
    ops.render_edges(_t(box, dev), _t(np.zeros(1, np.int32), dev), 3, 2, mask)
    ops.render_text(_t(runs, dev), _t(text, dev), d_font, mask)
    want = rc.paint_edges(rc.new_mask(*shape), box, [0], 3, 2)
    want = rc.paint_text(want, runs, text, font)
    assert (want[0, 0, :3] & 4).all() and (want[0, 129, 512:] & 4).all() and (want[0, 62:70, 500:] & 64).any()
    _same(mask, want)
    frames = rc.random_frames(*shape, seed=3)
    _same(ops.render_compose(_t(frames, dev), mask, True, 1), rc.compose(frames, want, True, 1))


def test_wrappers_refuse_what_the_kernels_cannot_take(dev):
    from retinanet_mi355x import ops, torch_ops  # noqa: F401  (registers torch.ops.retinanet_mi355x.*)
    mask = _mask(ops, dev, (1, 5, 7))
    odd = torch.zeros(35, dtype=torch.uint16, device=dev).view(1, 5, 7)              # no spare pixel behind an odd plane
    box, cam = torch.zeros((1, 8, 2), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for bad in (lambda: ops.render_edges(box, cam, 1, 2, odd), lambda: ops.render_edges(box.float(), cam, 1, 2, mask),
                lambda: ops.render_edges(box, cam.long(), 1, 2, mask), lambda: ops.render_edges(box, cam, 0, 2, mask),
                lambda: ops.render_edges(box, cam, 1, 16, mask), lambda: ops.render_rects(torch.zeros((1, 7), dtype=torch.int32, device=dev), mask),
                lambda: ops.render_compose(torch.zeros((1, 3, 5, 8), device=dev), mask, False, 1),
                lambda: ops.render_compose(torch.zeros((1, 3, 5, 7), device=dev), mask, False, 2)):
        with pytest.raises(RuntimeError):
            bad()
    torch.ops.retinanet_mi355x.render_edges(box + 2.0, cam, 1, 2, mask)
    got = mask.cpu().numpy()
    assert got[0, 2, 2] == 4 and int(got.astype(np.int64).sum()) == 4


# ------------------------------------------------------------------------------------------------ the tracker
def _run(dev, render=None, frame=None, **kw):
    from test_gpu_tracker_run import _tracker
    trk = _tracker(dev, params={} if render is None else dict(render=render), **kw)
    hw = trc.FRAME_HW
    if frame is not None:                                        # the scripted loaders hand out this frame instead of a blank one
        hw = tuple(frame.shape[1:])
        for loader in trk.loaders:
            loader.frame = frame
    shots = {}
    if render is not None:
        def hooked(*a, **k):
            """Render, then keep everything the frame's picture was made from (the filter has not moved yet)."""
            r = trk.renderer
            out = type(r).render_tracker(r, *a, **k)
            flt, per_cam = trk.filter, []
            for c in range(3):
                if flt.X is not None and len(flt.X):
                    per_cam.append(flt.view(with_direction=True, dt=flt.get_dt(float(trk.timestamps[c]) + float(trk.ts_bias[c])))[1].clone())
            shots[trk.frame_num] = dict(canvas=out.cpu().numpy(), last=dict(r.last), views_state=r.views_state.clone(), per_cam=per_cam,
                                        ims=[v.cpu().numpy() for v in trk.renderer.views()])
            return out
        import mc3d_render
        trk.renderer = mc3d_render.Renderer(3, *hw, dev)
        trk.renderer.render_tracker = hooked
    trk.track()
    return trk, shots


@pytest.fixture(scope="module")
def rendered_run(dev, tmp_path_factory):
    out = tmp_path_factory.mktemp("frames")
    return _run(dev, dict(out=str(out))) + (out,)


def test_tracker_is_unchanged_by_rendering(dev, rendered_run):
    plain, _ = _run(dev)
    trk = rendered_run[0]
    assert plain.renderer is None and plain.rendered is None and plain.time_metrics["plot"] < 0.01
    assert len(trk.records) == len(plain.records) == 14
    for a, b in zip(trk.records, plain.records):
        for k in trc.DISCRETE_KEYS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (a["frame_num"], k)
        for k in ("X", "P", "T", "ts_bias"):
            assert np.array_equal(a[k], b[k]), (a["frame_num"], k)                   # bit-equal
    assert all(torch.equal(x[2], y[2]) for x, y in zip(trk.all_tracks, plain.all_tracks))


def _numpy_args(last):
    def pair(p):
        return None if p is None else (p[0].cpu().numpy(), p[1].cpu().numpy())
    return dict(frames=last["frames"].cpu().numpy(), tracks=pair(last["tracks"]), detections=pair(last["detections"]),
                priors=pair(last["priors"]), crops=pair(last["crops"]), labels=last["labels"], banners=last["banners"],
                fancy_crop=last["fancy_crop"])


@pytest.mark.parametrize("kind", ["detection", "crop"])
def test_tracker_picture(dev, rendered_run, kind):
    import mc3d_post
    from mc3d_render import FONT
    from retinanet_mi355x import ops
    trk, shots, _ = rendered_run
    assert sorted(shots) == list(range(14)) and trk.renderer.copies == 14              # one copy per rendered frame
    f = max(k for k in shots if (k % 2 == 0) == (kind == "detection"))
    shot = shots[f]
    last = shot["last"]
    n = len(shot["per_cam"][0])
    assert n > 0 and last["tracks"][0].shape[0] == 3 * n and last["detections"] is not None
    assert (last["crops"] is not None) == (kind == "crop") and last["priors"] is None and len(last["labels"]) == 3 * n
    assert all(len(lines) == 5 for _, _, lines in last["labels"]) and all(b.startswith("Estimated time bias: ") and b.endswith("ft)") for b in last["banners"])
    # the corners are ops.hg_to_im of the filter viewed at each camera's stamp + bias
    assert torch.equal(shot["views_state"], torch.cat(shot["per_cam"]))
    _, _, P1, P2 = mc3d_post._camera_matrices(trk, dev)
    cam = torch.arange(3, dtype=torch.int32, device=dev).repeat_interleave(n)
    assert torch.equal(last["tracks"][0], ops.hg_to_im(shot["views_state"], P1, P2, cam)) and torch.equal(last["tracks"][1], cam)
    want, want_mask = rc.render_restated(3, *trc.FRAME_HW, FONT, **_numpy_args(last))
    c = last["tracks"][0].cpu().numpy()
    print("frame %d: layers %s; track corners x %.0f..%.0f y %.0f..%.0f" % (f, [k for k, b in rc.BIT.items() if (want_mask >> b & 1).any()],
                                                                           c[..., 0].min(), c[..., 0].max(), c[..., 1].min(), c[..., 1].max()))
    assert (want_mask & 128).any() and (want_mask & 256).any()
    assert np.array_equal(shot["canvas"], want)
    for i in range(3):
        assert np.array_equal(shot["ims"][i], want[(i // 2) * 64:(i // 2 + 1) * 64, (i % 2) * 96:(i % 2 + 1) * 96])
    if f == 13:
        assert np.array_equal(trk.rendered.cpu().numpy(), want) and len(trk.original_ims) == 3


def test_tracker_picture_at_camera_size(dev):
    """The scene's cameras are 1080p: on frames of that size the boxes, labels and crop windows land inside the picture (on
    the 64x96 frames of the scene only the banner does).  The first four frames; the last crop and detection frame checked."""
    from mc3d_render import FONT
    H, W = 1080, 1920
    frame = rc.random_frames(1, 4, W, seed=9)[0][:, :1, :].repeat(H, axis=1)          # vertical stripes: cheap and not blank
    trk, shots = _run(dev, dict(out=None, label_len=2), frame=_t(frame, dev), early_cutoff=3)
    assert sorted(shots) == [0, 1, 2, 3] and trk.renderer.copies == 4
    for f, layers in ((3, ("track", "det", "in_crop", "label", "label_text", "banner_text")), (2, ("track", "det", "label", "label_text"))):
        last = shots[f]["last"]
        want, want_mask = rc.render_restated(3, H, W, FONT, **_numpy_args(last))
        print("frame %d: pixels per layer %s" % (f, {k: int((want_mask >> b & 1).sum()) for k, b in rc.BIT.items()}))
        assert all((want_mask >> rc.BIT[k] & 1).any() for k in layers), f
        assert all(len(lines) == 2 for _, _, lines in last["labels"])
        assert np.array_equal(shots[f]["canvas"], want)


def test_boxes_sit_on_the_vehicles(rendered_run):
    """Frame 12 shows ten vehicles; G is oversized and never kept.  The true centre of at least six of them, projected into
    its camera at that camera's true time, falls within the image bounds of a track box drawn for that camera."""
    from oracle import homography as ohg
    trk, shots, _ = rendered_run
    shot = shots[12]
    corners, cam = (t.cpu().numpy() for t in shot["last"]["tracks"])
    P1, _, P2, _ = trc.camera_matrices()
    hits = 0
    for vi, veh in enumerate(trc.VEHICLES):
        if 12 not in veh[8]:
            continue
        rec = trk.records[12]
        c = trc.camera_of(trc.true_state(vi, rec["timestamps"][0])[0])
        st = np.array([trc.true_state(vi, rec["timestamps"][c] + trc.TRUE_BIAS[c])], np.float32)
        centre = ohg.wrapper_space_to_im(ohg.state_to_space(st), P1[[c]], P2[[c]])[0].mean(0)
        boxes = corners[cam == c]
        inside = (boxes[..., 0].min(1) <= centre[0]) & (centre[0] <= boxes[..., 0].max(1)) & \
                 (boxes[..., 1].min(1) <= centre[1]) & (centre[1] <= boxes[..., 1].max(1))
        hits += bool(inside.any())
    assert hits >= 6, hits


def test_png_frames(rendered_run):
    Image = pytest.importorskip("PIL.Image")
    trk, shots, out = rendered_run
    assert sorted(os.listdir(out)) == sorted(trc.CAMERAS + ["combined"])
    for name in trc.CAMERAS + ["combined"]:
        assert sorted(os.listdir(out / name)) == ["%05d.png" % f for f in range(14)]
    for f in (0, 13):
        assert np.array_equal(np.asarray(Image.open(out / "combined" / ("%05d.png" % f))), shots[f]["canvas"])
        for i, name in enumerate(trc.CAMERAS):
            assert np.array_equal(np.asarray(Image.open(out / name / ("%05d.png" % f))), shots[f]["ims"][i])

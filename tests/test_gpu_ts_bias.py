"""GPU: the per-camera time stamp bias (csrc/ts_bias.hip, ops.estimate_ts_bias, mc3d_track.estimate_ts_bias) against the
reference's own outputs in tests/golden/ts_bias.npz and against the numpy restatement in tests/ts_bias_cases.py.

Entry lists are compared exactly.  ts_bias is compared bit for bit wherever the two mean speeds do not depend on a
summation order (the fallback, or at most two tracks per direction).  Elsewhere the allowed difference is computed,
not chosen: ts_bias_cases.ulp_bound -- the largest change of the restatement's ts_bias when each mean speed is moved
one fp32 ulp up or down, times 2."""
import numpy as np
import pytest
import torch

import golden_cases as gc
import track_cases as tc
import ts_bias_cases as tb

pytestmark = pytest.mark.gpu


def _call(dev, c, max_pairs=None, bias=None, count=None):
    """-> (entries [e,4], time_error [e], ts_bias list, (pairs, status)) through ops."""
    from retinanet_mi355x import ops
    b = torch.tensor(c["ts_bias"] if bias is None else bias, dtype=torch.float64, device=dev)
    info, pairs, te = ops.estimate_ts_bias(
        torch.from_numpy(c["boxes"]).to(dev), torch.from_numpy(c["cams"]).to(dev), torch.from_numpy(c["objs"]).to(dev),
        torch.tensor(c["timestamps"], dtype=torch.float64, device=dev), b, c["phi"], tb.ALPHA, tb.MU_V, count=count,
        max_pairs=max_pairs, details=True)
    k, status = (int(x) for x in info.cpu())
    kk = min(k, len(pairs)) if status == 0 else 0
    p = pairs[:kk].cpu().numpy().astype(np.int64)
    cams = np.asarray(c["cams"])
    ent = np.zeros((2 * kk, 4), np.int64)
    if kk:
        ent[0::2] = np.stack((cams[p[:, 0]], cams[p[:, 1]], p[:, 0], p[:, 1]), 1)
        ent[1::2] = np.stack((cams[p[:, 1]], cams[p[:, 0]], p[:, 0], p[:, 1]), 1)
    return ent, te[:kk].cpu().numpy().reshape(-1), b.cpu().tolist(), (k, status)


def test_golden_cases(dev, golden):
    g = golden("ts_bias")
    for name, c in tb.cases().items():
        ent, te, bias, (k, status) = _call(dev, c)
        assert status == 0 and 2 * k == len(g[name + "_entries"]), name
        assert np.array_equal(ent, g[name + "_entries"]), name
        assert np.array_equal(te, g[name + "_time_error"]), name
        want = g[name + "_ts_bias"]
        if name in tb.ORDER_FREE or len(ent) == 0:
            assert np.array_equal(np.array(bias), want), (name, bias, want)
        else:
            bound = tb.ulp_bound(c["boxes"], c["cams"], c["objs"], c["timestamps"], c["ts_bias"], c["phi"], vel=tuple(g[name + "_vel"]))
            diff = float(np.abs(np.array(bias) - want).max())
            print("%s: bound %.3e observed %.3e" % (name, bound, diff))
            assert diff <= bound, name
    for name in ("cam0_only", "one_direction", "threshold", "overlap3"):
        assert name in tb.ORDER_FREE


def test_fuzz_equals_restatement(dev):
    """500 random scenes against the restatement fed with the device's own two mean speeds (_device_velocities): entry
    lists exactly equal, time_error and ts_bias bit for bit."""
    bad, with_pairs = [], 0
    for t in range(500):
        c = tb.fuzz_scene(t)
        ent, te, bias, (k, status) = _call(dev, c, max_pairs=4096)
        assert status == 0, t
        vel = _device_velocities(dev, c["objs"])
        r = tb.restated(c["boxes"], c["cams"], c["objs"], c["timestamps"], c["ts_bias"], c["phi"], vel=vel)
        with_pairs += len(r["entries"]) > 0
        ok = np.array_equal(ent, r["entries"]) and np.array_equal(te, r["time_error"], equal_nan=True) and \
            np.array_equal(np.array(bias), np.array(r["ts_bias"]), equal_nan=True)
        if not ok:
            bad.append(t)
    assert not bad, bad[:20]
    assert with_pairs >= 250, with_pairs


def _device_velocities(dev, objs):
    """The device's own two mean speeds, by the kernel's documented rule: fp64 sum, one division, one rounding to fp32
    (test_device_velocities_rule checks on the device that this is what the kernel uses)."""
    o = np.asarray(objs, np.float32).reshape(-1, 7)
    e, w = o[o[:, 5] == 1, 6].astype(np.float64), o[o[:, 5] == -1, 6].astype(np.float64)
    eb = np.float32(tb.MU_V) if len(e) == 0 else np.float32(_seq_sum(e) / len(e))
    wb = np.float32(-tb.MU_V) if len(w) == 0 else np.float32(np.float32(_seq_sum(w) / len(w)) * np.float32(-1))
    return eb, wb


def _seq_sum(v):
    s = 0.0
    for x in v:                    # at most 11 fp32 values of similar size: every fp64 partial sum is exact, any order
        s += float(x)
    return s


def test_device_velocities_rule(dev):
    """The rule _device_velocities applies is the kernel's: the time_error of one probe pair per direction, dx / vel
    with equal time stamps, is the restatement's with those speeds, bit for bit."""
    for t in range(40):
        objs = tb.fuzz_scene(t)["objs"]
        if len(objs) == 0:
            continue
        eb, wb = _device_velocities(dev, objs)
        for direction, v in ((1.0, eb), (-1.0, wb)):
            dx = np.float32(v) * np.float32(0.25)
            boxes = np.array([[500, 20, 60, 6, 5, direction], [500 + dx, 20, 60, 6, 5, direction]], np.float32)
            c = dict(boxes=boxes, cams=np.array([1, 0]), objs=objs, timestamps=[0.0, 0.0], ts_bias=[0.0, 0.0], phi=0.2)
            r = tb.restated(**c, vel=(eb, wb))
            ent, te, bias, _ = _call(dev, c)
            assert np.array_equal(te, r["time_error"]) and len(te) == 2, (t, direction)


def test_overflow_and_retry(dev, golden):
    from retinanet_mi355x import ops
    g = golden("ts_bias")
    c = tb.cases()["overlap3"]
    n_pairs = len(g["overlap3_entries"]) // 2
    ent, te, bias, (k, status) = _call(dev, c, max_pairs=n_pairs - 1)
    assert (k, status) == (n_pairs, ops.TS_OVERFLOW) and bias == c["ts_bias"]          # untouched at the C level
    ent, te, bias, (k, status) = _call(dev, c, max_pairs=n_pairs)
    assert status == 0 and np.array_equal(np.array(bias), g["overlap3_ts_bias"])
    # the drop-in starts from max(256, d) pairs: a scene with more than that
    v = tb._vehicles(30, 9000)
    boxes = np.concatenate([v] + [tb._second_view(v, 9001 + 10 * q) for q in range(5)])
    cams = np.repeat(np.arange(6), 30)
    c = dict(boxes=boxes, cams=cams, objs=tb._TRACKS_BOTH, timestamps=[1.0 + 0.001 * q for q in range(6)],
             ts_bias=[0.0, 0.001, 0.002, -0.001, 0.0, 0.003], phi=tb.PHI)
    r = tb.restated(**c)
    assert len(r["entries"]) // 2 > max(256, len(boxes))
    me = _drop_in(dev, c)
    calls = []
    real = ops.estimate_ts_bias

    def counting(*a, **k):
        calls.append(k.get("max_pairs"))
        return real(*a, **k)
    ops.estimate_ts_bias = counting
    try:
        me.estimate_ts_bias(torch.from_numpy(c["boxes"]).to(dev), torch.from_numpy(c["cams"]).to(dev))
    finally:
        ops.estimate_ts_bias = real
    assert calls == [None, len(r["entries"]) // 2]
    assert me.ts_bias == r["ts_bias"]
    c_bad = dict(c, cams=np.where(np.arange(len(cams)) == 7, 6, cams))
    info = ops.estimate_ts_bias(torch.from_numpy(c_bad["boxes"]).to(dev), torch.from_numpy(c_bad["cams"]).to(dev),
                                torch.from_numpy(c["objs"]).to(dev), torch.tensor(c["timestamps"], dtype=torch.float64, device=dev),
                                torch.zeros(6, dtype=torch.float64, device=dev), tb.PHI, tb.ALPHA, tb.MU_V, max_pairs=4096)
    assert int(info[1]) == ops.TS_BAD_CAMERA


class _View:
    """The filter as estimate_ts_bias reads it: view(with_direction=True) and mu_v."""
    def __init__(self, objs, dev=None):
        self.objs = torch.from_numpy(np.ascontiguousarray(objs))
        self.objs = self.objs.to(dev) if dev is not None else self.objs
        self.mu_v = torch.tensor(tb.MU_V)
        if dev is not None:
            self.device = dev

    def view(self, dt=None, with_direction=False):
        assert with_direction and dt is None
        return (list(range(len(self.objs))), self.objs) if len(self.objs) else ([], [])


def _drop_in(dev, c, filter_on_device=True):
    import mc3d_track
    me = mc3d_track.TrackManager()
    me.filter = _View(c["objs"], dev if filter_on_device else None)
    me.timestamps, me.ts_bias = list(c["timestamps"]), list(c["ts_bias"])
    me.phi_nms_space, me.ts_alpha = c["phi"], tb.ALPHA
    return me


def test_drop_in_device_cpu_and_empty_inputs(dev, golden):
    g = golden("ts_bias")
    for name, c in tb.cases().items():
        if name not in tb.ORDER_FREE and len(g[name + "_entries"]):
            continue
        results = []
        for on_gpu in (True, False):
            me = _drop_in(dev, c, filter_on_device=on_gpu)
            start = me.ts_bias
            b, k = torch.from_numpy(c["boxes"]), torch.from_numpy(c["cams"])
            assert me.estimate_ts_bias(b.to(dev) if on_gpu else b, k.to(dev) if on_gpu else k) is None
            assert isinstance(me.ts_bias, list) and all(isinstance(x, float) for x in me.ts_bias), name
            if len(g[name + "_entries"]) == 0:
                assert me.ts_bias is start, name                      # nothing written, as in the reference
            results.append(me.ts_bias)
        assert results[0] == results[1] == g[name + "_ts_bias"].tolist(), name
    me = _drop_in(dev, tb.cases()["no_detections"])
    me.estimate_ts_bias(torch.zeros((0, 6), device=dev), torch.zeros(0, dtype=torch.int64, device=dev))
    assert me.ts_bias == tb.cases()["no_detections"]["ts_bias"]


def test_device_count_limits_the_rows(dev):
    """d_count: the parser's device count stands in for the host's d -- rows past it are ignored."""
    c = tb.cases()["overlap3"]
    for k in (0, 5, 11, 16):
        sub = dict(c, boxes=c["boxes"][:k], cams=c["cams"][:k])
        want = tb.restated(**sub)
        ent, te, bias, _ = _call(dev, c, count=torch.tensor([k], dtype=torch.int32, device=dev))
        assert np.array_equal(ent, want["entries"]) and bias == want["ts_bias"], k


def test_custom_op_agrees_with_ops(dev):
    from retinanet_mi355x import ops, torch_ops
    c = tb.cases()["overlap3"]
    args = [torch.from_numpy(c["boxes"]).to(dev), torch.from_numpy(c["cams"]).to(dev), torch.from_numpy(c["objs"]).to(dev),
            torch.tensor(c["timestamps"], dtype=torch.float64, device=dev)]
    b1 = torch.tensor(c["ts_bias"], dtype=torch.float64, device=dev)
    b2 = b1.clone()
    i1 = ops.estimate_ts_bias(*args, b1, c["phi"], tb.ALPHA, tb.MU_V, max_pairs=64)
    i2 = torch.ops.retinanet_mi355x.estimate_ts_bias(*args, b2, c["phi"], tb.ALPHA, tb.MU_V, 64)
    assert torch.equal(i1, i2) and torch.equal(b1, b2) and not torch.equal(b1.cpu(), torch.tensor(c["ts_bias"], dtype=torch.float64))
    b3 = torch.tensor(c["ts_bias"], dtype=torch.float64, device=dev)
    torch.library.opcheck(torch_ops.estimate_ts_bias, (*args, b3, c["phi"], tb.ALPHA, tb.MU_V, 64),
                          test_utils=("test_schema", "test_autograd_registration"))


def _parse_tracker(dev, cls):
    import homography as hgm
    from util_track.kf import Torch_KF
    scores, labels, boxes, cams, names, (P, H), (P2, H2) = gc.tracker_post_inputs()

    def make_hg(Pm, Hm):
        hg = hgm.Homography(device=str(dev))
        hg.correspondence = {n: {"P": Pm[i], "H": Hm[i], "H_inv": np.linalg.inv(Hm[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    objs, ts, bias = tb.parse_scene()
    me = cls()
    me.sigma_d, me.phi_nms_im, me.phi_nms_space, me.ts_alpha = 0.1, 0.3, tb.PHI, tb.ALPHA
    me.cameras, me.est_ts = list(names), True
    me.hg = hgm.Homography_Wrapper(hg1=make_hg(P, H), hg2=make_hg(P2, H2))
    me.timestamps, me.ts_bias = list(ts), list(bias)
    me.filter = Torch_KF(dev, INIT=tc.kf_init())
    o = torch.from_numpy(objs)
    me.filter.add(o[:, :5].clone(), list(range(len(o))), o[:, 5].clone(), torch.zeros(len(o), dtype=torch.float64))
    me.filter.X[:, 5] = o[:, 6].to(dev)
    out = me.parse_detections(scores.to(dev), labels.to(dev), boxes.to(dev), cams.to(dev), refine_height=True)
    return me, out


def test_parse_est_ts_with_nothing_patched(dev, golden):
    """A class inheriting DetectionParser and TrackManager with the reference's default est_ts = True and nothing
    patched: the parser calls the drop-in estimate_ts_bias between the transforms and the space NMS.  A second run with
    a method that records what the parser hands over (and calls the drop-in) gives the very states the kernel saw:
    the restatement on those states has the golden's entry list exactly, the kernel's time_error and the tracker's
    ts_bias equal the restatement's bit for bit.  Against the golden itself, whose states differ from the device's
    within the parser's tolerance, every camera's bias is within ts_bias_cases.parse_bias_bound (two orders below the
    change of the biases)."""
    import mc3d_post
    import mc3d_track
    from retinanet_mi355x import ops
    g = golden("ts_bias")
    k = "parse_est_ts_"

    class Tracker(mc3d_post.DetectionParser, mc3d_track.TrackManager):
        pass
    seen = {}

    class Recording(Tracker):
        def estimate_ts_bias(self, boxes, camera_idxs):
            seen["boxes"], seen["cams"] = boxes.clone(), camera_idxs.clone()
            return mc3d_track.estimate_ts_bias(self, boxes, camera_idxs)
    me, (st, lb, sc, cm) = _parse_tracker(dev, Tracker)
    rec, _ = _parse_tracker(dev, Recording)
    assert np.array_equal(lb.cpu().numpy(), g[k + "labels"]) and np.array_equal(cm.cpu().numpy(), g[k + "cams"])
    assert np.array_equal(sc.cpu().numpy(), g[k + "scores"])
    assert np.allclose(st.cpu().numpy(), g[k + "state"], rtol=1e-5, atol=1e-4)
    assert rec.ts_bias == me.ts_bias and seen["boxes"].is_cuda
    objs, ts, bias = tb.parse_scene()
    states, cams = seen["boxes"].cpu().numpy(), seen["cams"].cpu().numpy()
    r = tb.restated(states, cams, objs, ts, bias, tb.PHI, vel=tuple(g[k + "vel"]))
    assert np.array_equal(r["entries"], g[k + "entries"])
    assert me.ts_bias == r["ts_bias"], (me.ts_bias, r["ts_bias"])
    ent, te, b2, (n_pairs, status) = _call(dev, dict(boxes=states, cams=cams, objs=objs, timestamps=ts, ts_bias=bias, phi=tb.PHI),
                                          max_pairs=1024)
    assert status == ops.TS_OK and np.array_equal(ent, g[k + "entries"]) and np.array_equal(te, r["time_error"])
    assert b2 == r["ts_bias"]
    bound, te_bound = tb.parse_bias_bound(states, r, len(bias))
    te_diff = np.abs(te.astype(np.float64) - g[k + "time_error"])
    diff = np.abs(np.array(me.ts_bias) - g[k + "ts_bias"])
    moved = np.abs(g[k + "ts_bias"] - np.array(bias))
    print("parse_est_ts: %d entries; per-camera ts_bias bound max %.3e, observed max %.3e, largest change of a bias %.3e; "
          "time_error bound max %.3e observed max %.3e" % (len(ent), bound.max(), diff.max(), moved.max(), te_bound.max(), te_diff.max()))
    assert (te_diff <= te_bound).all()
    assert (diff <= bound).all(), (diff, bound)
    assert bound.max() <= 0.02 * moved.max()


def test_sequence_through_the_gpu_filter(dev, golden):
    """8 frames: estimate_ts_bias -> space_nms -> associate -> prune on the GPU filter.  Ids, matchings and removals
    are exact per frame.  ts_bias per frame: against the restatement run on the very inputs the device saw (its own
    filter view, its own biases carried forward), within ulp_bound; against the golden within that bound summed over
    the frames so far (one update is a convex mix of two biases, so an earlier difference is passed on, not amplified)."""
    import mc3d_post
    import mc3d_track
    from util_track.kf import Torch_KF
    g = golden("ts_bias")

    class T(mc3d_post.DetectionParser, mc3d_track.TrackManager):
        pass
    t = T()
    for k, v in tc.PARAMS.items():
        setattr(t, k, v)
    t.class_dict = tc.class_dict()
    t.filter = Torch_KF(dev, INIT=tc.kf_init())
    t.fsld, t.all_classes, t.all_confs, t.all_cameras = {}, {}, {}, {}
    t.next_obj_id, t.updated_this_frame = 0, []
    t.ts_bias, t.phi_nms_space, t.ts_alpha = list(tb.SEQ_TS_BIAS), tb.PHI, tb.ALPHA
    log, phase = {}, ["none"]
    remove = t.filter.remove

    def logged_remove(ids):
        log[phase[0]] = sorted(int(i) for i in ids)
        remove(ids)
    t.filter.remove = logged_remove
    inc = t.increment_fslds

    def increment(*a):
        phase[0] = "fsld"
        return inc(*a)
    t.increment_fslds = increment
    allowed = 0.0
    for f, fr in enumerate(tb.sequence()):
        log.clear()
        key = "seq%d_" % f
        t.timestamps = list(fr["timestamps"])
        det = torch.from_numpy(fr["detections"]).to(dev)
        lab, sc, cam = (torch.from_numpy(fr[k]).to(dev) for k in ("labels", "scores", "cameras"))
        before = list(t.ts_bias)
        view = t.filter.view(with_direction=True)[1]
        objs = view.cpu().numpy() if len(view) else np.zeros((0, 7), np.float32)
        t.estimate_ts_bias(det.clone(), cam)
        vel = _device_velocities(dev, objs) if len(objs) else None
        r = tb.restated(fr["detections"], fr["cameras"], objs, fr["timestamps"], before, tb.PHI, vel=vel)
        assert np.array_equal(r["entries"], g[key + "entries"]), f
        bound = tb.ulp_bound(fr["detections"], fr["cameras"], objs, fr["timestamps"], before, tb.PHI, vel=vel)
        diff = float(np.abs(np.array(t.ts_bias) - np.array(r["ts_bias"])).max())
        allowed += bound                                                # against the golden: the same bound, carried forward
        gdiff = float(np.abs(np.array(t.ts_bias) - g[key + "ts_bias"]).max())
        print("frame %d: vs restatement bound %.3e observed %.3e | vs golden bound %.3e observed %.3e"
              % (f, bound, diff, allowed, gdiff))
        assert diff <= bound, f
        assert gdiff <= allowed, f
        idxs = t.space_nms(det, sc, threshold=t.phi_nms_space)
        assert np.array_equal(idxs.cpu().numpy(), g[key + "nms_idx"]), f
        det, lab, sc, cam = det[idxs], lab[idxs], sc[idxs], cam[idxs]
        pre_ids, matchings = t.associate(det, lab, sc, cam)
        phase[0] = "over"
        t.remove_overlaps()
        phase[0] = "anom"
        t.remove_anomalies(x_bounds=t.x_range)
        phase[0] = "none"
        assert pre_ids == g[key + "pre_ids"].tolist(), f
        m = matchings.cpu().numpy() if isinstance(matchings, torch.Tensor) else np.asarray(matchings)
        assert np.array_equal(m.reshape(-1, 2), g[key + "match"]), f
        assert sorted(t.fsld.items()) == [tuple(r_) for r_ in g[key + "fsld"].tolist()], f
        assert t.next_obj_id == int(g[key + "next_obj_id"]), f
        for ph in ("fsld", "over", "anom"):
            assert log.get(ph, []) == g[key + "rm_" + ph].tolist(), (f, ph)
        assert t.filter.view()[0] == g[key + "ids"].tolist(), f
        ck = sorted(t.all_classes)
        assert ck == g[key + "class_ids"].tolist() and np.array_equal(np.array([t.all_classes[c] for c in ck]), g[key + "classes"]), f
        want = g[key + "X"]
        assert float(np.abs(t.filter.X.cpu().numpy() - want).max() / max(1.0, np.abs(want).max())) <= 1e-4, f
        assert np.abs(t.filter.T.cpu().numpy() - g[key + "T"]).max() <= 1e-9 + allowed, f

"""GPU: detector validation on the device (csrc/eval_ap.hip: rn_eval_select / rn_eval_match / rn_eval_ap; ops.eval_*;
torch.ops.retinanet_mi355x.eval_*; csv_eval.evaluate / evaluate_detections) against the numpy restatement in
tests/eval_cases.py and the reference's own results in tests/golden/csv_eval.npz.

Compared exactly: the selected rows, the TP flag of every row, the sorted order, the annotation counts, status and
cursor.  The AP holds to T * 2^-52 absolute (T = the class's true positives, at least 2^-52): its terms come from the
same fp64 operations on both sides and are non-negative with a sum <= 1, so two summation orders of T terms differ by
at most 2 (T - 1) 2^-53 (eval_cases.ap_bound).  Two runs give the same bits."""

import numpy as np
import pytest
import torch

import eval_cases as ec
import golden_cases as gc

pytestmark = pytest.mark.gpu

GUARD = 64


def _t(dev, d):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in d)


def _via_ops(dev, dets, anns, C, iou_threshold=0.5, score_threshold=0.05, max_detections=100, box_cols=None, table_rows=None,
             custom=False):
    """The three stages through ops (or through the registered operators) -> what eval_cases.restated returns."""
    from retinanet_mi355x import ops, torch_ops  # noqa: F401  (torch_ops registers the operators)
    if table_rows is None:
        table_rows = sum(min(len(d[0]), max_detections) for d in dets)
    table, img_rows, state = ops.eval_table(table_rows, len(dets), dev)
    ab, ao = ec.pack_annotations(anns, C)
    ab, ao = torch.from_numpy(ab).to(dev), torch.from_numpy(ao).to(dev)
    for i, d in enumerate(dets):
        s, l, b = _t(dev, d)
        if custom:
            c0 = ops.eval_box_cols(b, box_cols)[0] if len(d[0]) else 0
            torch.ops.retinanet_mi355x.eval_select(s, l, b, table, img_rows, state, i, C, score_threshold, max_detections, c0)
        else:
            ops.eval_select(s, l, b, table, img_rows, state, i, C, score_threshold, max_detections, box_cols)
    if custom:
        tp, num = torch.ops.retinanet_mi355x.eval_match(table, img_rows, ab, ao, C, iou_threshold)
        ap, order = torch.ops.retinanet_mi355x.eval_ap(table, state, tp, num)
    else:
        tp, num = ops.eval_match(table, img_rows, ab, ao, C, iou_threshold)
        ap, order = ops.eval_ap(table, state, tp, num)
    D, status = (int(x) for x in state.cpu())
    assert (order[D:] == -1).all()
    return dict(rows=table[:D].cpu().numpy(), img_rows=img_rows.cpu().numpy(), tp=tp[:D].cpu().numpy(),
                order=order[:D].cpu().numpy(), num_annotations=num.cpu().numpy().astype(np.int64), ap=ap.cpu().numpy(),
                status=status)


class _Guarded:
    """nbytes of device memory between two guard zones."""
    def __init__(self, dev, nbytes, fill=0):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[GUARD:GUARD + self.n] = fill
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.n:] == 0xA5).all())

    def numpy(self, dtype):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(dtype)


def _via_cabi(dev, dets, anns, C, iou_threshold=0.5, score_threshold=0.05, max_detections=100, box_cols=(0, 4), table_rows=None):
    """The C ABI itself, every output between guard bytes and sized exactly."""
    from retinanet_mi355x import _hip
    lib = _hip.load()
    I = len(dets)
    if table_rows is None:
        table_rows = sum(min(len(d[0]), max_detections) for d in dets)
    ab, ao = ec.pack_annotations(anns, C)
    M = len(ab)
    abt, aot = torch.from_numpy(ab).to(dev), torch.from_numpy(ao).to(dev)
    table, img_rows, state = _Guarded(dev, 32 * table_rows), _Guarded(dev, 8 * I), _Guarded(dev, 8)
    tp, num, ap, order = _Guarded(dev, table_rows), _Guarded(dev, 4 * C), _Guarded(dev, 8 * C), _Guarded(dev, 4 * table_rows, 0xFF)
    taken, ws = _Guarded(dev, M), _Guarded(dev, lib.rn_eval_ap_workspace_bytes(table_rows))
    stream = _hip.stream()
    keep = []
    for i, d in enumerate(dets):
        s, l, b = _t(dev, d)
        keep.append((s, l, b))
        K = len(d[0])
        rc = lib.rn_eval_select(s.data_ptr() if K else None, l.data_ptr() if K else None, b.data_ptr() if K else None,
                                b.shape[1] if K else 4, box_cols[0], K, score_threshold, max_detections, i, I, C,
                                table.ptr if table_rows else None, table_rows, state.ptr, img_rows.ptr, stream)
        assert rc == 0
    assert lib.rn_eval_match(table.ptr if table_rows else None, table_rows, img_rows.ptr, I, C, abt.data_ptr() if M else None,
                             aot.data_ptr(), M, iou_threshold, taken.ptr if M else None, tp.ptr if table_rows else None, num.ptr,
                             stream) == 0
    assert lib.rn_eval_ap(table.ptr if table_rows else None, table_rows, state.ptr, tp.ptr if table_rows else None, num.ptr, C,
                          ws.ptr if table_rows else None, ap.ptr, order.ptr if table_rows else None, stream) == 0
    torch.cuda.synchronize()
    for g in (table, img_rows, state, tp, num, ap, order, taken, ws):
        assert g.intact()
    D, status = (int(x) for x in state.numpy(np.int32))
    o = order.numpy(np.int32)
    assert (o[D:] == -1).all()
    return dict(rows=table.numpy(np.int32).reshape(-1, 8)[:D], img_rows=img_rows.numpy(np.int32).reshape(-1, 2),
                tp=tp.numpy(np.uint8)[:D], order=o[:D], num_annotations=num.numpy(np.int32).astype(np.int64),
                ap=ap.numpy(np.float64), status=status)


def _same(got, want, what):
    assert got["status"] == want["status"], what
    assert np.array_equal(got["rows"], want["rows"]), what
    assert np.array_equal(got["img_rows"], want["img_rows"]), what
    assert np.array_equal(got["tp"], want["tp"]), what
    assert np.array_equal(got["order"], want["order"]), what
    assert np.array_equal(got["num_annotations"], want["num_annotations"]), what
    diff, bound = np.abs(got["ap"] - want["ap"]), ec.ap_bound(want["tp_count"])
    print("%s: AP diff max %.3e, bound min %.3e, T max %d" % (what, diff.max(), bound.min(), want["tp_count"].max()))
    assert (diff <= bound).all(), (what, diff, bound)


PATHS = {"ops": _via_ops, "cabi": _via_cabi, "custom": lambda *a, **k: _via_ops(*a, custom=True, **k)}


@pytest.fixture(scope="module")
def golden_restated(golden):
    g = golden("csv_eval")
    out = {}
    for name in ec.GOLDEN:
        dets, anns, C, kw = ec.unpack_golden(g, name)
        out[name] = (dets, anns, C, kw, ec.restated(dets, anns, C, **kw))
    return out


@pytest.mark.parametrize("path", sorted(PATHS))
def test_golden_cases(dev, golden, golden_restated, path):
    g = golden("csv_eval")
    for name, (dets, anns, C, kw, want) in golden_restated.items():
        got = PATHS[path](dev, dets, anns, C, **kw)
        _same(got, want, "%s/%s" % (path, name))
        diff = np.abs(got["ap"] - g[name + "_ap"])                               # ... and the reference's own numbers
        assert (diff <= ec.ap_bound(want["tp_count"])).all(), (name, diff)
        assert np.array_equal(got["num_annotations"].astype(np.float64), g[name + "_num_annotations"])


def test_edge_cases(dev):
    for name, c in ec.edge_cases().items():
        want = ec.restated(c["dets"], c["anns"], c["C"], **c["kw"])
        for path in ("ops", "cabi"):
            got = PATHS[path](dev, c["dets"], c["anns"], c["C"], **c["kw"])
            _same(got, want, "%s/%s" % (path, name))
            assert got["tp"].tolist() == c["tp"] and got["num_annotations"].tolist() == c["num_annotations"], name
            assert not np.isnan(got["ap"]).any()
            assert np.abs(got["ap"] - np.array(c["ap"])).max() <= 2.0 ** -52 * max(1, sum(c["tp"])), name


def _boxes(rng, n):
    xy = rng.uniform(0, 300, (n, 2))
    return np.concatenate((xy, xy + rng.uniform(10, 80, (n, 2))), 1).astype(np.float32)


def _scene(seed, Ks, C, levels=16, ann_per=3):
    """Images with Ks[i] detections, scores on a few levels (many ties), annotations copied from some detections."""
    rng = np.random.RandomState(seed)
    dets, anns = [], []
    for K in Ks:
        b = _boxes(rng, K)
        l = rng.randint(0, C, K)
        s = ((rng.randint(0, levels, K) + 1) / float(levels + 1)).astype(np.float32)
        dets.append((s, l.astype(np.int64), b))
        per = []
        for c in range(C):
            mine = np.where(l == c)[0][:ann_per]
            per.append(b[mine].astype(np.float64) if len(mine) else np.zeros((0, 4)))
        anns.append(per)
    return dets, anns


def test_selection_sizes_and_thresholds(dev):
    """K = 0, 1, max_detections - 1, max_detections, max_detections + 1; all scores equal; a score at the threshold;
    a negative threshold over signed zeros -- one dataset of eight images."""
    rng = np.random.RandomState(5)
    md = 7
    dets, anns = _scene(1, [0, 1, md - 1, md, md + 1, 20, 12, 9], 2, levels=5)
    dets[5] = (np.full(20, 0.5, np.float32), dets[5][1], dets[5][2])                       # all equal: the first md by index
    s = dets[6][0].copy()
    s[::3] = np.float32(0.3)
    dets[6] = (s, dets[6][1], dets[6][2])
    for thr, tag in ((0.3, "threshold"), (0.05, "default")):
        want = ec.restated(dets, anns, 2, score_threshold=thr, max_detections=md)
        if thr == 0.3:
            sel6 = want["rows"][want["rows"][:, 6] == 6]
            assert len(sel6) and not np.any(sel6[:, 4].view(np.float32) == np.float32(0.3))      # equal is not above
        for path in ("ops", "cabi"):
            _same(PATHS[path](dev, dets, anns, 2, score_threshold=thr, max_detections=md), want, tag + "/" + path)
    z = np.array([0.0, -0.0, -0.0, 0.0, -1.0, -0.0, 0.0], np.float32)
    dz = [(z, np.zeros(7, np.int64), _boxes(rng, 7))]
    az = [[dz[0][2][[1, 3]].astype(np.float64)]]
    want = ec.restated(dz, az, 1, score_threshold=-0.5, max_detections=4)
    assert want["rows"][:, 7].tolist() == [0, 1, 2, 3]
    _same(_via_ops(dev, dz, az, 1, score_threshold=-0.5, max_detections=4), want, "signed zeros")


def test_selection_limits_and_status(dev):
    """K at ops.EVAL_MAX_K; K one above it, a selected label equal to C, and a full table set their status bit and append
    nothing, while the other images of the dataset go in."""
    from retinanet_mi355x import ops
    rng = np.random.RandomState(9)
    K = ops.EVAL_MAX_K
    big = (((rng.randint(0, 1 << 16, K) + 1) / float((1 << 16) + 1)).astype(np.float32), rng.randint(0, 3, K).astype(np.int64),
           np.zeros((K, 4), np.float32))
    big[2][:, 2:] = 4.0
    small, anns1 = _scene(2, [9], 3)
    anns = [anns1[0], anns1[0]]
    want = ec.restated([big, small[0]], anns, 3, max_detections=100)
    assert len(want["rows"]) == 109
    _same(_via_ops(dev, [big, small[0]], anns, 3, max_detections=100), want, "K at the limit")
    over = tuple(np.concatenate((x, x[:1])) for x in big)
    want = ec.restated([over, small[0]], anns, 3)
    got = _via_ops(dev, [over, small[0]], anns, 3, table_rows=109)
    assert got["status"] == ops.EVAL_TOO_MANY and got["img_rows"].tolist()[0] == [0, 0] and len(got["rows"]) == 9
    _same(got, want, "K above the limit")
    bad = (small[0][0], small[0][1].copy(), small[0][2])
    bad[1][int(np.argmax(bad[0]))] = 3                                                    # label == C on a selected row
    want = ec.restated([bad, small[0]], anns, 3)
    got = _via_cabi(dev, [bad, small[0]], anns, 3)
    assert got["status"] == ops.EVAL_BAD_LABEL and len(got["rows"]) == 9
    _same(got, want, "label == C")
    want = ec.restated([small[0], small[0], small[0]], anns + anns[:1], 3, table_rows=20)
    got = _via_cabi(dev, [small[0], small[0], small[0]], anns + anns[:1], 3, table_rows=20)
    assert got["status"] == ops.EVAL_TABLE_FULL and got["img_rows"].tolist() == [[0, 9], [9, 18], [18, 18]]
    _same(got, want, "table full")
    with pytest.raises(RuntimeError):
        ops.eval_select(*_t(dev, small[0]), *ops.eval_table(10, 1, dev), 0, 3, max_detections=ops.EVAL_MAX_DET + 1)


@pytest.mark.parametrize("D", [63, 64, 65, 2047, 2048, 2049, 4100])
def test_sort_sizes(dev, D):
    """D one below, at and one above the sort's tile (64) and per-workgroup span (2048), and three workgroups; few score
    levels, so that most neighbours tie and the order is decided by stability."""
    from retinanet_mi355x import ops
    assert (ops.EVAL_SORT_TILE, ops.EVAL_SORT_SPAN) == (64, 2048) and D <= 2 * 2048 + 2048
    Ks = [D] if D <= 4096 else [4096, D - 4096]
    dets, anns = _scene(D, Ks, 3, levels=8, ann_per=5)
    want = ec.restated(dets, anns, 3, max_detections=4096)
    assert len(want["rows"]) == D
    _same(_via_ops(dev, dets, anns, 3, max_detections=4096), want, "D=%d" % D)
    if D in (65, 2049):
        _same(_via_cabi(dev, dets, anns, 3, max_detections=4096), want, "cabi D=%d" % D)


def test_sort_one_class_equal_scores_and_256_classes(dev):
    # every score equal over 60 images x 80 rows = 4800 rows (three workgroups), one class: the order is the table order
    dets, anns = _scene(3, [80] * 60, 1, levels=1, ann_per=4)
    want = ec.restated(dets, anns, 1)
    assert np.array_equal(want["order"], np.arange(4800))
    got = _via_ops(dev, dets, anns, 1)
    _same(got, want, "equal scores")
    again = _via_ops(dev, dets, anns, 1)
    assert got["ap"].tobytes() == again["ap"].tobytes()                                   # bit-identical repeats
    # 256 classes, some without annotations, some without detections
    dets, anns = _scene(4, [90] * 30, 256, levels=6, ann_per=1)
    for per in anns:
        per[7] = np.zeros((0, 4))
    dets = [(s, np.where(l == 9, 10, l), b) for s, l, b in dets]
    want = ec.restated(dets, anns, 256)
    assert want["num_annotations"][7] == 0 and want["num_annotations"][9] > 0 and not np.any(want["rows"][:, 5] == 9)
    got = _via_ops(dev, dets, anns, 256)
    _same(got, want, "256 classes")
    assert got["ap"][7] == 0 and got["ap"][9] == 0
    assert got["ap"].tobytes() == _via_cabi(dev, dets, anns, 256)["ap"].tobytes()


def test_evaluate_detections_matches_the_stages(dev, golden_restated):
    """csv_eval.evaluate_detections: the reference's dict of Python floats, (0, 0) for a class without annotations, and a
    RuntimeError for a status."""
    from retinanet_mi355x import csv_eval
    dets, anns, C, kw, want = golden_restated["b"]
    res = csv_eval.evaluate_detections([_t(dev, d) for d in dets], anns, C, **kw)
    twice = csv_eval.evaluate_detections([_t(dev, d) for d in dets], anns, C, **kw)
    assert res == twice and sorted(res) == list(range(C))
    for c in range(C):
        assert isinstance(res[c][0], float) and res[c][1] == float(want["num_annotations"][c])
        assert abs(res[c][0] - want["ap"][c]) <= ec.ap_bound(want["tp_count"][c])
    c = ec.edge_cases()["empty_classes"]
    res = csv_eval.evaluate_detections([_t(dev, d) for d in c["dets"]], c["anns"], 3)
    assert res == {0: (1.0, 1.0), 1: (0, 0), 2: (0.0, 2.0)}
    with pytest.raises(RuntimeError, match="label"):
        csv_eval.evaluate_detections([_t(dev, d) for d in c["dets"]], [a[:1] for a in c["anns"]], 1)


class _Frames:
    """The generator surface csv_eval.evaluate uses."""
    def __init__(self, frames, anns, C):
        self.frames, self.anns, self.C = frames, anns, C

    def __len__(self):
        return len(self.frames)

    def num_classes(self):
        return self.C

    def __getitem__(self, i):
        return (self.frames[i],)

    def load_annotations(self, i):
        return self.anns[i]

    def label_to_name(self, label):
        return "class%d" % label


class _Recorder(torch.nn.Module):
    """Keeps what the model returned, so that both entry points see the same outputs."""
    def __init__(self, net):
        super().__init__()
        self.net, self.outs = net, []

    def forward(self, x):
        out = self.net(x)
        self.outs.append(out)
        return out


@pytest.mark.parametrize("directional", [False, True])
def test_evaluate_end_to_end(dev, directional, capsys):
    """csv_eval.evaluate with the 2D and the directional model on two small frames equals evaluate_detections on the same
    model outputs; the annotations are some of the model's own boxes, so that there are true positives."""
    from retinanet_mi355x import csv_eval, modules
    _, sd, img, _ = gc.model_case("resnet18", directional)
    net = modules.resnet18(num_classes=4, directional=directional)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    with torch.no_grad():
        net.classificationModel.output.bias.add_(3.0)                                     # scores above 0.05
        first = [net(img[i:i + 1].to(dev)) for i in range(2)]
    cols = (16, 20) if directional else (0, 4)
    assert all(o[2].dim() == 2 and o[2].shape[1] == (20 if directional else 4) and o[0].numel() > 0 for o in first)
    anns = []
    for s, l, b in first:
        l, b = l.cpu().numpy(), b.cpu().numpy().astype(np.float64)[:, cols[0]:cols[1]]
        anns.append([np.concatenate((b[l == c][:2], np.full((len(b[l == c][:2]), 1), float(c))), 1) for c in range(4)])
    rec = _Recorder(net)
    got = csv_eval.evaluate(_Frames(list(img), anns, 4), rec)
    assert len(rec.outs) == 2 and not net.training
    want = csv_eval.evaluate_detections(rec.outs, anns, 4, box_cols=cols)
    assert want == csv_eval.evaluate_detections(rec.outs, anns, 4)                        # the default box_cols
    assert got == want and any(v[0] > 0 for v in got.values())
    text = capsys.readouterr().out
    assert "\nmAP:\n" in text and "class0: %s" % got[0][0] in text
    if directional:
        import retinanet.csv_eval as mirror                                               # the drop-in's name
        assert mirror.evaluate is csv_eval.evaluate and mirror.compute_overlap is csv_eval.compute_overlap

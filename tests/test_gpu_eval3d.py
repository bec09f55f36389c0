"""GPU: validation of the detector's 3D boxes on the device (csrc/eval_cuboid.hip: rn_eval_corners / rn_eval_cuboid_overlap /
rn_eval_cuboid_assign / rn_eval_cuboid_errors; ops.eval_corners / eval_cuboid_*; torch.ops.retinanet_mi355x.*;
eval3d.evaluate_cuboids / evaluate_3d / validator) against the restatement in tests/eval3d_cases.py.

Compared bit for bit: the corner table, best_iou, best_ann, every TP flag, the matched annotation, the annotation counts,
the per-row error terms and the per-class sums -- the restatement performs the same fp64 operations in the same order, and
fp64 sqrt and division are correctly rounded on both sides -- together with the selected rows, the sorted order, status and
cursor.  The AP holds to eval_cases.ap_bound.  Two runs give the same bytes."""
import numpy as np
import pytest
import torch

import eval3d_cases as e3
import eval_cases as ec
import golden_cases as gc

pytestmark = pytest.mark.gpu

GUARD = 64
EXACT = ("corners", "best_iou", "best_ann", "tp", "matched", "num_annotations", "terms", "sums", "rows", "img_rows", "order")


def _t(dev, d):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in d)


def _rows(dets, max_detections, table_rows):
    return sum(min(len(d[0]), max_detections) for d in dets) if table_rows is None else table_rows


def _via_ops(dev, dets, labels, C, overlap="silhouette", iou_thresholds=(0.5, 0.7), score_threshold=0.05, max_detections=100,
             table_rows=None, custom=False):
    """The stages through ops (or through the registered operators) -> what eval3d_cases.restated returns."""
    from retinanet_mi355x import ops, torch_ops  # noqa: F401  (torch_ops registers the operators)
    t = torch.ops.retinanet_mi355x
    rows = _rows(dets, max_detections, table_rows)
    table, img_rows, state = ops.eval_table(rows, len(dets), dev)
    corners = torch.zeros((rows, 16), dtype=torch.float32, device=dev)
    ac, ao = e3.pack_labels(labels, C)
    M = len(ac)
    ac, ao = torch.from_numpy(ac).to(dev), torch.from_numpy(ao).to(dev)
    thr = [float(x) for x in iou_thresholds]
    for i, d in enumerate(dets):
        s, l, b = _t(dev, d)
        if custom:
            t.eval_select(s, l, b, table, img_rows, state, i, C, score_threshold, max_detections, 16)
            t.eval_corners(b, table, img_rows, i, corners)
        else:
            ops.eval_select(s, l, b, table, img_rows, state, i, C, score_threshold, max_detections, (16, 20))
            ops.eval_corners(b, table, img_rows, i, corners)
    if custom:
        best_iou, best_ann = t.eval_cuboid_overlap(table, img_rows, corners, ac, ao, C, overlap)
        tp, num, matched = t.eval_cuboid_assign(table, img_rows, best_iou, best_ann, ao, M, C, thr)
        terms, sums = t.eval_cuboid_errors(table, state, img_rows, corners, ac, ao, C, tp[0], matched, best_iou)
    else:
        best_iou, best_ann = ops.eval_cuboid_overlap(table, img_rows, corners, ac, ao, C, overlap)
        tp, num, matched = ops.eval_cuboid_assign(table, img_rows, best_iou, best_ann, ao, M, C, thr)
        terms, sums = ops.eval_cuboid_errors(table, state, img_rows, corners, ac, ao, C, tp[0], matched, best_iou)
    aps, order = [], None
    for k in range(len(thr)):
        ap, order = ops.eval_ap(table, state, tp[k], num)
        aps.append(ap.cpu().numpy())
    D, status = (int(x) for x in state.cpu())
    for x, fill in ((best_iou, 0), (best_ann, -1), (matched, -1), (terms, 0), (tp.t(), 0)):
        assert (x[D:] == fill).all()                                               # rows behind the cursor
    return dict(rows=table[:D].cpu().numpy(), img_rows=img_rows.cpu().numpy(), status=status, order=order[:D].cpu().numpy(),
                corners=corners[:D].cpu().numpy(), best_iou=best_iou[:D].cpu().numpy(), best_ann=best_ann[:D].cpu().numpy(),
                tp=tp[:, :D].cpu().numpy(), matched=matched[:D].cpu().numpy(), num_annotations=num.cpu().numpy().astype(np.int64),
                ap=np.stack(aps), terms=terms[:D].cpu().numpy(), sums=sums.cpu().numpy())


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


def _via_cabi(dev, dets, labels, C, overlap="silhouette", iou_thresholds=(0.5, 0.7), score_threshold=0.05, max_detections=100,
              table_rows=None):
    """The C ABI itself, every output between guard bytes and sized exactly."""
    from retinanet_mi355x import _hip, ops
    lib = _hip.load()
    I, T = len(dets), len(iou_thresholds)
    R = _rows(dets, max_detections, table_rows)
    ac, ao = e3.pack_labels(labels, C)
    M = len(ac)
    act, aot = torch.from_numpy(ac).to(dev), torch.from_numpy(ao).to(dev)
    thr = torch.tensor([float(x) for x in iou_thresholds], dtype=torch.float64, device=dev)
    table, img_rows, state = _Guarded(dev, 32 * R), _Guarded(dev, 8 * I), _Guarded(dev, 8)
    corners, best_iou, best_ann = _Guarded(dev, 64 * R), _Guarded(dev, 8 * R, 0x11), _Guarded(dev, 4 * R, 0x11)
    tp, matched, num, taken = _Guarded(dev, T * R, 0x11), _Guarded(dev, 4 * R, 0x11), _Guarded(dev, 4 * C), _Guarded(dev, T * M)
    terms, sums = _Guarded(dev, 32 * R, 0x11), _Guarded(dev, 40 * C, 0x11)
    ap, order, ws = _Guarded(dev, 8 * C * T), _Guarded(dev, 4 * R, 0xFF), _Guarded(dev, lib.rn_eval_ap_workspace_bytes(R))
    stream = _hip.stream()
    some = lambda g: g.ptr if R else None                                          # noqa: E731
    keep = []
    for i, d in enumerate(dets):
        s, l, b = _t(dev, d)
        keep.append((s, l, b))
        K = len(d[0])
        assert lib.rn_eval_select(s.data_ptr() if K else None, l.data_ptr() if K else None, b.data_ptr() if K else None,
                                  20, 16, K, score_threshold, max_detections, i, I, C, some(table), R, state.ptr, img_rows.ptr,
                                  stream) == 0
        assert lib.rn_eval_corners(b.data_ptr() if K else None, 20, K, i, I, img_rows.ptr, some(table), R, some(corners),
                                   stream) == 0
    assert lib.rn_eval_cuboid_overlap(some(table), R, img_rows.ptr, I, C, some(corners), act.data_ptr() if M else None,
                                      aot.data_ptr(), M, ops.EVAL_CUBOID_OVERLAPS[overlap], some(best_iou), some(best_ann),
                                      stream) == 0
    assert lib.rn_eval_cuboid_assign(some(table), R, img_rows.ptr, I, C, aot.data_ptr(), M, some(best_iou), some(best_ann),
                                     thr.data_ptr(), T, taken.ptr if M else None, some(tp), num.ptr, some(matched), stream) == 0
    assert lib.rn_eval_cuboid_errors(some(table), R, state.ptr, I, C, some(corners), act.data_ptr() if M else None,
                                     aot.data_ptr(), M, some(tp), some(matched), some(best_iou), some(terms), sums.ptr,
                                     stream) == 0
    for k in range(T):
        assert lib.rn_eval_ap(some(table), R, state.ptr, (tp.ptr + k * R) if R else None, num.ptr, C, ws.ptr if R else None,
                              ap.ptr + 8 * C * k, some(order), stream) == 0
    torch.cuda.synchronize()
    for g in (table, img_rows, state, corners, best_iou, best_ann, tp, matched, num, taken, terms, sums, ap, order, ws):
        assert g.intact()
    D, status = (int(x) for x in state.numpy(np.int32))
    return dict(rows=table.numpy(np.int32).reshape(-1, 8)[:D], img_rows=img_rows.numpy(np.int32).reshape(-1, 2), status=status,
                order=order.numpy(np.int32)[:D], corners=corners.numpy(np.float32).reshape(-1, 16)[:D],
                best_iou=best_iou.numpy(np.float64)[:D], best_ann=best_ann.numpy(np.int32)[:D],
                tp=tp.numpy(np.uint8).reshape(T, -1)[:, :D], matched=matched.numpy(np.int32)[:D],
                num_annotations=num.numpy(np.int32).astype(np.int64), ap=ap.numpy(np.float64).reshape(T, C),
                terms=terms.numpy(np.float64).reshape(-1, 4)[:D], sums=sums.numpy(np.float64).reshape(C, 5))


PATHS = {"ops": _via_ops, "cabi": _via_cabi, "custom": lambda *a, **k: _via_ops(*a, custom=True, **k)}


def _same(got, want, what):
    assert got["status"] == want["status"], what
    for key in EXACT:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():                                             # bit for bit
            bad = np.argwhere(a != b)
            raise AssertionError("%s: %s differs at %s: %r against %r" % (what, key, bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))
    diff, bound = np.abs(got["ap"] - want["ap"]), ec.ap_bound(want["tp_count"])
    print("%s: AP diff max %.3e, bound min %.3e, true positives %s" % (what, diff.max(), bound.min(), want["tp_count"].sum(1).tolist()))
    assert (diff <= bound).all(), (what, diff, bound)


# ------------------------------------------------------------------------------------------------ closed-form scenes
@pytest.mark.parametrize("path", sorted(PATHS))
def test_closed_form_scenes(dev, path):
    for name, s in e3.scenes().items():
        want = e3.restated(s["dets"], s["labels"], s["C"], **s["kw"])
        got = PATHS[path](dev, s["dets"], s["labels"], s["C"], **s["kw"])
        _same(got, want, "%s/%s" % (path, name))
        assert got["best_ann"].tolist() == s["best_ann"] and got["tp"].tolist() == s["tp"], name
        if "best_iou" in s:
            assert got["best_iou"].tolist() == s["best_iou"], name
        if "reversed" in s:
            assert got["sums"][:, 4].tolist() == s["reversed"], name


# ------------------------------------------------------------------------------------------------ generated datasets
def _dataset(seed, spec, C, levels=6, jitter=4.0):
    """spec: per image a list of (class, detections, annotations).  Annotations are projected cuboids (fp64); a detection is
    a jittered copy of one of its group's annotations, or a cuboid of its own; scores on a few levels, so that many tie."""
    rng = np.random.RandomState(seed)
    dets, labels = [], []
    for groups in spec:
        rows, labs = [], []
        for c, n_det, n_ann in groups:
            anns = []
            for _ in range(n_ann):
                w, h = rng.uniform(20, 200), rng.uniform(20, 150)
                anns.append(np.asarray(e3.cuboid(rng.uniform(0, 600), rng.uniform(0, 400), w, h)))
                labs.append(e3.label(anns[-1], c))
            for _ in range(n_det):
                if anns and rng.rand() < 0.8:
                    d = anns[rng.randint(len(anns))] + rng.normal(0, jitter, 16)
                    if rng.rand() < 0.15:
                        d = d.reshape(8, 2)[e3.REVERSED].reshape(-1)
                else:
                    d = np.asarray(e3.cuboid(rng.uniform(0, 600), rng.uniform(0, 400), rng.uniform(20, 200), rng.uniform(20, 150)))
                rows.append(((rng.randint(levels) + 1) / float(levels + 1), c, d))
        order = rng.permutation(len(rows))
        dets.append(e3.det_rows([rows[k] for k in order]))
        labels.append(e3.labels_of(*labs) if labs else np.zeros((0, 21)))
    return dets, labels


@pytest.fixture(scope="module")
def mixed():
    """Seven images over 8 classes: one without detections, one without annotations, one whose selection sets a status and
    appends nothing; class 6 has annotations and no detections, class 7 detections and no annotations."""
    spec = [[(0, 5, 2), (1, 3, 3), (6, 0, 2)], [], [(2, 4, 0), (7, 3, 0)], [(0, 6, 3), (3, 2, 1), (7, 2, 0)],
            [(1, 4, 2), (2, 3, 2)], [(4, 5, 4), (5, 1, 1), (6, 0, 1)], [(0, 3, 1), (5, 4, 3)]]
    dets, labels = _dataset(31, spec, 8)
    labels[1] = e3.labels_of(e3.label(e3.cuboid(10, 10, 50, 40), 3))                # annotations, no detections
    bad = dets[4][1].copy()
    bad[int(np.argmax(dets[4][0]))] = 8                                            # a selected label == C
    dets[4] = (dets[4][0], bad, dets[4][2])
    return dets, labels


@pytest.mark.parametrize("path", sorted(PATHS))
def test_dataset_with_empty_images_and_a_status(dev, mixed, path):
    dets, labels = mixed
    want = e3.restated(dets, labels, 8)
    assert want["status"] == ec.BAD_LABEL and want["img_rows"][1].tolist() == [0 + len(dets[0][0])] * 2
    assert want["img_rows"][4, 0] == want["img_rows"][4, 1] and want["tp"][0].sum() > 5 and want["sums"][:, 4].sum() >= 1
    assert want["num_annotations"][6] == 3 and not np.any(want["rows"][:, 5] == 6) and want["num_annotations"][7] == 0
    got = PATHS[path](dev, dets, labels, 8)
    _same(got, want, path)
    assert got["ap"][0, 6] == 0 and got["ap"][0, 7] == 0
    again = PATHS[path](dev, dets, labels, 8)
    for key in EXACT + ("ap",):
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(again[key]).tobytes(), key


@pytest.mark.parametrize("thresholds", [(0.5,), (0.7, 0.5), (0.1, 0.3, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95)])
def test_one_two_and_eight_thresholds(dev, mixed, thresholds):
    dets, labels = mixed[0][:4], mixed[1][:4]
    want = e3.restated(dets, labels, 8, iou_thresholds=thresholds)
    assert want["tp"].shape[0] == len(thresholds) and want["tp"][0].sum() >= want["tp"][-1].sum()
    if len(thresholds) == 8:
        assert want["tp"][0].sum() > want["tp"][6].sum() > want["tp"][7].sum()
    for path in ("ops", "cabi"):
        _same(PATHS[path](dev, dets, labels, 8, iou_thresholds=thresholds), want, "%s/T=%d" % (path, len(thresholds)))


@pytest.mark.parametrize("overlap", ["silhouette", "base", "top"])
def test_overlap_choices(dev, mixed, overlap):
    dets, labels = mixed[0][:4], mixed[1][:4]
    want = e3.restated(dets, labels, 8, overlap=overlap)
    for path in ("ops", "cabi"):
        _same(PATHS[path](dev, dets, labels, 8, overlap=overlap), want, "%s/%s" % (path, overlap))
    if overlap != "silhouette":
        assert not np.array_equal(want["best_iou"], e3.restated(dets, labels, 8)["best_iou"])


@pytest.mark.parametrize("max_detections", [7, 8, 9])
def test_max_detections_below_at_and_above_k(dev, mixed, max_detections):
    dets, labels = mixed[0][3:4], mixed[1][3:4]
    assert len(dets[0][0]) == 8 + 2                                                 # K = 10: also cut at 9
    dets = [tuple(x[:8] for x in dets[0])]
    want = e3.restated(dets, labels, 8, max_detections=max_detections)
    assert len(want["rows"]) == min(8, max_detections)
    for path in ("ops", "cabi"):
        _same(PATHS[path](dev, dets, labels, 8, max_detections=max_detections), want, "%s/max %d" % (path, max_detections))


def test_one_class(dev):
    dets, labels = _dataset(32, [[(0, 6, 3)], [(0, 1, 1)], [(0, 2, 0)]], 1)
    want = e3.restated(dets, labels, 1)
    for path in sorted(PATHS):
        _same(PATHS[path](dev, dets, labels, 1), want, path + "/C=1")


@pytest.fixture(scope="module")
def group_sizes():
    """Groups of 0, 1, 63, 64 and 65 annotations and of 1, 64 and 65 rows; 64 rows x 65 annotations is one group, so that a
    row's pairs cross the wave's stride; 65 rows take a second chunk of table rows."""
    spec = [[(0, 1, 0), (1, 64, 1)], [(0, 65, 63)], [(0, 64, 65), (1, 3, 64)]]
    dets, labels = _dataset(37, spec, 2, jitter=2.0)
    return dets, labels, e3.restated(dets, labels, 2, max_detections=200)


@pytest.mark.parametrize("path", ["ops", "cabi"])
def test_group_sizes_around_the_wave(dev, group_sizes, path):
    dets, labels, want = group_sizes
    sizes = sorted((int(np.sum(want["rows"][b:e, 5] == c)), int(np.sum(labels[i][:, 20] == c)))
                   for i, (b, e) in enumerate(want["img_rows"]) for c in range(2))
    assert sizes == sorted([(1, 0), (64, 1), (65, 63), (0, 0), (64, 65), (3, 64)])
    assert want["best_ann"].max() == 64 and want["tp"][0].sum() > 60
    _same(PATHS[path](dev, dets, labels, 2, max_detections=200), want, path + "/group sizes")


# ------------------------------------------------------------------------------------------------ the module
def test_evaluate_cuboids_returns_the_restated_numbers_twice(dev, mixed):
    from retinanet_mi355x import eval3d
    dets, labels = mixed[0][:4], mixed[1][:4]
    want = e3.restated(dets, labels, 8)
    tdets = [_t(dev, d) for d in dets]
    res = eval3d.evaluate_cuboids(tdets, labels, 8)
    batched = np.full((4, 12, 27), -1.0)
    for i, l in enumerate(labels):
        batched[i, :len(l), :21] = l
    assert res == eval3d.evaluate_cuboids(tdets, torch.from_numpy(batched).to(dev), 8)        # the loader's batched layout
    exp = e3.summary(want, (0.5, 0.7))
    assert res["errors"] == exp["errors"] and sorted(res) == ["ap", "errors", "mAP"] and sorted(res["ap"]) == [0.5, 0.7]
    assert sum(v["tp"] for v in res["errors"].values()) == int(want["tp"][0].sum()) > 0
    for t, thr in enumerate((0.5, 0.7)):
        for c in range(8):
            assert res["ap"][thr][c][1] == exp["ap"][thr][c][1]
            assert abs(res["ap"][thr][c][0] - exp["ap"][thr][c][0]) <= ec.ap_bound(want["tp_count"][t, c])
        assert abs(res["mAP"][thr] - exp["mAP"][thr]) <= ec.ap_bound(want["tp_count"][t].max())
    assert res["ap"][0.5][7] == (0, 0) and isinstance(res["mAP"][0.5], float)
    with pytest.raises(RuntimeError, match="label"):
        eval3d.evaluate_cuboids([_t(dev, d) for d in mixed[0]], mixed[1], 8)


def test_rectangles_agree_with_the_2d_evaluation(dev):
    """Where the cuboid is a rectangle (top equals base) the silhouette is the box of columns 16:20: the TP flags are those of
    csv_eval's matching, and the AP at 0.5 is evaluate_detections' AP."""
    from retinanet_mi355x import csv_eval, eval3d, ops
    det, ann = e3.fuzz_pairs(n=300, seed=7, rectangles=True)
    C, per = 3, 10
    rng = np.random.RandomState(8)
    dets, labels, anns2d = [], [], []
    for i in range(0, 300, per):
        cls = rng.randint(0, C, per)
        scores = rng.permutation(per).astype(np.float32) / 16 + 0.1
        dets.append(e3.det_rows([(scores[k], cls[k], det[i + k]) for k in range(per)]))
        labels.append(e3.labels_of(*[e3.label(ann[i + k], cls[k]) for k in range(per)]))
        anns2d.append([labels[-1][labels[-1][:, 20] == c][:, 16:20] for c in range(C)])
    got = _via_ops(dev, dets, labels, C)
    table, img_rows, state = ops.eval_table(300, len(dets), dev)
    for i, d in enumerate(dets):
        ops.eval_select(*_t(dev, d), table, img_rows, state, i, C)
    ab, ao = ec.pack_annotations(anns2d, C)
    for t, thr in enumerate((0.5, 0.7)):
        tp2d, _ = ops.eval_match(table, img_rows, torch.from_numpy(ab).to(dev), torch.from_numpy(ao).to(dev), C, thr)
        assert np.array_equal(got["tp"][t], tp2d.cpu().numpy())
    assert 60 < got["tp"][0].sum() < 290 and got["tp"][1].sum() < got["tp"][0].sum()
    tdets = [_t(dev, d) for d in dets]
    assert eval3d.evaluate_cuboids(tdets, labels, C)["ap"][0.5] == csv_eval.evaluate_detections(tdets, anns2d, C)


class _Recorder(torch.nn.Module):
    """Keeps what the model returned, so that both entry points see the same outputs."""
    def __init__(self, net):
        super().__init__()
        self.net, self.outs = net, []

    def forward(self, x):
        out = self.net(x)
        self.outs.append(out)
        return out


def _net(dev, bias=3.0):
    from retinanet_mi355x import modules
    _, sd, img, ann = gc.model_case("resnet18", True)
    net = modules.resnet18(num_classes=4, directional=True)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    with torch.no_grad():
        net.classificationModel.output.bias.add_(bias)                                 # scores above 0.05
    return net, img, ann


def test_evaluate_3d_end_to_end(dev):
    """evaluate_3d with a directional ResNet-18 on two small frames equals evaluate_cuboids on the same model outputs; the
    annotations are some of the model's own boxes, so that there are true positives."""
    from retinanet_mi355x import eval3d
    net, img, _ = _net(dev)
    with torch.no_grad():
        first = [net(img[i:i + 1].to(dev)) for i in range(2)]
    assert all(o[2].dim() == 2 and o[2].shape[1] == 20 and o[0].numel() > 0 for o in first)
    label = torch.full((2, 8, 27), -1.0)
    for i, (s, l, b) in enumerate(first):
        l, b = l.cpu(), b.cpu()
        k = 0
        for c in range(4):
            for row in b[l == c][:2]:
                label[i, k, :20], label[i, k, 20] = row, float(c)
                k += 1
    net.train()
    rec = _Recorder(net)
    got = eval3d.evaluate_3d([(img, label)], rec, num_classes=4)
    assert len(rec.outs) == 2 and not net.training
    want = eval3d.evaluate_cuboids(rec.outs, label, 4)
    assert got == want and sum(v["tp"] for v in got["errors"].values()) > 0
    assert any(v[0] > 0 for v in got["ap"][0.7].values()) and max(v["corner_px"] for v in got["errors"].values()) < 0.01
    assert got == eval3d.evaluate_3d([(img[:1], label[:1]), (img[1:].to(dev), label[1:].to(dev))], net)      # num_classes from the model


def test_validator_lands_in_the_training_history(dev):
    from retinanet_mi355x import eval3d, trainer
    net, img, ann = _net(dev)
    img, ann = img.to(dev), ann.to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-5)
    logs = []
    hist = trainer.train(net, opt, None, lambda epoch: [(img, ann)], 1, clip_norm=0.1, log=logs.append,
                         validate=eval3d.validator(lambda epoch: [(img, ann)], num_classes=4, iou_thresholds=(0.5,)))
    v = hist[0]["validation"]
    assert sorted(v) == ["ap", "errors", "mAP"] and sorted(v["ap"]) == [0.5] and sorted(v["errors"]) == [0, 1, 2, 3]
    assert sum(x[1] for x in v["ap"][0.5].values()) == float((ann[:, :, 20] != -1).sum())
    assert any("validation" in m and "mAP" in m for m in logs) and hist[0]["iterations"] == 1

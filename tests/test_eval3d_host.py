"""CPU: the restatement of the 3D validation (tests/eval3d_cases.py) against hand-computed scenes, its mutations, and
exact rational arithmetic; the host side of retinanet_mi355x/eval3d.py.  The GPU tests compare the kernels with this
restatement bit for bit, so this file is what ties them to the definitions."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import eval3d_cases as e3


@pytest.fixture(scope="module")
def scene_results():
    return {name: e3.restated(s["dets"], s["labels"], s["C"], **s["kw"]) for name, s in e3.scenes().items()}


def test_scenes_have_their_closed_form_values(scene_results):
    for name, s in e3.scenes().items():
        got = scene_results[name]
        assert got["status"] == 0, name
        assert got["best_ann"].tolist() == s["best_ann"], name
        assert got["tp"].tolist() == s["tp"], name
        if "best_iou" in s:
            assert got["best_iou"].tolist() == s["best_iou"], (name, got["best_iou"])         # exact equality
        if "n_hull" in s:
            assert got["n_hull"].tolist() == s["n_hull"], name
        if "sums" in s:
            assert got["sums"].tolist() == s["sums"], name
        if "reversed" in s:
            assert got["sums"][:, 4].tolist() == s["reversed"], name
        if "corner_px" in s:
            assert got["sums"][:, 2].tolist() == s["corner_px"] and got["sums"][:, 3].tolist() == s["corner_rel"], name


def test_reversed_box_keeps_its_silhouette_and_is_counted(scene_results):
    got = scene_results["reversed"]
    assert got["best_iou"].tolist() == [1.0] and got["sums"][0, 4] == 1.0 and got["sums"][0, 0] == 1.0
    assert got["terms"][0, 3] == 0.0 and got["terms"][0, 1] > 1.0                # it fits turned, not straight
    assert e3.summary(got, (0.5, 0.7))["errors"][0]["reversed"] == 1


def test_non_finite_corners_give_no_overlap(scene_results):
    got = scene_results["non_finite"]
    assert got["best_iou"].tolist() == [0.0] * 4 and not got["tp"].any() and not np.isnan(got["sums"]).any()


@pytest.mark.parametrize("name", sorted(e3.MUTATIONS))
def test_each_mutation_is_caught_by_its_scene(scene_results, name):
    kw, scene, key = e3.MUTATIONS[name]
    s = e3.scenes()[scene]
    mutated = e3.restated(s["dets"], s["labels"], s["C"], **dict(s["kw"], **kw))
    assert not np.array_equal(mutated[key], scene_results[scene][key]), (name, scene, key)


@pytest.mark.parametrize("overlap", ["base", "top"])
def test_overlap_subsets(overlap):
    """The hexagon cuboid against itself moved up by 4: its base is where the other's top is."""
    up = [v - (4 if k % 2 else 0) for k, v in enumerate(e3.HEXAGON)]
    det, lab = e3.det_rows([(0.9, 0, up)]), e3.labels_of(e3.label(e3.HEXAGON))
    got = e3.restated([det], [lab], 1, overlap=overlap)
    base_on_top = e3.pair_iou(e3._points(up, "base"), e3._points(e3.HEXAGON, "top"))[0]
    assert base_on_top == 1.0 and got["best_iou"][0] == 0.0                     # the parallelograms 4 apart do not meet
    same = e3.restated([e3.det_rows([(0.9, 0, e3.HEXAGON)])], [lab], 1, overlap=overlap)
    assert same["best_iou"][0] == 1.0 and same["n_hull"][0] == 4


@pytest.fixture(scope="module")
def fuzz():
    det, ann = e3.fuzz_pairs()
    got = np.array([e3.pair_iou(e3._points(d, "silhouette"), e3._points(a, "silhouette"))[0] for d, a in zip(det, ann)])
    exact = [e3.exact_iou(e3._points(d, "silhouette"), e3._points(a, "silhouette")) for d, a in zip(det, ann)]
    return det, ann, got, exact


def test_fuzz_set_is_what_it_says(fuzz):
    det, ann, got, exact = fuzz
    assert len(det) == 3000 and ann[:, 0::2].min() >= 0 and ann[:, 0::2].max() <= 1920 and ann[:, 1::2].max() <= 1080
    same = [i for i in range(3000) if i % 10 == 3 and i % 17 != 5]
    assert all(np.array_equal(det[i], ann[i].astype(np.float32)) for i in same) and min(got[i] for i in same) > 0.999
    assert all(exact[i] == 0 for i in range(3000) if i % 17 == 5)
    assert 0.2 < np.mean(got >= 0.5) < 0.9 and 0.1 < np.mean(got >= 0.7) < 0.8       # both sides of both thresholds


def test_restated_against_exact_rational_arithmetic(fuzz):
    _, _, got, exact = fuzz
    err = np.array([abs(float(Fraction(float(v)) - x)) for v, x in zip(got, exact)])
    print("fuzz: max |restated - exact| = %.3e (recorded %.3e, bound %.3e)" % (err.max(), e3.FUZZ_MAX_ERROR, e3.FUZZ_BOUND))
    assert e3.FUZZ_BOUND == 8.0 * e3.FUZZ_MAX_ERROR
    assert err.max() <= e3.FUZZ_BOUND
    left_out = 0
    for thr in (0.5, 0.7):
        t = Fraction(thr)
        for v, x in zip(got, exact):
            if abs(x - t) <= Fraction(e3.FUZZ_BOUND):
                left_out += 1
                continue
            assert (v >= thr) == (x >= t)
    print("fuzz: %d pairs within the bound of a threshold" % left_out)
    assert left_out <= 0.01 * len(got)


# ------------------------------------------------------------------------------------------------ the module's host side
def test_split_labels_takes_the_loader_layouts():
    from retinanet_mi355x import eval3d
    batch = torch.zeros(2, 3, 27)
    batch[:, :, 20] = -1
    batch[0, 0, 20], batch[1, 1, 20], batch[1, 2, 20] = 2, 0, 1
    per = eval3d.split_labels(batch)
    assert [p.shape for p in per] == [(1, 27), (2, 27)] and per[0].dtype == np.float64
    per = eval3d.split_labels([batch, np.zeros((0, 21)), np.ones((4, 21))])
    assert [p.shape[0] for p in per] == [1, 2, 0, 4]
    corners, off = eval3d._pack_labels(eval3d.split_labels(batch), 3)
    assert corners.shape == (3, 16) and off.tolist() == [0, 0, 0, 1, 2, 3, 3]
    ours, theirs = e3.pack_labels(eval3d.split_labels(batch), 3)
    assert np.array_equal(ours, corners) and np.array_equal(theirs, off)
    with pytest.raises(RuntimeError, match="class"):
        eval3d._pack_labels(eval3d.split_labels(batch), 2)
    with pytest.raises(RuntimeError):
        eval3d.split_labels([np.zeros((2, 5))])


def test_operators_limits_and_reexport_are_declared():
    from retinanet_mi355x import eval3d, ops, torch_ops
    for name in ("eval_corners", "eval_cuboid_overlap", "eval_cuboid_assign", "eval_cuboid_errors"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name) and hasattr(ops, name)
    assert ops.EVAL_CUBOID_MAX_VERTS == e3.MAX_VERTS and sorted(ops.EVAL_CUBOID_OVERLAPS) == sorted(e3.SUBSETS)
    assert ops.EVAL_CUBOID_TERMS == e3.TERMS and ops.EVAL_CUBOID_SUMS == e3.SUMS
    import retinanet.eval3d as mirror
    assert mirror.evaluate_cuboids is eval3d.evaluate_cuboids and mirror.validator is eval3d.validator
    with pytest.raises(RuntimeError):
        ops.eval_cuboid_overlap(*[torch.zeros(1)] * 5, 1)
    with pytest.raises(RuntimeError, match="overlap"):
        eval3d.evaluate_cuboids([(torch.zeros(0),) * 3], [np.zeros((0, 21))], 1, overlap="volume")


def test_validator_hands_the_epoch_on():
    from retinanet_mi355x import eval3d
    seen = []

    def batches(epoch):
        seen.append(epoch)
        return []
    validate = eval3d.validator(batches, num_classes=1)
    with pytest.raises(RuntimeError):                                            # no GPU here: the table refuses a CPU device
        validate(torch.nn.Linear(1, 1), 3)
    assert seen == [3]

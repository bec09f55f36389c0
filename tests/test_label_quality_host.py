"""CPU: the plain restatement of the label scores (tests/label_quality_cases.py) against the reference's own numbers
(tests/golden/label_quality.npz, written by tools/make_golden_label_quality.py): bit for bit wherever only IEEE operations are
involved, within the derived bounds for theta (atan2) and the RMSE (summation order)."""
import os

import numpy as np
import pytest

import label_quality_cases as qc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_quality.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, scene in qc.golden_scenes().items():
        out.update(qc.restated(name, scene))
    return out


def test_golden_holds_what_the_restatement_writes(golden, restated):
    assert sorted(golden) == sorted(restated)
    for k in golden:
        assert golden[k].shape == restated[k].shape and golden[k].dtype == restated[k].dtype, k


@pytest.mark.parametrize("key", ["x_var", "x_range", "feasible", "ids", "off", "time", "v", "a", "rmse_counts"])
def test_exact_figures(golden, restated, key):
    for name in qc.golden_scenes():
        assert np.array_equal(golden[name + "_" + key], restated[name + "_" + key]), (name, key)


def test_theta_within_the_atan2_bound(golden, restated):
    for name in qc.golden_scenes():
        want, got = golden[name + "_theta"], restated[name + "_theta"]
        bound = np.array([qc.theta_bound(t) for t in want])
        assert len(want) > 100 and np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))


def test_rmse_within_the_summation_bound(golden, restated):
    for name in qc.golden_scenes():
        want, got = golden[name + "_rmse_groups"], restated[name + "_rmse_groups"]
        counts, largest = golden[name + "_rmse_counts"], golden[name + "_rmse_largest"]
        assert len(want) == 3 and np.all(want > 0)
        for g in range(len(want)):
            assert abs(got[g] - want[g]) <= qc.rmse_bound(int(counts[g]), float(largest[g])), g
        assert abs(restated[name + "_rmse"][0] - golden[name + "_rmse"][0]) <= qc.rmse_bound(int(counts.max()), float(largest.max()))


def test_the_scene_holds_what_it_is_scripted_for():
    """Dropped and kept overlap rows, a camera that runs backwards, -0.0, both directions, an ignored id."""
    scene = qc.golden_scenes()["score"]
    offsets, cols, _ = qc.table(scene["data"], scene["names"])
    C = len(scene["names"])
    assert (len(offsets) - 1) // C == 15 and any(item["id"] == 17 for fd in scene["data"] for item in fd.values())
    per = qc.series_table(offsets, cols, C)[5]
    assert any(0 < sum(s["keep"]) < s["n"] for s in per)                       # some rows dropped, some kept
    t13 = cols[offsets[13 * C + 2]:offsets[13 * C + 3], 2]
    assert np.any(np.diff(t13) < 0) and per[13]["order"] != sorted(per[13]["order"])
    assert any(v == 0.0 and np.signbit(v) for v in per[12]["v"])
    assert per[14]["m"] == 1 and per[14]["variation"] == 0.0
    assert all(y < 60 for y in per[0]["y"]) and all(y > 60 for y in per[5]["y"])
    fr = qc.ref_feasibility(qc.rc.Labels(scene))
    assert len(fr) == 14 and any(0 < f < 1 for f in fr)


def test_exact_ties_keep_the_camera_outer_order():
    rows = [(0.0, 0.0, 1.0), (1.0, 0.0, 0.5), (2.0, 0.0, 1.0), (3.0, 0.0, 0.5)]
    s = qc.series(rows)
    assert s["order"] == [1, 3, 0, 2] and s["keep"] == [1, 0, 1, 0] and s["x"] == [1.0, 0.0]

"""CPU: the numpy restatement of csv_eval.evaluate (tests/eval_cases.py) against the reference's own results in
tests/golden/csv_eval.npz and against hand-computed edge cases; every mutation of it is caught by a named case; the
trainer's ``validate`` hook.  The GPU tests compare the kernels with this restatement, so this file is what ties them to
the reference."""
import numpy as np
import pytest
import torch

import eval_cases as ec


@pytest.mark.parametrize("name", sorted(ec.GOLDEN))
def test_restatement_reproduces_the_reference_bit_for_bit(golden, name):
    g = golden("csv_eval")
    dets, anns, C, kw = ec.unpack_golden(g, name)
    r = ec.restated(dets, anns, C, **kw)
    assert r["status"] == ec.OK
    assert np.array_equal(r["ap"], g[name + "_ap"]), (r["ap"], g[name + "_ap"])                 # np.sum, as the reference
    assert np.array_equal(r["num_annotations"].astype(np.float64), g[name + "_num_annotations"])
    assert len(r["rows"]) > 500 and r["tp_count"].min() > 0


def test_golden_inputs_are_what_the_generator_makes_and_scores_are_unique(golden):
    g = golden("csv_eval")
    for name, p in ec.GOLDEN.items():
        dets, anns = ec.golden_inputs(name)
        for k, v in ec.pack_golden(dets, anns, p["classes"]).items():
            assert np.array_equal(v, g[name + "_" + k]), (name, k)
        s = g[name + "_det_scores"]
        assert len(np.unique(s)) == len(s)                          # the reference's unstable sorts have no freedom


@pytest.mark.parametrize("name", sorted(ec.edge_cases()))
def test_edge_case_expectation(name):
    c = ec.edge_cases()[name]
    r = ec.restated(c["dets"], c["anns"], c["C"], **c["kw"])
    assert r["tp"].tolist() == c["tp"]
    assert r["ap"].tolist() == c["ap"]
    assert r["num_annotations"].tolist() == c["num_annotations"]
    assert not np.isnan(r["ap"]).any()


@pytest.mark.parametrize("mutation", sorted(ec.MUTATIONS))
def test_mutation_is_caught(mutation):
    kw, name = ec.MUTATIONS[mutation]
    c = ec.edge_cases()[name]
    args = dict(c["kw"])
    args.update(kw)
    r = ec.restated(c["dets"], c["anns"], c["C"], **args)
    assert (r["tp"].tolist(), r["ap"].tolist(), r["num_annotations"].tolist()) != (c["tp"], c["ap"], c["num_annotations"])


def test_status_rules_of_the_selection():
    """A selected label outside [0, C) or a full table: a status bit and the image appends nothing; a bad label that the
    selection drops is harmless."""
    d_ok = (np.array([0.9], np.float32), np.array([0]), np.array([[0, 0, 4, 4]], np.float32))
    d_bad = (np.array([0.9, 0.8], np.float32), np.array([0, 2]), np.array([[0, 0, 4, 4]] * 2, np.float32))
    anns = [[np.zeros((0, 4))] * 3] * 2
    r = ec.restated([d_bad, d_ok], anns, 2)
    assert r["status"] == ec.BAD_LABEL and r["img_rows"].tolist() == [[0, 0], [0, 1]] and len(r["rows"]) == 1
    assert ec.restated([d_bad, d_ok], anns, 2, max_detections=1)["status"] == ec.OK
    r = ec.restated([d_ok, d_bad], anns, 3, table_rows=2)
    assert r["status"] == ec.TABLE_FULL and len(r["rows"]) == 1


def test_host_helpers_of_the_drop_in_match_the_restatement():
    from retinanet_mi355x import csv_eval
    rng = np.random.RandomState(0)
    a = rng.uniform(0, 50, (5, 2))
    a = np.concatenate((a, a + rng.uniform(1, 30, (5, 2))), 1)
    b = rng.uniform(0, 50, (7, 2))
    b = np.concatenate((b, b + rng.uniform(1, 30, (7, 2))), 1)
    got = csv_eval.compute_overlap(a, b)
    assert got.shape == (5, 7)
    for i in range(5):
        assert np.array_equal(got[i], ec.overlap(a[i], b))
    flags = rng.rand(50) < 0.4
    tps, fps = np.cumsum(flags), np.cumsum(~flags)
    assert csv_eval._compute_ap(tps / 30.0, tps / np.maximum(tps + fps, ec.EPS)) == ec.ap_from_flags(flags, 30.0)
    buf, n_off, head, M = csv_eval._pack_annotations([[np.zeros((0, 5)), np.array([[1., 2, 3, 4, 9]])]], 2)
    assert (n_off, M, head) == (3, 1, 16) and buf[:12].view(np.int32).tolist() == [0, 0, 1]
    assert buf[head:].view(np.float64).tolist() == [1, 2, 3, 4]


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(6, 3)

    def forward(self, inputs):
        x, y = inputs
        d = (self.a(x) - y) ** 2
        return d.mean().reshape(1), d.sum().reshape(1) * 0.1, d.abs().mean().reshape(1)


def _batches(epoch):
    g = torch.Generator().manual_seed(epoch)
    for _ in range(2):
        yield torch.randn(4, 6, generator=g), torch.randn(4, 3, generator=g)


def test_trainer_validate_lands_in_the_history():
    from retinanet_mi355x import trainer
    torch.manual_seed(0)
    net = _Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    seen, logs = [], []

    def validate(n, epoch):
        seen.append((epoch, n is net, n.training, torch.is_grad_enabled()))
        return {0: (0.25 + epoch, 3.0)}
    hist = trainer.train(net, opt, None, _batches, 2, log=logs.append, validate=validate)
    assert seen == [(0, True, False, False), (1, True, False, False)]          # under eval() and no_grad()
    assert [h["validation"] for h in hist] == [{0: (0.25, 3.0)}, {0: (1.25, 3.0)}]
    assert any("validation" in m and "0.25" in m for m in logs)
    assert all(np.isfinite(h["mean_loss"]) and h["iterations"] == 2 for h in hist)


def test_trainer_without_validate_is_unchanged():
    from retinanet_mi355x import trainer
    torch.manual_seed(0)
    net = _Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    logs = []
    hist = trainer.train(net, opt, None, _batches, 1, log=logs.append)
    assert sorted(hist[0]) == ["epoch", "iterations", "lr", "mean_loss", "skipped"]
    assert not any("validation" in m for m in logs)
    torch.manual_seed(0)
    twin = _Net()
    hist2 = trainer.train(twin, torch.optim.SGD(twin.parameters(), lr=0.01), None, _batches, 1, log=lambda m: None,
                          validate=lambda n, e: {})
    assert hist2[0]["mean_loss"] == hist[0]["mean_loss"]                       # the training itself does not change
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), twin.parameters()))


def test_eval_operators_and_limits_are_declared():
    from retinanet_mi355x import ops, torch_ops
    for name in ("eval_select", "eval_match", "eval_ap"):
        assert name in torch_ops.OPERATORS
    assert (ops.EVAL_OK, ops.EVAL_TOO_MANY, ops.EVAL_BAD_LABEL, ops.EVAL_TABLE_FULL) == (ec.OK, ec.TOO_MANY, ec.BAD_LABEL, ec.TABLE_FULL)
    assert ops.EVAL_MAX_K == ec.MAX_K
    with pytest.raises(RuntimeError):
        ops.eval_table(4, 1, "cpu")

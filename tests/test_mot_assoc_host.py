"""CPU: the restatement of the identity and association scores (tests/mot_assoc_cases.py) against the closed forms and against an
independent vectorised form of the same definitions, written the way the published evaluators write them (sum(0) / sum(1),
fancy-index +=, the padded (G+P)^2 identity problem); the alpha table, key names, defaults, and that MOT_Evaluator without the
new keys is unchanged.

Tolerances.  Integers are equal and every frame's matched pairs are identical (a condition of the fixtures: seeds are chosen so
that it holds).  The fp64 sums (Loc_k, the three association sums) then add the same terms in two orders; for a non-negative sum
of n terms two orderings differ by at most 2 n 2^-53 relative to first order, n = the terms that are not zero.  A per-alpha
figure adds a quotient (and HOTA a product and a root): 8 more units of 2^-53; a mean over the 19 alphas 2 * 19 more.
"""
import inspect

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import mot_assoc_cases as ac

U = 2.0 ** -53
CLOSED = ac.closed_form_scenes()
EDGE = ac.edge_scenes()


def vectorised(scene, id_iou=0.5):
    """The published evaluators' formulation: two passes over the frames, numpy reductions in numpy's own order."""
    gids, gmap = ac.dense_ids(scene["gt_ids"])
    pids, pmap = ac.dense_ids(scene["pred_ids"])
    G, P, K = len(gmap), len(pmap), len(ac.ALPHAS)
    eps = np.finfo("float").eps
    potential, id_pot = np.zeros((G, P)), np.zeros((G, P))
    gt_count, tr_count = np.zeros((G, 1)), np.zeros((1, P))
    for t, (g, p) in enumerate(zip(gids, pids)):
        gt_count[g] += 1
        tr_count[0, p] += 1
        if len(g) and len(p):
            sim = scene["ious"][t]
            den = sim.sum(0)[np.newaxis, :] + sim.sum(1)[:, np.newaxis] - sim
            sim_iou = np.zeros_like(sim)
            mask = den > 0 + eps
            sim_iou[mask] = sim[mask] / den[mask]
            potential[g[:, np.newaxis], p[np.newaxis, :]] += sim_iou
            id_pot[g[:, np.newaxis], p[np.newaxis, :]] += np.greater_equal(sim, id_iou)
    # identity: the padded problem
    fp_mat, fn_mat = np.zeros((G + P, G + P)), np.zeros((G + P, G + P))
    fp_mat[G:, :P] = 1e10
    fn_mat[:G, P:] = 1e10
    for g in range(G):
        fn_mat[g, :P] = gt_count[g, 0]
        fn_mat[g, P + g] = gt_count[g, 0]
    for p in range(P):
        fp_mat[:G, p] = tr_count[0, p]
        fp_mat[p + G, p] = tr_count[0, p]
    fn_mat[:G, :P] -= id_pot
    fp_mat[:G, :P] -= id_pot
    r, c = linear_sum_assignment(fn_mat + fp_mat)
    IDFN, IDFP = int(fn_mat[r, c].sum()), int(fp_mat[r, c].sum())
    IDTP = int(gt_count.sum()) - IDFN
    # HOTA
    ga = potential / (gt_count + tr_count - potential)
    TP, FN, FP, loc = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros(K)
    counts = [np.zeros((G, P)) for _ in range(K)]
    pairs = []
    for t, (g, p) in enumerate(zip(gids, pids)):
        if len(g) == 0:
            FP += len(p)
            continue
        if len(p) == 0:
            FN += len(g)
            continue
        sim = scene["ious"][t]
        score = ga[g[:, np.newaxis], p[np.newaxis, :]] * sim
        rows, cols = linear_sum_assignment(-score)
        pairs.append((t, rows.tolist(), cols.tolist()))
        for a, alpha in enumerate(ac.ALPHAS):
            ok = sim[rows, cols] >= alpha - eps
            m = int(ok.sum())
            TP[a] += m
            FN[a] += len(g) - m
            FP[a] += len(p) - m
            if m:
                loc[a] += sum(sim[rows[ok], cols[ok]])
                counts[a][g[rows[ok]], p[cols[ok]]] += 1
    a_sum, re_sum, pr_sum = np.zeros(K), np.zeros(K), np.zeros(K)
    for a in range(K):
        mcnt = counts[a]
        a_sum[a] = np.sum(mcnt * (mcnt / np.maximum(1, gt_count + tr_count - mcnt)))
        re_sum[a] = np.sum(mcnt * (mcnt / np.maximum(1, gt_count)))
        pr_sum[a] = np.sum(mcnt * (mcnt / np.maximum(1, tr_count)))
    fig, per = ac.figures(TP, FN, FP, loc, a_sum, re_sum, pr_sum)
    fig.update(IDR=IDTP / np.maximum(1.0, IDTP + IDFN), IDP=IDTP / np.maximum(1.0, IDTP + IDFP),
               IDF1=IDTP / np.maximum(1.0, IDTP + 0.5 * IDFP + 0.5 * IDFN))
    return dict(fig, IDTP=IDTP, IDFN=IDFN, IDFP=IDFP, TP=TP, FN=FN, FP=FP, loc=loc, a_sum=a_sum, re_sum=re_sum, pr_sum=pr_sum,
                pairs=pairs, per_alpha=per, counts=counts, C=id_pot.astype(np.int64), gc=gt_count[:, 0].astype(np.int64),
                pc=tr_count[0].astype(np.int64), pot=potential)


def _close(a, b, units):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= units * U * np.maximum(np.abs(a), np.abs(b))))


def test_alpha_table():
    assert len(ac.ALPHAS) == ac.N_ALPHA == 19
    assert ac.ALPHAS.tobytes() == np.array([0.05 + k * 0.05 for k in range(19)], np.float64).tobytes()
    from retinanet_mi355x import ops
    assert ops.mot_alphas().tobytes() == ac.ALPHAS.tobytes() and ops.MOT_ALPHAS == 19
    assert ops.MOT_ASSOC_RESULT == 19 * 7 + 2 and ops.MOT_ASSOC_MAX_CELLS == ac.MAX_CELLS
    assert ac.prefix_length(0.5) == 10 and ac.prefix_length(0.0) == 0 and ac.prefix_length(1.0) == 19
    assert ac.prefix_length(0.05 - 2.0 ** -52) == 1 and ac.prefix_length(0.05 - 2.0 ** -51) == 0


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_restatement_reproduces_the_closed_forms(name):
    scene, want = CLOSED[name]
    got = ac.restated(scene)
    for key, w in want.items():
        if isinstance(w, int):
            assert got[key] == w and isinstance(got[key], int), key
        elif (w * 2.0 ** 20) % 1 == 0:                                   # dyadic: to the last bit
            assert got[key] == w, (key, got[key], w)
        else:                                                            # 1 ulp
            assert abs(got[key] - w) <= np.spacing(w), (key, got[key], w)
    per = ac.closed_form_per_alpha(name)
    for key in ("TP", "FN", "FP"):
        assert np.array_equal(got[key], per[key]), key
    assert got["HOTA(0)"] == got["per_alpha"]["HOTA"][0]


@pytest.mark.parametrize("name", sorted(EDGE) + sorted(CLOSED))
def test_restatement_agrees_with_the_vectorised_form(name):
    scene, id_iou = EDGE[name] if name in EDGE else (CLOSED[name][0], 0.5)
    a, b = ac.restated(scene, id_iou), vectorised(scene, id_iou)
    for key in ("IDTP", "IDFN", "IDFP"):
        assert a[key] == b[key], key
    for key in ("TP", "FN", "FP", "gc", "pc", "C"):
        assert np.array_equal(a[key], b[key]), key
    mine = {}
    for t, i, j, s, n, g, p in a["slots"]:
        mine.setdefault(t, ([], []))
        mine[t][0].append(i), mine[t][1].append(j)
    assert [(t, r, c) for t, (r, c) in sorted(mine.items())] == b["pairs"], "a frame's matched pairs differ: replace the seed"
    assert np.array_equal(a["M"], np.array(b["counts"]).astype(np.int64))
    nn = np.array([s[4] for s in a["slots"]], np.int64)
    for k in range(19):
        n_loc, n_cell = int((nn > k).sum()), int((a["M"][k] > 0).sum())
        assert _close(a["loc"][k], b["loc"][k], 2 * n_loc), ("Loc", k)
        for key in ("a_sum", "re_sum", "pr_sum"):
            assert _close(a[key][k], b[key][k], 2 * n_cell), (key, k)
        for key in ac.FIGURES:
            n = n_loc if key == "LocA" else n_cell
            assert _close(a["per_alpha"][key][k], b["per_alpha"][key][k], 2 * n + 8), (key, k)
    n_all = max(len(a["slots"]), a["C"].size)
    for key in ac.FIGURES + ("HOTA(0)", "IDF1", "IDP", "IDR"):
        assert _close(a[key], b[key], 2 * n_all + 8 + 2 * 19), key


def test_edge_scenes_reach_their_paths():
    shapes = {k: [(len(g), len(p)) for g, p in zip(s["gt_ids"], s["pred_ids"])] for k, (s, _) in EDGE.items()}
    assert any(a < b for a, b in shapes["transpose"]) and any(a > b for a, b in shapes["transpose"])
    assert max(max(a, b) for a, b in shapes["wide70"]) == 70
    r = {k: ac.restated(*EDGE[k]) for k in ("ids_tall", "ids_wide", "ids300", "ties", "on_id_iou", "absent")}
    assert r["ids_tall"]["C"].shape[0] > r["ids_tall"]["C"].shape[1] > 64
    assert r["ids_wide"]["C"].shape[1] > r["ids_wide"]["C"].shape[0] > 64
    assert min(r["ids300"]["C"].shape) >= 300
    C = r["ties"]["C"]
    assert any(len(set(row[row > 0].tolist())) < (row > 0).sum() for row in C)             # equal counts in a row of C
    s = EDGE["on_id_iou"][0]
    assert any((m == 0.5).any() for m in s["ious"] if m is not None)
    assert any(len(g) == 0 for g in EDGE["absent"][0]["gt_ids"]) and any(len(p) == 0 for p in EDGE["absent"][0]["pred_ids"])
    assert max(len(s["gt_ids"]) for s, _ in EDGE.values()) <= 60
    with pytest.raises(ValueError):
        ac.restated(ac.duplicate_scene())
    with pytest.raises(ValueError, match="invalid numeric entries"):
        ac.restated(ac.nan_scene())


def test_scene_rows_pack_to_the_scene():
    """The CSV rows built from a scene pack to the scene's counts, dense ids and flat IoU order."""
    scene, _ = EDGE["absent"]
    gt, pred, flat = ac.scene_rows(scene)
    gids, gmap = ac.dense_ids(scene["gt_ids"])
    assert sorted(set(gt) | set(pred)) == list(range(len(scene["gt_ids"])))
    assert [len(gt.get(t, ())) for t in range(len(gids))] == [len(g) for g in gids]
    assert [int(r[2]) for r in gt[0]] == list(scene["gt_ids"][0])
    assert len(flat) == sum(m.size for m in scene["ious"] if m is not None)
    from retinanet_mi355x import ops
    off, frame, row = ops.mot_id_csr([len(g) for g in scene["gt_ids"]], [len(p) for p in scene["pred_ids"]],
                                     np.concatenate(gids), len(gmap))
    assert off[0] == 0 and off[-1] == len(frame) == sum(len(g) for g, p in zip(gids, scene["pred_ids"]) if len(p))
    for g in range(len(gmap)):
        fr = frame[off[g]:off[g + 1]]
        assert np.all(np.diff(fr) > 0)
        assert all(gids[f][r] == g for f, r in zip(fr, row[off[g]:off[g + 1]]))


def test_names_defaults_and_unchanged_evaluator():
    import mot_evaluator as me
    from retinanet_mi355x import ops, torch_ops
    sig = inspect.signature(me.evaluate_association)
    assert list(sig.parameters) == ["gt_rows", "pred_rows", "homography", "cutoff_frame", "id_iou", "collect", "ious"]
    assert sig.parameters["cutoff_frame"].default == 10000 and sig.parameters["id_iou"].default == 0.5
    assert sig.parameters["collect"].default is False and sig.parameters["ious"].default is None
    for name in ("mot_id_counts", "mot_id_assign", "mot_hota_align", "mot_hota_assign", "mot_hota_reduce"):
        assert name in torch_ops.OPERATORS and hasattr(ops, name)
    # the figures from a result block, as the device would return it for the "half" scene
    want = ac.restated(CLOSED["half"][0])
    res = np.zeros(ops.MOT_ASSOC_RESULT + me.ASSOC_TAIL)
    blk = res[:19 * 7].reshape(19, 7)
    for k, key in enumerate(("TP", "FN", "FP", "loc", "a_sum", "re_sum", "pr_sum")):
        blk[:, k] = want[key]
    res[ops.MOT_ASSOC_RESULT - 1] = -1
    res[ops.MOT_ASSOC_RESULT:] = [want["IDTP"], 0, 0, -1, 0, -1]
    m = me.association_from_result(res, want["n_gt"], want["n_pred"])
    assert list(m) == list(me.ASSOC_SCALARS) + ["alphas", "per_alpha"]
    for key in me.ASSOC_SCALARS:
        assert m[key] == want[key], key
    assert m["alphas"].tobytes() == ac.ALPHAS.tobytes() and m["per_alpha"]["HOTA"].shape == (19,)
    res[ops.MOT_ASSOC_RESULT + 2] = ops.MOT_DUPLICATE_ID
    with pytest.raises(ValueError, match="twice"):
        me.association_from_result(res, 1, 1)
    # without the new keys the evaluator's metrics are the reference's: the same keys, in the same order
    blk = np.zeros(ops.MOT_RESULT)
    blk[:3] = (5, 1, 2)
    blk[16:49:3] = 5
    metrics, _ = me.metrics_from_result(blk, 0.5)
    assert list(metrics) == ["iou_threshold", "True unique objects", "Predicted unique objects", "TP", "FP", "FN", "FP edge-case",
                             "FP @ 0.2", "FN @ 0.2", "Recall", "Precision", "False Alarm Rate", "Fragmentations", "ID switches", "MOTA",
                             "MOTA edge-case", "MOTA @ 0.2", "Pre-threshold IOU", "Match IOU", "Width precision", "Height precision",
                             "Length precision", "Velocity precision", "X precision", "Y precision", "Bottom im precision",
                             "Top im precision"]
    assert not set(metrics) & set(me.ASSOC_SCALARS)
    src = inspect.getsource(me.MOT_Evaluator.evaluate)
    assert "if self.association:" in src
    with pytest.raises(RuntimeError, match="cells"):
        ops.mot_assoc_dims("test", 2048, 1024)

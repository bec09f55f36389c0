"""GPU: csrc/label_rebase.hip (ops.label_rebase / label_offset_y) and the public label_rewrite functions on top of it, against
the restatement of tests/label_rewrite_cases.py and the reference's own output (tests/golden/label_rewrite.npz).

Device against restatement is compared BIT FOR BIT -- centre, error and winning index: the kernel's arithmetic is fp64 with one
rounding per operation in the restatement's order, so there is no tolerance to choose.  Device against the reference: every
winning index equal, x and y bit-equal, the minimum errors within 1e-9 relative (the reference's matrix product is
torch.matmul's; tools/make_golden_label_rewrite.py keeps every round's two smallest errors 1e-6 apart, so no index can flip).

Shapes: 1, 63, 64 and 65 boxes (one wave per box, four waves per block: the last block is partly empty at each), grids of 8
(64 candidates: exactly one pass), 11 (121: a second pass with 7 idle lanes) and 16 (256: four full passes), one round and
three."""
import contextlib
import io
import pickle

import numpy as np
import pytest
import torch

import label_audit_cases as lc
import label_rewrite_cases as rc

pytestmark = pytest.mark.gpu
SCENES = rc.golden_scenes()
FUZZ_SEED = 8                                                   # 3 cameras, 41 frames, 6 ids, 99 manual boxes


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same(a, b):
    """bit_equal, but a NaN is a NaN whatever its bits (a box that was left out)."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and bit_equal(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


@pytest.fixture(scope="module")
def Me(dev):
    import homography
    import label_audit as la
    import label_rewrite as lw

    class Me(rc.Labels, la.LabelAudit, lw.LabelRewrite):
        def __init__(self, scene):
            rc.Labels.__init__(self, scene, homography.Homography, homography.Homography_Wrapper)

        def wrapper(self, spec):
            return rc.build_hg(spec, homography.Homography, homography.Homography_Wrapper)
    return Me


def table(spec, key):
    return np.stack([spec[key][n].reshape(12) for n in sorted(spec[key])])


def random_boxes(n, seed, n_cam=4):
    """Boxes of several cameras interleaved, both directions, some at y = 55 (their grid straddles the y > 60 switch)."""
    rng = np.random.RandomState(seed)
    cam = rng.randint(0, n_cam, n).astype(np.int32)
    kind = rng.randint(0, 3, n)
    y = np.where(kind == 0, rng.uniform(10, 50, n), np.where(kind == 1, 55.0 + rng.uniform(-1, 1, n), rng.uniform(70, 110, n)))
    state = np.stack([60.0 * cam - 15.0 + rng.uniform(0, 100, n), y, rng.uniform(12, 60, n), rng.uniform(5, 9, n),
                      rng.uniform(4, 13, n), np.where(y < 60, 1.0, -1.0)], axis=1)
    names = lc.camera_names(n_cam)
    old, new = rc.hg_spec(names, seed=seed + 1, scale=0.002), rc.hg_spec(names, seed=seed + 2, scale=0.04)
    return state, cam, [table(old, "P1"), table(old, "P2"), table(new, "P1"), table(new, "P2")]


def on_device(dev, state, cam, tables, rads, grid):
    from retinanet_mi355x import ops
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ops.label_rebase(up(state), up(np.asarray(cam, np.int32)), *(up(t) for t in tables), up(np.array(rads, np.float64)), grid)
    return [t.cpu().numpy() for t in got]


def same_as_restatement(dev, state, cam, tables, rads=None, grid=rc.GRID, status=0):
    rads = rc.radii() if rads is None else rads
    centre, err, idx, st = on_device(dev, state, cam, tables, rads, grid)
    w_centre, w_err, w_idx, every = rc.rebase_boxes(state, cam, *tables, rads=rads, grid=grid)
    assert int(st[0]) == status
    assert bit_equal(idx, w_idx) and same(centre, w_centre) and same(err, w_err)
    return centre, err, idx, every


@pytest.mark.parametrize("grid,rounds", [(11, 3), (8, 1), (16, 3), (8, 3), (11, 1)])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_rebase_equals_the_restatement_bit_for_bit(dev, n, grid, rounds):
    state, cam, tables = random_boxes(n, seed=10 * n + grid)
    centre, err, idx, _ = same_as_restatement(dev, state, cam, tables, rc.radii()[:rounds], grid)
    assert idx.shape == (n, rounds) and idx.min() >= 0 and idx.max() < grid * grid and np.isfinite(err).all()
    if n >= 63:
        assert len(set(cam.tolist())) == 4 and len(set(idx[:, 0].tolist())) > 1 and (np.abs(centre - state[:, :2]) > 0).any()
        assert idx.max() >= 64 or grid == 8                     # winners of the second pass


def test_equal_errors_go_to_the_lower_index(dev):
    state, cam, tables = random_boxes(9, seed=3)
    for t in tables[2:]:
        t[:, [1, 5, 9]] = 0.0                                   # the new image ignores y: the candidates of one ix tie
    tables[3] = None
    centre, err, idx, every = same_as_restatement(dev, state, cam, tables)
    e = every[0][0].reshape(rc.GRID, rc.GRID)
    assert (e == e[:, :1]).all() and (idx % rc.GRID == 0).all()
    assert bit_equal(centre[:, 1], ((state[:, 1] - 50) - 10.0) - 2.0)


def test_a_grid_that_straddles_the_switch_mixes_both_matrices(dev):
    state, cam, tables = random_boxes(8, seed=4)
    state[:, 1], state[:, 5], state[:, 3] = 55.0, 1.0, 6.0
    centre, err, idx, _ = same_as_restatement(dev, state, cam, tables)
    corner = (rc.linspace(5.0, 105.0, rc.GRID) - 3.0).astype(np.float32)
    assert 0 < (corner > 60).sum() < rc.GRID and not bit_equal(tables[2], tables[3])
    single, _, idx1, _ = same_as_restatement(dev, state, cam, tables[:3] + [None])
    other, _, idx2, _ = same_as_restatement(dev, state, cam, [tables[0], tables[1], tables[3], None])
    assert not bit_equal(single, other)
    assert not bit_equal(centre, single) or not bit_equal(centre, other)       # the wrapper is neither side alone


def test_without_a_second_matrix_there_is_no_switch(dev):
    state, cam, tables = random_boxes(20, seed=5)
    for keep in ((0, None, 2, None), (0, 1, 2, None), (0, None, 2, 3)):
        same_as_restatement(dev, state, cam, [None if k is None else tables[k] for k in keep])


def test_the_same_homography_keeps_every_centre(dev):
    state, cam, tables = random_boxes(30, seed=6)
    state[:, :5] = np.round(state[:, :5] * 4) / 4               # exact in float32, so both corner rules agree
    centre, err, idx, _ = same_as_restatement(dev, state, cam, tables[:2] + tables[:2])
    assert (idx == 60).all() and (err == 0.0).all() and bit_equal(centre, state[:, :2].copy())


def test_a_bad_camera_or_error_sets_its_bit_and_leaves_only_that_box_out(dev):
    from retinanet_mi355x import ops
    state, cam, tables = random_boxes(6, seed=7, n_cam=3)
    cam[:] = (0, 3, 2, -1, 1, 2 ** 30)
    centre, err, idx, _ = same_as_restatement(dev, state, cam, tables, status=ops.LABEL_BAD_CAMERA)
    out = np.array([False, True, False, True, False, True])
    assert np.isnan(centre[out]).all() and np.isnan(err[out]).all() and (idx[out] == -1).all()
    assert np.isfinite(centre[~out]).all() and (idx[~out] >= 0).all()
    with pytest.raises(RuntimeError, match="camera index outside"):
        ops.label_check(ops.LABEL_BAD_CAMERA)
    cam[:] = (0, 1, 2, 0, 1, 2)
    tables[2][1, 3] = np.nan                                    # camera 1's new P1: every candidate of its boxes is NaN
    tables[3][1, 3] = np.nan
    centre, err, idx, _ = same_as_restatement(dev, state, cam, tables, status=ops.LABEL_BAD_ERROR)
    assert np.isnan(centre[[1, 4]]).all() and (idx[[1, 4]] == -1).all() and np.isfinite(centre[[0, 2, 3, 5]]).all()
    tables[2][1, 3] = tables[3][1, 3] = 0.0
    same_as_restatement(dev, state, cam, tables)                # the device is still well
    with pytest.raises(RuntimeError):
        on_device(dev, state, cam, tables, rc.radii(), 17)
    with pytest.raises(RuntimeError):
        on_device(dev, state, cam, tables, rc.radii(), 1)


@pytest.mark.parametrize("reverse", [False, True])
def test_offset_y_equals_the_restatement_bit_for_bit(dev, reverse):
    from retinanet_mi355x import ops
    rng = np.random.RandomState(11)
    n = 300                                                     # more than one block
    xy = np.stack([rng.uniform(-100, 2000, n), rng.uniform(0, 120, n)], axis=1)
    coef = np.stack([rng.uniform(-3e-5, 3e-5, n), rng.uniform(-3e-3, 3e-3, n), rng.uniform(-1, 1, n)], axis=1)
    straight, direction = rng.uniform(60, 80, n), rng.choice([1, -1, 0], n).astype(np.int32)
    got = ops.label_offset_y(*(torch.from_numpy(a).to(dev) for a in (xy, coef, straight, direction)), reverse).cpu().numpy()
    want = np.array([rc.offset_y(xy[i, 0], xy[i, 1], coef[i], straight[i], direction[i], reverse) for i in range(n)])
    assert bit_equal(got, want) and {1, -1, 0} == set(direction.tolist())
    assert ops.label_offset_y(*(torch.from_numpy(a[:0]).to(dev) for a in (xy, coef, straight, direction))).shape == (0,)


def rewritten(Me, scene, pickles=None):
    """Every pass on a fresh stand-in -> {key: array} under the names of rc.restated (without the scene prefix)."""
    out, names = {}, scene["names"]
    with contextlib.redirect_stdout(io.StringIO()) as log:
        if rc.all_have_gen(scene):
            me = Me(scene)
            new = me.wrapper(scene["hg_new"])
            errors = me.replace_homgraphy(None if pickles else new)
            assert me.hg is new or pickles
            out["rebase_err"] = np.array(errors, np.float64)
            kept = [me.data[f][k] for f, k, o in rc.visit(rc.Labels(scene), scene["last_frame"] + 1) if o["gen"] == "Manual"]
            assert all(type(b["x"]) is float and type(b["y"]) is float for b in kept) and len(kept) == len(errors)
            out["rebase_xy"] = np.array([[b["x"], b["y"]] for b in kept], np.float64).reshape(-1, 2)
            rc.dumped(out, "hg", me, names)
        for tag, reverse in (("y0", False), ("y1", True)):
            me = Me(scene)
            assert me.replace_y(reverse) is None
            rc.dumped(out, tag, me, names)
        me = Me(scene)
        me.replace_timestamps()
        rc.dumped(out, "ts", me, names)
        out["ts_table"] = lc.ts_table(me.all_ts, names)
    out["log"] = log.getvalue()
    return out


def check_against(got, want, tag):
    for k in want:
        if k in ("rebase_win", "box_y"):
            continue
        if k == "rebase_err":
            assert got[k].shape == want[k].shape and np.all(np.abs(got[k] - want[k]) <= 1e-9 * np.abs(want[k])), (tag, k)
        else:
            assert bit_equal(got[k], want[k]), (tag, k)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_pass_equals_the_reference(Me, dev, golden, name, tmp_path, monkeypatch):
    g, scene = golden("label_rewrite"), SCENES[name]
    want = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    if name == "rebase":                                        # the default: the two pickles of the working directory
        new = Me(scene).wrapper(scene["hg_new"])
        for side, hg in (("EB", new.hg1), ("WB", new.hg2)):
            with open(tmp_path / "{}_homography5.cpkl".format(side), "wb") as f:
                pickle.dump(hg, f)
        monkeypatch.chdir(tmp_path)
    got = rewritten(Me, scene, pickles=name == "rebase")
    check_against(got, want, name)
    log = got["log"].splitlines()
    assert "Replaced timestamps" in log
    if name == "rebase":
        mean = sum([0] + got["rebase_err"].tolist()) / (1 + len(got["rebase_err"]))
        assert "Re-based 87 manual boxes. Average error: {}".format(mean) in log
        me = rc.Labels(scene)
        boxes = [o for _, _, o in rc.visit(me, scene["last_frame"] + 1) if o["gen"] == "Manual"]
        state = np.array([[float(o[k]) for k in rc.STATE_KEYS] for o in boxes])
        cam = [scene["names"].index(o["camera"]) for o in boxes]
        tables = rc.tables(me.hg, scene["names"]) + rc.tables(rc.build_hg(scene["hg_new"]), scene["names"])
        centre, err, idx, _ = same_as_restatement(dev, state, cam, tables)
        assert bit_equal(idx.astype(np.int64), want["rebase_win"]) and bit_equal(centre, want["rebase_xy"])
        assert np.all(np.abs(err - want["rebase_err"]) <= 1e-9 * np.abs(want["rebase_err"]))


def test_a_fuzz_scene_equals_the_restatement_exactly(Me):
    scene = rc.fuzz_scene(FUZZ_SEED)
    assert len(scene["names"]) == 3 and len(scene["data"]) == 41 and lc.unused_id(scene["data"]) == 6
    want = {k[2:]: v for k, v in rc.restated("f", scene).items()}
    got = rewritten(Me, scene)
    assert len(want["rebase_err"]) == 99 and bit_equal(got["rebase_err"], want["rebase_err"])
    check_against(got, want, "fuzz")


def test_a_status_bit_raises_and_leaves_data_and_hg_as_they_were(Me, monkeypatch):
    from retinanet_mi355x import ops
    scene = SCENES["rebase"]
    me = Me(scene)
    data, hg, before = me.data, me.hg, lc.dump(me.data, scene["names"])
    real = ops.label_rebase

    def one_bad_camera(state6, cam, *rest, **kw):
        cam = cam.clone()
        cam[5] = len(scene["names"])
        return real(state6, cam, *rest, **kw)
    monkeypatch.setattr(ops, "label_rebase", one_bad_camera)
    with pytest.raises(RuntimeError, match="camera index outside"):
        me.replace_homgraphy(me.wrapper(scene["hg_new"]))
    assert me.data is data and me.hg is hg and all(bit_equal(a, b) for a, b in zip(before, lc.dump(me.data, scene["names"])))


def test_empty_label_sets_pass_through(Me):
    scene = lc.empty_scene(2, 5, seed=1)
    scene["hg_old"] = scene["hg_new"] = rc.hg_spec(scene["names"])
    with contextlib.redirect_stdout(io.StringIO()):
        me = Me(scene)
        assert me.replace_homgraphy(me.wrapper(scene["hg_new"])) == [] and me.data == [{}] * 5
        me.replace_y()
        me.replace_timestamps()
    assert me.data == [{}] * 5


def test_custom_ops_agree_with_ops_and_pass_opcheck(dev):
    from retinanet_mi355x import ops, torch_ops
    state, cam, tables = random_boxes(5, seed=9)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = [up(t.reshape(-1, 3, 4)) for t in tables]
    args = (up(state), up(cam), P[0], None, P[2], P[3], up(np.array(rc.radii(), np.float64)), 11)
    rng = np.random.RandomState(1)
    yargs = (up(rng.uniform(0, 100, (7, 2))), up(rng.uniform(-1, 1, (7, 3))), up(rng.uniform(60, 80, 7)),
             up(np.array([1, -1, 1, -1, 0, 1, -1], np.int32)), True)
    for name, a in (("label_rebase", args), ("label_offset_y", yargs)):
        got, want = getattr(torch.ops.retinanet_mi355x, name)(*a), getattr(ops, name)(*a)
        got, want = (got, want) if isinstance(got, (tuple, list)) else ((got,), (want,))
        assert len(got) == len(want) and all(bit_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(got, want)), name
        torch.library.opcheck(getattr(torch_ops, name), a, test_utils=("test_schema", "test_autograd_registration"))

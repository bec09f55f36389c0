"""GPU: csrc/label_audit.hip (ops.label_pair_samples / label_outliers / label_interpolate) and the public label_audit
functions on top of it, against the reference's own output (tests/golden/label_audit.npz) and the restatement of
tests/label_audit_cases.py.

Everything is compared BIT FOR BIT: the kernels' arithmetic is fp64 with one rounding per operation in the reference's order,
and the means are numpy's on identical lists, so there is no tolerance to choose.

Shapes: the golden scenes hold tracklets of 0, 1, 2, 63, 64, 65 and 130 rows (the wave-stride edges of the min / max and
crossing scans), gaps of 1 and 70 frames, 3 to 6 cameras; the 100 fuzz scenes have 3 to 5 cameras, up to 60 frames and 8 ids.

The extinct-id RuntimeError of remove_outliers cannot be reached from real labels: a row deleted by the previous-frame test
has a surviving predecessor, and a row deleted by the next-frame test hands the question to its successor, whose predecessor
is then gone, and so on to the tracklet's last visited row, which has no test left to fire -- at least one row of every
tracklet survives.  The check reads the kernel's flags, so the test hands it flags that delete everything."""
import contextlib
import io

import numpy as np
import pytest
import torch

import label_audit_cases as lc

pytestmark = pytest.mark.gpu
SCENES = lc.golden_scenes()


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def Me(dev):
    import label_audit as la

    class Me(lc.Labels, la.LabelAudit):
        pass
    return Me


def audited(Me, scene):
    """Every method on a fresh stand-in -> {key: array} under the names of lc.restated, plus the returned statistics."""
    out, names = {}, scene["names"]
    with contextlib.redirect_stdout(io.StringIO()) as log:
        me = Me(scene)
        out["used"] = me.estimate_ts_bias()
        out["ts_bias"] = np.array(me.ts_bias, np.float64)
        try:
            all_diffs, out["y_stats"] = Me(scene).est_y_error()
            out["y_means"] = np.array(all_diffs, np.float64).reshape(-1)
        except ValueError:
            out["y_means"] = "ValueError"
        for tag, flag in (("proj", False), ("curve", True)):
            xe, ye = Me(scene).estimate_projection_error(reverse_curve_offset=flag)
            assert all(type(v) is np.float64 for v in xe + ye)
            out[tag + "_x"], out[tag + "_y"] = np.array(xe, np.float64).reshape(-1), np.array(ye, np.float64).reshape(-1)
        me = Me(scene)
        assert me.remove_outliers() is None
        out["outliers_idx"], out["outliers_val"] = lc.dump(me.data, names)
        me = Me(scene)
        out["added"] = me.interpolate_all()
        me.interpolate(4, verbose=False)
        out["interp_idx"], out["interp_val"] = lc.dump(me.data, names)
        me = Me(scene)
        me.unbias_timestamps()
        out["unbias_idx"], out["unbias_val"] = lc.dump(me.data, names)
        out["unbias_ts"], out["unbias_bias"] = lc.ts_table(me.all_ts, names), np.array(me.ts_bias, np.float64)
    out["log"] = log.getvalue()
    return out


def check_against(got, want, tag):
    """want: the arrays of lc.restated / the golden file, without the scene prefix."""
    for k in ("ts_bias", "y_means", "proj_x", "proj_y", "curve_x", "curve_y", "outliers_idx", "outliers_val", "interp_idx",
              "interp_val", "unbias_idx", "unbias_val", "unbias_ts", "unbias_bias"):
        assert bit_equal(got[k], want[k]), (tag, k)
    lists = {tuple(p): want["ts_diffs"][want["ts_off"][i]:want["ts_off"][i + 1]] for i, p in enumerate(want["ts_pairs"].tolist())}
    for cam, used in enumerate(got["used"]):
        mine = [p for p in lists if p[0] == cam]
        assert (used is None) == (not mine), (tag, cam)
        if used is not None:
            d = lists[(cam, used[0])]
            assert mine == [(cam, used[0])] and used[3] == len(d), (tag, cam)
            assert bit_equal(used[1], np.mean(d)) and bit_equal(used[2], np.std(d)), (tag, cam)
    ylists = {tuple(p): want["y_diffs"][want["y_off"][i]:want["y_off"][i + 1]] for i, p in enumerate(want["y_pairs"].tolist())}
    for i, st in enumerate(got["y_stats"]):
        d = ylists.get((i + 1, i))
        assert (st is None) == (d is None), (tag, i)
        if st is not None:
            assert bit_equal(st[0], np.mean(d)) and bit_equal(st[1], np.std(d)), (tag, i)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_method_equals_the_reference_bit_for_bit(Me, golden, name):
    g = golden("label_audit")
    want = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    got = audited(Me, SCENES[name])
    check_against(got, want, name)
    assert got["added"] == int((want["interp_idx"][:, 4] == 1).sum()) - (14 + 3 if name == "interp" else 0)
    log = got["log"].splitlines()
    assert "Done)" in log and "Un-biased timestamps" in log and any(l.startswith("Removed ") and l.endswith(" outlier data points") for l in log)
    if name == "audit":
        assert "No matching points for cameras p1c4 and p1c3" in log and "No matching points for cameras p1c6 and p1c1" in log
        assert "Error 1458 search for it" in log and any(l.startswith("Average y-error over all cameras: ") for l in log)
        mean = "Camera p1c2 ofset relative to camera p1c1: {}s ({}s absolute)".format(got["used"][1][1], got["ts_bias"][1])
        assert mean in log


@pytest.mark.parametrize("part", range(4))
def test_fuzz_scenes_equal_the_restatement_bit_for_bit(Me, part):
    for seed in range(25 * part, 25 * part + 25):
        scene = lc.fuzz_scene(seed)
        try:
            want = {k[2:]: v for k, v in lc.restated("f", scene).items()}
        except ValueError:                                      # est_y_error with nothing to carry: the same refusal
            with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
                Me(scene).est_y_error()
            continue
        check_against(audited(Me, scene), want, seed)


def test_interpolation_prefix_carries_across_a_chunk_of_tracklets(Me):
    """la_prefix_kernel walks the tracklets 256 at a time: 257 tracklets (one camera), most of one row, with gaps in tracklets
    3, 254 and 255 (the first chunk) and 256 (alone in the second), so the fill's rows depend on the carry between the chunks."""
    scene = lc.empty_scene(1, 12, seed=9)
    gaps = {3: (0, 4), 254: (1, 3, 9), 255: (2, 5), 256: (0, 7, 8, 11)}
    for oid in range(257):
        for f in gaps.get(oid, (oid % 12,)):
            lc.put(scene, f, 0, oid, 3.0 * f + 0.25 * oid, 20.0 + 0.5 * f + 0.01 * oid, cls=oid)
    want = lc.Labels(scene)
    assert lc.ref_interpolate(want) == 3 + 6 + 2 + 8
    me = Me(scene)
    assert me.interpolate_all() == 19
    for got_a, want_a in zip(lc.dump(me.data, scene["names"]), lc.dump(want.data, scene["names"])):
        assert bit_equal(got_a, want_a)


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("cols", [(0, 2, -1), (0, 1, -1), (2, 0, 1)])
def test_sample_block_equals_the_restatement(dev, name, cols):
    import label_audit as la
    from retinanet_mi355x import ops
    scene = SCENES[name]
    tab = la.pack_tracklets(scene["data"], scene["names"])
    off, table = torch.from_numpy(tab["offsets"]).to(dev), torch.from_numpy(tab["cols"]).to(dev)
    flags, values, status = ops.label_pair_samples(off, table, tab["n_cam"], *cols)
    want_flags, want_values = lc.sample_block(scene, *cols)
    assert int(status) == 0
    assert bit_equal(flags.cpu().numpy(), want_flags) and bit_equal(values.cpu().numpy(), want_values)
    if name == "audit" and cols == (0, 2, -1):
        assert {int(f) for f in want_flags.reshape(-1)} >= {0, 1, 3, 5, 7}      # every combination of the flags occurs


def test_mixin_mutates_its_object_as_the_reference_does(Me):
    scene = SCENES["interp"]
    me = Me(scene)
    data, all_ts, bias = me.data, me.all_ts, me.ts_bias
    with contextlib.redirect_stdout(io.StringIO()) as log:
        me.interpolate(0)
    assert log.getvalue() == "Interpolated boxes for object 0\n"
    assert me.data is data and list(data[6]) == ["p1c1_0", "p1c2_0"] and list(data[5]) == ["p1c2_0", "p1c1_0"]    # camera inner; behind what was there
    new = data[40]["p1c1_0"]
    assert list(new) == ["x", "y", "l", "w", "h", "direction", "id", "class", "timestamp", "camera", "gen"]
    assert new["gen"] == "Interpolation" and new["id"] == 0 and new["camera"] == "p1c1" and new["timestamp"] is all_ts[40]["p1c1"]
    assert new["l"] == data[3]["p1c1_0"]["l"] and new["h"] == data[3]["p1c1_0"]["h"] != data[74]["p1c1_0"]["h"]   # the row BEFORE the gap
    assert type(new["x"]) is float and "p1c3_4" not in data[101]
    t1, t2, ti = all_ts[3]["p1c1"], all_ts[74]["p1c1"], all_ts[40]["p1c1"]
    p1 = float(t2 - ti) / float(t2 - t1)
    assert new["x"] == p1 * data[3]["p1c1_0"]["x"] + (1.0 - p1) * data[74]["p1c1_0"]["x"]
    with contextlib.redirect_stdout(io.StringIO()):
        me.interpolate(4, verbose=False)                        # an id above the first unused one, asked for by name
        assert me.interpolate_all() == 0                        # nothing is left to fill
    assert "p1c3_4" in data[101] and me.get_unused_id() == 3
    stamp = data[0]["p1c1_0"]["timestamp"]
    with contextlib.redirect_stdout(io.StringIO()) as log:
        me.unbias_timestamps()
    assert me.ts_bias is bias and bias[0] == 0 and bias[2] == scene["ts_bias"][2] and me.all_ts is all_ts
    assert data[9]["p1c2_0"]["timestamp"] == scene["all_ts"][9]["p1c2"] + bias[1] and data[0]["p1c1_0"]["timestamp"] == stamp
    assert all_ts[7]["p1c2"] == scene["all_ts"][7]["p1c2"] + bias[1] and all_ts[7]["p1c3"] == scene["all_ts"][7]["p1c3"] + bias[2]
    assert str(bias) in log.getvalue() and str(me.seq_keys) in log.getvalue()


def test_extinct_id_raises_and_leaves_data_untouched(Me, monkeypatch):
    from retinanet_mi355x import ops
    scene = SCENES["outliers"]
    me = Me(scene)
    real = ops.label_outliers

    def everything(*a, **k):
        delete, status = real(*a, **k)
        return torch.ones_like(delete), status
    monkeypatch.setattr(ops, "label_outliers", everything)
    with pytest.raises(RuntimeError, match="every box of id 0"):
        me.remove_outliers()
    assert bit_equal(lc.dump(me.data, scene["names"])[0], lc.dump(scene["data"], scene["names"])[0])


def test_empty_data_and_a_single_camera(Me):
    for n_cam, frames in ((2, 0), (2, 5), (1, 5)):
        scene = lc.empty_scene(n_cam, frames, seed=1)
        if n_cam == 1:
            lc.track(scene, 0, 0, 0, 5, 0.0, 40.0, 30.0)        # every step is a jump: row 0 goes against the last frame, 1..3 from ahead
        me = Me(scene)
        with contextlib.redirect_stdout(io.StringIO()) as log:
            assert me.estimate_ts_bias() == [None] * n_cam and me.ts_bias[0] == 0
            assert me.est_y_error() == ([], [None] * (n_cam - 1))
            assert me.estimate_projection_error() == ([], []) and me.estimate_projection_error(True) == ([], [])
            assert me.interpolate_all() == 0
            me.remove_outliers()
            me.unbias_timestamps()
        log = log.getvalue().splitlines()
        assert log.count("Done)") == 2
        assert ("No matching points for cameras p1c2 and p1c1" in log) == (n_cam == 2)
        assert "Removed {} outlier data points".format(4 if n_cam == 1 else 0) in log
        assert [len(fd) for fd in me.data] == ([] if frames == 0 else [0] * 5 if n_cam == 2 else [0, 0, 0, 0, 1])


def test_corrupted_tables_set_the_status_word_and_raise(dev):
    import label_audit as la
    from retinanet_mi355x import ops
    scene = SCENES["audit"]
    tab = la.pack_tracklets(scene["data"], scene["names"])
    R, F, C = len(tab["cols"]), tab["n_frames"], tab["n_cam"]
    cols, frame = torch.from_numpy(tab["cols"]).to(dev), torch.from_numpy(tab["frame"]).to(dev)
    ts = torch.from_numpy(lc.ts_table(scene["all_ts"], scene["names"])).to(dev)
    track = np.repeat(np.arange(len(tab["offsets"]) - 1), np.diff(tab["offsets"]))
    rows = int((np.diff(tab["frame"]) - 1)[track[1:] == track[:-1]].sum())      # every missing frame inside a tracklet
    assert rows > 0
    good = torch.from_numpy(tab["offsets"]).to(dev)
    out = ops.label_interpolate(good, cols, frame, ts, rows)
    assert int(out[4]) == 0 and int(out[3]) == rows and int((out[1] < 0).sum()) == 0
    for spoil in ({1: R + 5}, {3: -7}, {2: 400, 3: 10}, {len(tab["offsets"]) - 1: 2 ** 40}):
        bad = tab["offsets"].copy()
        for i, v in spoil.items():
            bad[i] = v
        off = torch.from_numpy(bad).to(dev)
        calls = (lambda: ops.label_pair_samples(off, cols, C, 0, 2)[-1], lambda: ops.label_outliers(off, cols, frame, F, F)[-1],
                 lambda: ops.label_interpolate(off, cols, frame, ts, rows)[-1])
        for call in calls:
            status = int(call())
            assert status & ops.LABEL_BAD_OFFSETS, (spoil, status)
            with pytest.raises(RuntimeError, match="refused their input"):
                ops.label_check(status)
    for spoil in ({5: F}, {5: -1}, {6: int(tab["frame"][5])}):                  # outside the frames; not ascending
        bad = tab["frame"].copy()
        for i, v in spoil.items():
            bad[i] = v
        fr = torch.from_numpy(bad).to(dev)
        assert int(ops.label_outliers(good, cols, fr, F, F)[-1]) & ops.LABEL_BAD_FRAME, spoil
        assert int(ops.label_interpolate(good, cols, fr, ts, rows)[-1]) & (ops.LABEL_BAD_FRAME | ops.LABEL_BAD_PREFIX), spoil
    assert int(ops.label_interpolate(good, cols, frame, ts, rows - 3)[-1]) == ops.LABEL_BAD_PREFIX      # fewer rows than gaps
    assert int(ops.label_outliers(good, cols, frame, F, F)[-1]) == 0            # the device is still well


def test_custom_ops_agree_with_ops_and_pass_opcheck(dev):
    import label_audit as la
    from retinanet_mi355x import ops, torch_ops
    scene = SCENES["interp"]
    tab = la.pack_tracklets(scene["data"], scene["names"])
    off, cols, frame = (torch.from_numpy(tab[k]).to(dev) for k in ("offsets", "cols", "frame"))
    ts = torch.from_numpy(lc.ts_table(scene["all_ts"], scene["names"])).to(dev)
    F, C, rows = tab["n_frames"], tab["n_cam"], 1 + 70 + 3
    calls = (("label_pair_samples", (off, cols, C, 2, 0, 1)), ("label_outliers", (off, cols, frame, F, F)),
             ("label_interpolate", (off, cols, frame, ts, rows)))
    for name, args in calls:
        got = getattr(torch.ops.retinanet_mi355x, name)(*args)
        want = getattr(ops, name)(*args)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert bit_equal(a.cpu().numpy(), b.cpu().numpy()), name
        torch.library.opcheck(getattr(torch_ops, name), args, test_utils=("test_schema", "test_autograd_registration"))

"""CPU: the restatement of Data_Reader's load / reinterpolate / write_to_file in tests/datareader_cases.py against the
reference's own output (tests/golden/datareader.npz, written by tools/make_golden_datareader.py), and the host side of the
mirror (3d-playground_amd/datareader.py): the parser, ``__next__``, the walk over instants, the packing, the refusals.

String-equal with the reference: the header and columns 0-3, 8-10 and 27-45 of every row (timestamp, id, class, the fp32 space
and state cells, theta, camera, ts_bias: fp32 elementwise arithmetic and Python-float interpolation leave no freedom).  The
four BBox and sixteen image cells go through the reference's BLAS matrix product, whose summation order is the library's:
numeric, at the bound the project holds state_to_im to against reference goldens (tests/test_gpu_dropin.py: rtol 1e-9, atol
1e-9).  Every fixture keeps the homogeneous divisor above 0.1, so that bound is about rounding, not cancellation.  The dump
of ``data`` (instant, id, timestamp, the six interpolated fields) is bit-equal."""
import os

import numpy as np
import pytest

import datareader_cases as dc

RTOL = ATOL = 1e-9


@pytest.mark.parametrize("case", list(dc.GOLDEN_CASES))
def test_restatement_equals_the_reference(golden, case):
    g = golden("datareader")
    text, names, P, P2, kw, freq = dc.case_inputs(g, case)
    data, got = dc.run(text, names, P, P2, frequency=freq, **kw)
    want = g[case + "_out"].tobytes().decode()
    assert want.endswith("\r\n") and got.count("\r\n") == want.count("\r\n")
    worst = dc.compare_text(got, want, RTOL, ATOL)
    print("%s: %d rows, largest image-cell deviation restated vs reference %.3e px" % (case, len(dc.parse(want)) - 1, worst))
    d = dc.dump(data)
    assert d.shape == g[case + "_dump"].shape and d.tobytes() == g[case + "_dump"].tobytes()
    items, st, keep = dc.states(data)
    w = dc.divisors(st[keep], [o["camera"] for o, k in zip(items, keep) if k], names, P, P2)
    assert w.min() > dc.MIN_DIVISOR


def test_fixture_covers_what_it_is_for(golden):
    g = golden("datareader")
    rows = {c: dc.parse(g[c + "_out"].tobytes().decode())[1:] for c in dc.GOLDEN_CASES}
    y = np.array([float(r[40]) for r in rows["wrapper"]])
    assert (y > 60).any() and (y < 60).any()                                   # both matrix sets of the wrapper are used
    differ = [a[11:27] != b[11:27] for a, b in zip(rows["wrapper"], rows["hz30"])]
    assert any(differ) and not all(differ)
    n = {c: len(set(r[1] for r in rows[c])) for c in rows}
    assert n["hz10"] < n["plain"] < n["hz30"] < n["hz120"]                      # the walk skips frames / repeats a pair
    assert len(set(r[36] for r in rows["working"])) == 6
    _, loaded = dc.load(g["in_irregular"].tobytes().decode())
    sizes = [len(f) for f in loaded]
    ids = [set(f) for f in loaded]
    assert any(a - b for a, b in zip(ids, ids[1:])) and any(b - a for a, b in zip(ids, ids[1:]))      # deaths and births
    assert any(list(a) != sorted(a) for a in loaded) and max(sizes) > min(sizes)


def edge_file(tmp_path):
    text = dc.tracking_csv(seed=11, n_frames=20, n_objs=6, edges=True)
    path = os.path.join(str(tmp_path), "in.csv")
    with open(path, "w", newline="") as f:
        f.write(text)
    return text, path


def test_parser_edges(tmp_path, golden):
    import datareader
    text, path = edge_file(tmp_path)
    assert text == golden("datareader")["in_irregular"].tobytes().decode()      # the generator is portable: same bytes
    plain_header, plain_rows = dc.tracking_rows(11, 20, 6)
    dr = datareader.Data_Reader(path, None)
    cams, want = dc.load(text)
    assert dr.cameras == cams == dc.NAMES[:6] and dr.d_idx == 0 and dr.hg is None
    assert len(dr.class_colors) == 11 and dr.classes["truck"] == 5 and dr.classes[5] == "truck (other)" and len(dr.classes) == 17
    assert dr.data == want and [list(a) for a in dr.data] == [list(b) for b in want]       # values and dict order
    first_ts = np.round(float(plain_rows[0][1]), 4)
    frame0 = dr.data[0]
    assert list(frame0.values())[0]["timestamp"] == first_ts and isinstance(first_ts, np.float64)
    # the junk lines and the "Frame #" row are headers; the row with "12.5ft" and the short row are skipped
    assert sum(len(f) for f in dr.data) == len(plain_rows) + 1                  # + the id 999 row; the repeated (ts, id) replaces
    # the repeated (ts, id): the later row's value, the earlier row's position
    k0 = int(plain_rows[0][2])
    assert list(frame0)[0] == k0 and frame0[k0]["x"] == float(plain_rows[0][39]) + 1.0
    with999 = [f for f in dr.data if 999 in f]                                  # the empty camera cell
    assert len(with999) == 1 and with999[0][999]["camera"] == "p1c1" and with999[0][999]["timestamp"] == np.round(float(plain_rows[1][1]), 4)
    assert with999[0][int(plain_rows[1][2])]["camera"] == plain_rows[1][36] != ""
    assert set(frame0[k0]) == {"timestamp", "id", "class", "x", "y", "l", "w", "h", "direction", "v", "ts_bias", "camera", "frame"}
    assert frame0[k0]["ts_bias"] == {c: round(0.01 * i, 3) for i, c in enumerate(cams)} and frame0[k0]["frame"] == plain_rows[0][0]
    assert isinstance(frame0[k0]["direction"], int) and isinstance(frame0[k0]["x"], float)
    # metric: Python-float products
    m = datareader.Data_Reader(path, None, metric=True)
    a, b = m.data[3], dr.data[3]
    for oid in b:
        for key in dc.FIELDS:
            assert a[oid][key] == b[oid][key] * 3.281
    assert m.data == dc.load(text, metric=True)[1]


def test_next_and_walk(tmp_path):
    import datareader
    text, path = edge_file(tmp_path)
    dr = datareader.Data_Reader(path, None)
    n = len(dr.data)
    datum, ts, next_ts, next_datum = next(dr)
    assert datum == dr.data[0] and datum is not dr.data[0] and next_datum == dr.data[1] and dr.d_idx == 1
    assert ts == dc._first_ts(dr.data[0]) and next_ts == dc._first_ts(dr.data[1])
    dr.d_idx = n - 1
    datum, ts, next_ts, next_datum = next(dr)
    assert datum == dr.data[-1] and next_ts is None and next_datum is None and dr.d_idx == n
    assert next(dr) == (None, None, None, None) and dr.d_idx == n
    for hz in (30, 10, 120, 7.5):
        dr.d_idx = 0
        a, t = dr._walk(hz)
        want = dc.walk(dr.data, hz)
        assert a == [w[0] for w in want] and np.array(t).tobytes() == np.array([w[1] for w in want]).tobytes()
        assert all(isinstance(v, np.float64) for v in t)
    pk = datareader.pack_frames(dr.data)
    assert pk["offsets"].dtype == np.int64 and pk["offsets"][0] == 0 and pk["offsets"][-1] == len(pk["rows"]) == len(pk["ids"])
    assert np.array_equal(np.diff(pk["offsets"]), [len(f) for f in dr.data])
    assert pk["fields"].shape == (len(pk["rows"]), 6) and pk["fields"].dtype == np.float64
    assert list(pk["ids"][:len(dr.data[0])]) == list(dr.data[0])
    assert np.array_equal(pk["frame_ts"], [dc._first_ts(f) for f in dr.data])
    assert np.isnan(datareader.pack_frames([{}, dr.data[0]])["frame_ts"][0])


def test_refusals(tmp_path):
    import torch
    import datareader
    from retinanet_mi355x import ops, torch_ops
    text, path = edge_file(tmp_path)
    dr = datareader.Data_Reader(path, None)
    before = [dict(f) for f in dr.data]
    for bad in (0, -30, float("nan")):
        with pytest.raises(ValueError):
            dr.reinterpolate(frequency=bad)
    assert dr.data == before and dr.d_idx == 0
    for call in (lambda: datareader.Camera_Wrapper("p1c1.mp4"), lambda: datareader.test_integrity("p1c1.mp4"),
                 lambda: dr.plot_labels(None, [], [], [], [], [], [], []), lambda: dr.plot_in([])):
        with pytest.raises(NotImplementedError, match="cv2"):
            call()
    import inspect
    assert inspect.signature(dr.reinterpolate).parameters["save"].default == "reinterpolated_3D_tracking_outputs.csv"
    assert inspect.signature(dr.write_to_file).parameters["save_file"].default == "default_save_file.csv"
    # the ops refuse CPU tensors, and dtype / shape before any launch
    off, ids = torch.tensor([0, 2, 3]), torch.tensor([5, 6, 5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reinterp_mate(off, ids)
    with pytest.raises(RuntimeError):
        ops.reinterp_offsets(off, torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.reinterp_rows(off, torch.zeros(2, dtype=torch.float64), torch.zeros(3, 6, dtype=torch.float64), torch.zeros(3, dtype=torch.int32),
                          torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError):
        ops.track_rows(torch.zeros(3, 6, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), torch.zeros(1, 3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="status 17"):
        ops.reinterp_check(ops.REINTERP_BAD_OFFSETS | ops.REINTERP_BAD_MAT_INDEX)
    ops.reinterp_check(0)
    for name in ("reinterp_mate", "reinterp_offsets", "reinterp_rows", "track_rows"):
        assert name in torch_ops.OPERATORS and hasattr(torch.ops.retinanet_mi355x, name)


def test_results_rows_takes_row_cameras_and_a_ready_box():
    import results_csv
    names, P, _ = dc.cameras(6)
    st = np.array([[300.0, 20.0, 18.0, 6.5, 5.0, 1.0, 88.0], [250.0, 90.0, 40.0, 8.0, 12.0, -1.0, 70.0]], np.float32)
    cams = ["p1c2", "p1c5"]
    space, im, box = dc.project(st, cams, names, P)
    args = ([7, 8], [np.float64(1.5), np.float64(2.5)], st, space, im, ["sedan", "semi"], [[0.0], [0.0]])
    a = results_csv.results_rows(*args, camera=cams, box=box)
    b = results_csv.results_rows(*args, camera=cams)
    assert dc.csv_text(a) == dc.csv_text(b) and [r[36] for r in a] == cams and a[1][41] == np.pi / 2.0 and a[0][41] == 0
    assert [r[36] for r in results_csv.results_rows(*args)] == ["p1c1", "p1c1"]

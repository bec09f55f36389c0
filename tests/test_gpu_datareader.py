"""GPU: csrc/datareader.hip (ops.reinterp_mate / reinterp_offsets / reinterp_rows / track_rows) and the public
Data_Reader on top of it, against the restatement of tests/datareader_cases.py and the reference's own output
(tests/golden/datareader.npz).

Bit-equal with the restatement: the interpolated fields (fp64, one rounding per operation on both sides), the instants, the
row order, the source rows, the fp32 state, the space corners and keep.  Image corners and box: the bound tests/test_gpu_ops.py
holds rn_state_to_im to against oracle/homography.py (rtol 1e-9, atol 1e-8) -- the oracle's einsum sums in its own order.
Against the reference's files: the cells tests/test_datareader_host.py compares as strings are equal, the image cells within
rtol 1e-9, atol 1e-9 (tests/test_gpu_ops.py against the homography golden), the dump of ``data`` bit-equal.

Shapes: the frame sizes 0, 1, 63, 64, 65, 257 and 1031 / 1200 (above the RN_REINTERP_TILE = 1024 ids of one LDS tile) cross
the wave, workgroup and tile edges of the mate search and of the compaction."""
import os

import numpy as np
import pytest
import torch

import datareader_cases as dc

pytestmark = pytest.mark.gpu
IM_RTOL, IM_ATOL = 1e-9, 1e-8


# ------------------------------------------------------------------------------------------------ packed level
def packed_edges():
    """Hand-built frames -> (offsets, ids, fields, frame_ts, inst_a, inst_time).  Pair by pair:
    (0,1) row 0 of frame 0 unmated (first), the rest found in a permuted, larger frame with extra ids, in both LDS tiles;
    (1,2) only every other row of the first 130 is mated; (2,3) and (3,4) an empty frame on either side; (4,5) a frame of one
    row; (5,6) the last row unmated, order reversed; (6,7) no common id; (7,8) 1031 rows mated into 1200 permuted ones."""
    rng = np.random.RandomState(3)
    f0 = np.arange(257)
    f1 = rng.permutation(np.arange(1, 1032))
    f2 = f1[0:130:2].copy()
    f3 = np.zeros(0, np.int64)
    f4 = np.array([5000])
    f5 = np.arange(5062, 4999, -1)
    f6 = np.concatenate((np.arange(5001, 5063), [7000, 7001]))
    f7 = np.arange(20000, 21031)
    f8 = rng.permutation(np.arange(19900, 21100))
    frames = [f0, f1, f2, f3, f4, f5, f6, f7, f8]
    assert [len(f) for f in frames] == [257, 1031, 65, 0, 1, 63, 64, 1031, 1200]
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    ids = np.concatenate(frames).astype(np.int64)
    fields = (rng.rand(len(ids), 6) * 1000.0 - 200.0) * (1.0 + rng.rand(len(ids), 6) * 1e-7)
    frame_ts = 1623877000.0 + np.cumsum(0.02 + 0.05 * rng.rand(len(frames)))
    inst_a, inst_time = [], []
    for a in (0, 0, 1, 2, 3, 4, 4, 4, 5, 6, 7, 7, 5, 0):                         # repeated pairs, and not in order
        inst_a.append(a)
        inst_time.append(frame_ts[a] + (frame_ts[a + 1] - frame_ts[a]) * (len(inst_a) % 4) / 3.0)    # ts itself, thirds, next_ts
    return offsets, ids, fields, frame_ts, np.array(inst_a, np.int32), np.array(inst_time, np.float64)


def brute_force(offsets, ids, fields, frame_ts, inst_a, inst_time):
    """datareader.py:411-430 on the packed arrays, in Python floats."""
    out_f, out_src, out_inst, mate = [], [], [], np.full(len(ids), -1, np.int64)
    for f in range(len(offsets) - 2):
        nxt = {}
        for r in range(offsets[f + 1], offsets[f + 2]):
            nxt.setdefault(int(ids[r]), r)
        for r in range(offsets[f], offsets[f + 1]):
            mate[r] = nxt.get(int(ids[r]), -1)
    for t, (a, time) in enumerate(zip(inst_a, inst_time)):
        ts, next_ts = float(frame_ts[a]), float(frame_ts[a + 1])
        for r in range(offsets[a], offsets[a + 1]):
            if mate[r] >= 0:
                r1 = (float(time) - ts) / (next_ts - ts)
                r2 = 1 - r1
                out_f.append([float(fields[r, k]) * r1 + float(fields[mate[r], k]) * r2 for k in range(6)])
                out_src.append(r)
                out_inst.append(t)
    return np.array(out_f, np.float64).reshape(-1, 6), np.array(out_src, np.int32), np.array(out_inst, np.int32), mate


@pytest.fixture(scope="module")
def edges():
    args = packed_edges()
    return args, brute_force(*args)


def test_mates_counts_and_rows_at_the_edges(dev, edges):
    import datareader
    from retinanet_mi355x import ops, torch_ops     # noqa: F401  (registers torch.ops.retinanet_mi355x.*)
    args, (want_f, want_src, want_inst, want_mate) = edges
    offsets, ids, fields, frame_ts, inst_a, inst_time = args
    up = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    mate, status = ops.reinterp_mate(up(offsets), up(ids))
    assert mate.dtype == torch.int32 and np.array_equal(mate.cpu().numpy(), want_mate)
    count, prefix, status = ops.reinterp_offsets(up(offsets), mate, up(inst_a), status=status)
    per_frame = np.array([(want_mate[offsets[f]:offsets[f + 1]] >= 0).sum() for f in range(len(offsets) - 1)])
    assert list(per_frame) == [256, 65, 0, 0, 1, 62, 0, 1031, 0]
    assert np.array_equal(count.cpu().numpy(), per_frame[inst_a])
    assert prefix.dtype == torch.int64 and np.array_equal(prefix.cpu().numpy(), np.concatenate(([0], np.cumsum(per_frame[inst_a]))))
    assert int(status) == 0
    got_f, got_src, got_inst, got_prefix = datareader.resample_packed(*args, dev)
    assert len(got_src) == len(want_src) == int(got_prefix[-1])
    assert np.array_equal(got_src, want_src) and np.array_equal(got_inst, want_inst)          # order, source rows, instants
    assert got_f.dtype == np.float64 and got_f.tobytes() == want_f.tobytes()                   # bit-equal interpolation
    at_ts = inst_time == frame_ts[inst_a]                                                      # t == ts: the NEXT frame's value
    rows = np.isin(got_inst, np.nonzero(at_ts)[0])
    assert rows.any() and np.array_equal(got_f[rows], fields[want_mate[got_src[rows]]])
    again = datareader.resample_packed(*args, dev)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (got_f, got_src, got_inst, got_prefix)))
    # the registered operators are the same entry points
    t_mate, _ = torch.ops.retinanet_mi355x.reinterp_mate(up(offsets), up(ids))
    assert torch.equal(t_mate, mate)


def test_offsets_carry_across_a_chunk_of_instants(dev):
    """dr_prefix_kernel walks the instants 256 at a time: 257 of them over five small frames, so the prefix of the last
    instant and the total hold the carry out of the first chunk."""
    from retinanet_mi355x import ops
    frames = [np.array([1, 2, 3]), np.array([3, 9, 1, 2]), np.array([9, 4]), np.array([5, 4, 6, 7, 9]), np.array([7])]
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    ids = np.concatenate(frames).astype(np.int64)
    inst_a = ((np.arange(257) * 7) % 4).astype(np.int32)                                       # inst_a[256] = 0, a frame of 3 mates
    none = np.zeros(0)
    want_mate = brute_force(offsets, ids, np.zeros((len(ids), 6)), np.arange(5.0), none, none)[3]
    per_frame = np.array([(want_mate[offsets[f]:offsets[f + 1]] >= 0).sum() for f in range(len(frames))])
    assert list(per_frame) == [3, 1, 2, 1, 0]
    up = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    mate, status = ops.reinterp_mate(up(offsets), up(ids))
    assert np.array_equal(mate.cpu().numpy(), want_mate)
    count, prefix, status = ops.reinterp_offsets(up(offsets), mate, up(inst_a), status=status)
    assert int(status) == 0 and np.array_equal(count.cpu().numpy(), per_frame[inst_a])
    assert prefix.dtype == torch.int64 and np.array_equal(prefix.cpu().numpy(), np.concatenate(([0], np.cumsum(per_frame[inst_a]))))


def test_empty_and_single_frame_inputs(dev):
    import datareader
    none = np.zeros(0)
    for offsets, ids, ts in (([0], [], []), ([0, 3], [1, 2, 3], [5.0]), ([0, 0, 0], [], [1.0, 2.0])):
        f, src, inst, prefix = datareader.resample_packed(offsets, ids, np.zeros((len(ids), 6)), ts, none, none, dev)
        assert f.shape == (0, 6) and len(src) == len(inst) == 0 and list(prefix) == [0]
    f, src, inst, prefix = datareader.resample_packed([0, 0, 0], [], np.zeros((0, 6)), [1.0, 2.0], [0, 0], [1.0, 1.5], dev)
    assert f.shape == (0, 6) and list(prefix) == [0, 0, 0]                                     # instants without a mated row


def test_bad_indices_set_the_status_and_are_left_out(dev, edges):
    import datareader
    from retinanet_mi355x import ops
    offsets, ids, fields, frame_ts, inst_a, inst_time = edges[0]
    for bad in (offsets[::-1].copy(), np.where(np.arange(len(offsets)) == 2, 10 ** 9, offsets),
                np.where(np.arange(len(offsets)) == 1, -5, offsets)):
        with pytest.raises(RuntimeError, match="frame offsets"):
            datareader.resample_packed(bad, ids, fields, frame_ts, inst_a, inst_time, dev)
    for bad_a in (np.array([0, 8], np.int32), np.array([-1], np.int32), np.array([2 ** 31 - 1], np.int32)):
        with pytest.raises(RuntimeError, match="frame pair"):
            datareader.resample_packed(offsets, ids, fields, frame_ts, bad_a, np.ones(len(bad_a)), dev)
    up = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    mate = torch.full((len(ids),), -1, dtype=torch.int32, device=dev)
    mate[0] = 5                                                                                 # inside frame 0, not frame 1
    mate[1] = int(offsets[1])
    count, prefix, status = ops.reinterp_offsets(up(offsets), mate, up(inst_a[:1]))
    assert int(status) == ops.REINTERP_BAD_MATE and count.cpu().tolist() == [1]
    out_f, out_src, _, status = ops.reinterp_rows(up(offsets), up(frame_ts), up(fields), mate, up(inst_a[:1]), up(inst_time[:1]),
                                                  torch.tensor([0, 7], device=dev), 0)         # a prefix past the 0 output rows
    assert int(status) & ops.REINTERP_BAD_PREFIX and out_f.shape == (0, 6)
    # track_rows: a matrix index outside the set
    names, P, P2 = dc.cameras(3)
    f = np.array([[300.0, 20.0, 18.0, 6.5, 5.0, 80.0]] * 4)
    idx = torch.tensor([0, 3, 2, -1], dtype=torch.int32, device=dev)
    state, space, im, box, keep, status = ops.track_rows(up(f), up(np.ones(4)), up(P), None, idx)
    assert int(status) == ops.REINTERP_BAD_MAT_INDEX and keep.cpu().tolist() == [1, 0, 1, 0]
    assert float(im[1].abs().max()) == 0 and float(im[3].abs().max()) == 0 and float(im[0].abs().min()) > 0
    with pytest.raises(RuntimeError, match="mat_index"):
        ops.reinterp_check(status)


# ------------------------------------------------------------------------------------------------ rows of the file
def mirror_hg(names, P, P2=None):
    import homography

    def one(M):
        hg = homography.Homography()
        hg.correspondence = {n: {"P": M[i]} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    return one(P) if P2 is None else homography.Homography_Wrapper(hg1=one(P), hg2=one(P2))


def write_input(tmp_path, text, name="in.csv"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w", newline="") as f:
        f.write(text)
    return path


def read(path):
    with open(path, newline="") as f:
        return f.read()


@pytest.mark.parametrize("cams,wrapper", [(6, False), (1, False), (6, True)], ids=["per_row", "one_camera", "wrapper"])
def test_track_rows_against_the_restatement(dev, cams, wrapper):
    import datareader
    names, P, P2 = dc.cameras(cams)
    if cams == 1:                                                                              # one camera for every row: one that
        P = dc.cameras()[1][2:3]                                                               # sees the whole stretch of road
    P2 = P2 if wrapper else None
    _, data = dc.load(dc.tracking_csv(seed=5, n_frames=14, n_objs=70, n_cams=cams))            # 300+ rows: more than one workgroup
    items, st, keep = dc.states(data)
    assert len(items) > 256 and (not wrapper or ((st[:, 1] > 60).any() and (st[:, 1] < 60).any()))
    fields = np.array([[o[k] for k in dc.FIELDS] for o in items])
    fields[3, 0], fields[4, 0], fields[5, 0] = 0.0, 1e-50, -1e-50                               # zero in fp32, dropped
    direction = [o["direction"] for o in items]
    row_cams = [o["camera"] for o in items]
    g_state, g_space, g_im, g_box, g_keep = datareader.project_rows(mirror_hg(names, P, P2), fields, direction, row_cams, dev)
    want = np.concatenate((fields[:, :5], np.array(direction, np.float64)[:, None], fields[:, 5:]), 1).astype(np.float32)
    assert g_state.dtype == np.float32 and g_state.tobytes() == want.tobytes()
    assert list(np.nonzero(g_keep == 0)[0]) == [3, 4, 5] and g_keep.dtype == np.uint8
    space, im, box = dc.project(want, row_cams, names, P, P2)
    assert g_space.dtype == np.float32 and g_space.tobytes() == space.tobytes()
    k = g_keep != 0                                                                            # the reference projects only these
    assert dc.divisors(want[k], [c for c, on in zip(row_cams, k) if on], names, P, P2).min() > dc.MIN_DIVISOR
    print("largest deviation from the restatement: im %.3e px, box %.3e px" % (np.abs(g_im - im)[k].max(), np.abs(g_box - box)[k].max()))
    assert np.allclose(g_im[k], im[k], rtol=IM_RTOL, atol=IM_ATOL) and np.allclose(g_box[k], box[k], rtol=IM_RTOL, atol=IM_ATOL)
    assert np.array_equal(g_box, np.stack((g_im[:, :, 0].min(1), g_im[:, :, 1].min(1), g_im[:, :, 0].max(1), g_im[:, :, 1].max(1)), 1))


# ------------------------------------------------------------------------------------------------ the public class
@pytest.mark.parametrize("case", list(dc.GOLDEN_CASES))
def test_data_reader_equals_the_reference(dev, golden, tmp_path, case):
    import datareader
    g = golden("datareader")
    text, names, P, P2, kw, freq = dc.case_inputs(g, case)
    dr = datareader.Data_Reader(write_input(tmp_path, text), mirror_hg(names, P, P2), **kw)
    out = os.path.join(str(tmp_path), "out.csv")
    if freq is None:
        dr.write_to_file(save_file=out)
    else:
        dr.reinterpolate(frequency=freq, save=out)                                             # writes to ``save``
        assert dr.d_idx == 0 and not os.path.exists("reinterpolated_3D_tracking_outputs.csv")
    worst = dc.compare_text(read(out), g[case + "_out"].tobytes().decode(), 1e-9, 1e-9)
    print("%s: largest image-cell deviation device vs reference %.3e px" % (case, worst))
    d = dc.dump(dr.data)
    assert d.shape == g[case + "_dump"].shape and d.tobytes() == g[case + "_dump"].tobytes()
    want_data = dc.load(text, **kw)[1] if freq is None else dc.reinterpolate(dc.load(text, **kw)[1], freq)
    assert dr.data == want_data and [list(f) for f in dr.data] == [list(f) for f in want_data]   # all thirteen keys, dict order


def test_zero_x_is_kept_in_data_and_dropped_from_the_file(dev, tmp_path):
    import datareader
    names, P, _ = dc.cameras(6)
    present = {0: [3, 2, 1, 0], 1: [0, 1, 2, 3, 4], 2: [4, 5], 3: [0, 1], 4: [1, 0, 2]}       # (1,2) shares one id, (2,3) none
    header, rows = dc.tracking_rows(9, 5, 6, frame_objs=present)
    text = dc.csv_text([header] + rows)
    dr = datareader.Data_Reader(write_input(tmp_path, text), mirror_hg(names, P))
    for frame in dr.data[:2]:
        frame[101]["x"] = 0.0                                                                  # exactly 0 in both frames
        frame[102]["x"] = 1e-50                                                                # non-zero in fp64, zero in fp32
    start = [{k: dict(v) for k, v in f.items()} for f in dr.data]
    out, again = os.path.join(str(tmp_path), "out.csv"), os.path.join(str(tmp_path), "again.csv")
    dr.reinterpolate(frequency=60, save=out)
    want = dc.reinterpolate(start, 60)
    assert dr.data == want and [list(f) for f in dr.data] == [list(f) for f in want]
    assert any(len(f) == 0 for f in dr.data) and any(list(f) == [103, 102, 101, 100] for f in dr.data)
    zero = [o for f in dr.data for o in f.values() if o["id"] == 101 and o["x"] == 0.0]
    tiny = [o for f in dr.data for o in f.values() if o["id"] == 102 and 0 < o["x"] < 1e-40]
    assert zero and tiny
    got = dc.parse(read(out))
    dc.compare_text(read(out), dc.file_text(want, dr.cameras, names, P), IM_RTOL, IM_ATOL)
    written = [(r[1], r[2]) for r in got[1:]]
    assert len(written) == sum(len(f) for f in dr.data) - len(zero) - len(tiny)
    assert not any(str(o["timestamp"]) == ts and oid == str(o["id"]) for o in zero + tiny for ts, oid in written)
    dr.write_to_file(save_file=again)                                                          # repeatable: the same bytes
    assert read(again) == read(out)


def test_one_instant_and_empty_input(dev, tmp_path):
    import datareader
    names, P, _ = dc.cameras(6)
    header, rows = dc.tracking_rows(4, 1, 3, frame_objs={0: [0, 1, 2]})
    out = os.path.join(str(tmp_path), "out.csv")
    one = datareader.Data_Reader(write_input(tmp_path, dc.csv_text([header] + rows)), mirror_hg(names, P))
    assert len(one.data) == 1
    one.write_to_file(save_file=out)
    assert len(dc.parse(read(out))) == 4
    one.reinterpolate(save=out)
    assert one.data == [] and read(out) == dc.csv_text([header])                               # a single instant: nothing to resample
    none = datareader.Data_Reader(write_input(tmp_path, dc.csv_text([header]), "none.csv"), mirror_hg(names, P))
    none.reinterpolate(save=out)
    assert none.data == [] and none.cameras == names and read(out) == dc.csv_text([header])


def test_a_refused_input_raises_and_writes_nothing(dev, tmp_path, monkeypatch):
    import datareader
    names, P, _ = dc.cameras(6)
    dr = datareader.Data_Reader(write_input(tmp_path, dc.tracking_csv(seed=2, n_frames=6, n_objs=4)), mirror_hg(names, P))
    before = [dict(f) for f in dr.data]
    out = os.path.join(str(tmp_path), "never.csv")
    real_pack, real_mats = datareader.pack_frames, datareader._matrices

    def bad_pack(data):
        pk = real_pack(data)
        pk["offsets"] = pk["offsets"][::-1].copy()
        return pk

    def bad_mats(hg, cameras, device):
        M, M2, idx = real_mats(hg, cameras, device)
        return M, M2, idx + M.shape[0]
    monkeypatch.setattr(datareader, "pack_frames", bad_pack)
    with pytest.raises(RuntimeError, match="frame offsets"):
        dr.reinterpolate(save=out)
    assert dr.data == before and not os.path.exists(out)
    monkeypatch.setattr(datareader, "pack_frames", real_pack)
    monkeypatch.setattr(datareader, "_matrices", bad_mats)
    with pytest.raises(RuntimeError, match="mat_index"):
        dr.write_to_file(save_file=out)
    assert not os.path.exists(out)

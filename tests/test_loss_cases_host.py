"""The cases of tests/loss_cases.py reach the paths of focal_kernel (csrc/focal_loss.hip) they are named after, its float64
reference agrees with oracle/losses.py in float32 -- losses to 1e-6, identical zero patterns, values inside the envelopes
-- and the comparison the GPU tests use rejects kernels with one mistake each (no GPU).  The wrong kernels are float64
evaluations of the loss on other integer decisions, or the reference's outputs altered afterwards (wrong_kernel below); a
result that holds a NaN or an infinity is rejected as well."""
import numpy as np
import pytest
import torch

import loss_cases as lc

U = 2.0 ** -24


def _states(case):
    return [None if a is None else a[2].numpy() for a in lc.assignment(case)]


# ------------------------------------------------------------------------------------------------ the reference
def test_clamp_bounds_are_the_float32_ones():
    """torch's float32 clamp(1e-4, 1 - 1e-4), the kernel's ``1.0f - 1e-4f`` and the reference's HI are one number."""
    x = torch.tensor([0.9998, 0.9999, 0.99995, 1.0], dtype=torch.float32)
    assert np.float32(x.clamp(1e-4, 1.0 - 1e-4).max()) == np.float32(1) - np.float32(1e-4) == lc.HI32
    assert np.float32(torch.zeros(1).clamp(1e-4, 1.0 - 1e-4)[0]) == lc.LO32
    assert lc.LO < 1e-4 and float(np.float32(1e-4)) == lc.LO       # a double clamp would cut what float32 passes
    v = lc.clamp_values()
    assert v[6] == 0.0 < v[1] < v[0] < v[2] < v[4] < v[3] < v[5] < v[7] == 1.0


@pytest.mark.parametrize("fam", lc.FAMILIES)
def test_reference_is_pinned_to_the_oracle(fam):
    assert [c.name for c in lc.family(fam)] == lc.names(fam)
    for case in lc.family(fam):
        ref, orc, fig = lc.reference(case), lc.oracle32(case), lc.oracle_figures(case)
        print("%-24s B %d A %d C %d N %d G %d | oracle32: R %.3g  dreg rows %s  losses %s"
              % (case.name, case.B, case.A, case.C, case.N, lc.focal_groups(case.B, case.A), fig["R"],
                 np.array2string(fig["dreg"], precision=3), np.array2string(fig["loss"], precision=3)))
        assert np.all(fig["loss"] <= 1e-6), case.name
        assert np.array_equal(ref.dcls != 0, orc.dcls != 0) and np.array_equal(ref.dreg != 0, orc.dreg != 0), case.name
        assert fig["exact"]
        # inside the envelope with an R of a few roundings: a*a, the weight, the logarithm, two products, the mean's scale
        assert fig["R"] <= 8 * U, (case.name, fig["R"])
        assert np.all(np.isfinite(fig["dreg"])) and np.all(fig["dreg"] <= 1e-3), (case.name, fig["dreg"])
        assert np.isfinite(ref.dcls).all() and np.isfinite(ref.dreg).all() and np.isfinite(ref.losses).all()
    print(fam, {k: v for k, v in lc.family_figures(fam).items()})


def test_golden_figures_are_the_measured_ones():
    """The golden case: R about 1.2e-7 where the plain relative error is 1.9e-4 (no flat rtol can work), rows as measured."""
    for case, rows in zip(lc.family("fast_path_values"), ((1.1e-5, 1.8e-6, 5.9e-7), (1.4e-5,))):
        ref, orc, fig = lc.reference(case), lc.oracle32(case), lc.oracle_figures(case)
        nz = ref.dcls != 0
        plain = float((np.abs(orc.dcls[nz] - ref.dcls[nz]) / np.abs(ref.dcls[nz])).max())
        print(case.name, "plain relative error %.3g, R %.3g, cond max %.3g" % (plain, fig["R"], lc.cond_of(case)[nz].max()))
        assert plain > 1e-5 and fig["R"] < 2e-7
        assert np.all(fig["dreg"] <= 1.5 * np.array(rows)) and np.all(fig["dreg"] >= np.array(rows) / 1.5)
    assert abs(float(lc.dcls_cond(np.array([1.0 - 1e-4]))[0]) - 1.2e-3) < 1e-4


@pytest.mark.parametrize("fam", lc.FAMILIES)
def test_float32_and_float64_assignments_agree(fam):
    for case in lc.family(fam):
        for a32, a64 in zip(lc.assignment(case), lc.assign_images(case, dtype=torch.float64)):
            assert (a32 is None) == (a64 is None)
            if a32 is not None:
                assert torch.equal(a32[2], a64[2]) and torch.equal(a32[1][a32[2] == 1], a64[1][a64[2] == 1]), case.name


@pytest.mark.parametrize("fam", [f for f in lc.FAMILIES if f != "fast_path_values"])
def test_regression_keeps_its_distance(fam):
    """Every positive is REG_GAP away from e == 0 and from the smooth-L1 kink, and its centre gradient does not cancel."""
    for case in lc.family(fam):
        for j, idx, gap, centre in lc.positive_gaps(case):
            assert gap.min() >= lc.REG_GAP and centre.min() >= lc.CENTRE_MIN, (case.name, j)


def test_golden_regression_keeps_its_distance():
    for case in lc.family("fast_path_values"):
        assert min(gap.min() for _, _, gap, _ in lc.positive_gaps(case)) >= lc.REG_GAP


# ------------------------------------------------------------------------------------------------ the paths
def test_focal_groups_mirror():
    assert lc.focal_groups(8, 389205) == 96 and lc.focal_groups(2, 389205) == 384 and lc.focal_groups(1, 389205) == 768
    assert lc.focal_groups(5, 2313) == 5 and lc.focal_groups(96, lc.QF_A) == 8 and lc.focal_groups(97, 3969) == 8
    assert lc.focal_groups(lc.QF2D_B, lc.QF_A) == 8 and lc.focal_groups(lc.QF2D_B - 1, lc.QF_A) == 16


@pytest.mark.parametrize("fam", ["queue_full", "queue_full_2d"])
def test_queue_full_fills_the_queue(fam):
    case = lc.family(fam)[0]
    B, A = case.B, case.A
    assert case.directional == (fam == "queue_full") and case.C == (8 if case.directional else 4)
    assert lc.focal_groups(B, A) == 8 and A % lc.UNIT == lc.UNIT - 37
    walk = lc.wave_units(B, A)
    assert sorted(len(u) for u in walk.values()) == [2] * 27 + [3] * 5          # an odd count of at least 3: A, B, A buffers
    assert [k for k, u in walk.items() if len(u) == 3] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)] and walk[1, 0][-1] == 68
    asg, st = lc.assignment(case), _states(case)
    for j in (0, 1):
        assert (st[j] == 1).all() and float(asg[j][0].min()) >= 0.6
        for u in walk.values():
            assert all((st[j][k * lc.UNIT:(k + 1) * lc.UNIT] == 1).sum() == lc.UNIT for k in u[:2])
        # qn reaches QCAP exactly; the five waves with a third unit break, drain and re-issue unprimed
        assert lc.queue_trace(B, A, st[j]) == (lc.QCAP, 5)
    assert set(asg[0][3].tolist()) == {1, 2} and set(asg[1][1].tolist()) == {1, 2}  # image 1: rows behind an invalid one
    assert (st[2][:lc.QF_SPLIT] == 1).all() and (st[2][lc.QF_SPLIT:] == 0).all() and lc.queue_trace(B, A, st[2]) == (lc.UNIT, 0)
    assert st[3] is None
    assert (st[4] == 0).all() and bool((case.ann[4, :, lc.cls_col(case.directional)] != -1).any())   # labels, npos == 0
    frac = [float((s == 1).mean()) for s in st[5:]]
    assert max(frac) < 0.05 and sum(f > 0 for f in frac) >= 5 and all((s == -1).any() for s in st[5:])
    if fam == "queue_full_2d":
        assert lc.focal_groups(B - 1, A) > 8                                        # the smallest such batch


def test_tail_sizes_reach_the_small_grids():
    cases = {c.name: c for c in lc.family("tail_sizes")}
    assert sorted({c.A for c in cases.values()}) == sorted(lc.TAIL_A)
    for A in lc.TAIL_A:
        for d, C in ((True, 8), (False, 4)):
            c = cases["tail_A%d_%s_C%d" % (A, "dir" if d else "2d", C)]
            assert c.B == 2 and torch.equal(c.anchors[0], lc.anchor_table(lc.TAIL_HW[A <= 2313])[:A])
            st = np.concatenate(_states(c))
            if A >= 64:
                assert (st == 1).any() and (st == -1).any() and (st == 0).any()
    assert all(("tail_A%d_dir_C3" % A) in cases and ("tail_A%d_2d_C3" % A) in cases for A in lc.TAIL_C3)
    units = lambda A: (A + lc.UNIT - 1) // lc.UNIT
    assert all(lc.focal_groups(2, A) == 1 for A in lc.TAIL_A if A <= 512)          # one workgroup, waves past the units idle
    assert lc.focal_groups(2, 513) == 2 and units(513) == 5                         # G = need < 8: three idle waves
    assert lc.focal_groups(2, 3969) == 8 and units(3969) == 32 and 3969 % lc.UNIT == 1          # need == 8 exactly
    for A in (1, 129, 513, 3969):                                                   # the last unit holds one anchor ...
        assert A % lc.UNIT == 1
    st = _states(cases["tail_A3969_dir_C8"])
    assert st[0][3968] == 1                                                         # ... and it is a positive


def test_many_labels_cross_the_register_boundary():
    cases = {c.name: c for c in lc.family("many_labels")}
    assert sorted({c.N for c in cases.values()}) == sorted(lc.ML_N) and max(lc.ML_N) == lc.MAX_GT
    for c in cases.values():
        cc, N = lc.cls_col(c.directional), c.N
        asg = lc.assignment(c)
        r = min(63, N - 1)
        assert float(c.ann[0, r, cc]) == np.float32(2.7) and bool((c.ann[0, :, cc] != -1).all())
        hit = (asg[0][2] == 1) & (asg[0][1] == r)
        assert int(hit.sum()) >= 20 and set(asg[0][3][hit].tolist()) == {2}       # 2.7 truncates to 2
        if N > 64:                                                                  # the tie: rows 63 and 64, first maximum wins
            box = slice(16, 20) if c.directional else slice(0, 4)
            assert torch.equal(c.ann[0, 63, box], c.ann[0, 64, box]) and float(c.ann[0, 64, cc]) == 3.0
            assert not bool((asg[0][1] == 64).any())
            alone = lc.assign_images(c, torch.cat((c.ann[:, :63], c.ann[:, 64:]), 1))[0]
            assert torch.equal(alone[0], asg[0][0]) and int(((alone[1] == 63) & (alone[2] == 1)).sum()) == int(hit.sum())
        if N > 65:
            assert bool(((asg[0][1] > 64) & (asg[0][2] == 1)).any())                # positives that only the LDS rows give
        assert int((c.ann[1, :, cc] != -1).sum()) == 1 and float(c.ann[1, N - 1, cc]) == 1.0
        assert bool((asg[1][2] == 1).any()) and bool((asg[1][1] == N - 1).all())
        assert bool((c.ann[2, :, cc] != -1).all()) and float(asg[2][0].max()) == 0.0 and bool((asg[2][2] == 0).all())


def test_thresholds_are_bit_exact():
    for c in lc.family("thresholds"):
        for j in range(c.B):
            iou, row, state = (t.numpy() for t in lc.assignment(c)[j][:3])
            for i, kind in enumerate(c.kinds):
                a = c.first + i
                assert iou[a] == lc.th_expected_iou(kind), (kind, iou[a])
                assert state[a] == lc.TH_STATE[kind]
                assert row[a] == (i if j == 0 else len(c.kinds) - 1 - i)
            far = np.ones(c.A, bool)
            far[c.first:c.first + len(c.kinds)] = False
            assert (iou[far] == 0).all()
        assert np.float32(0.5) == 0.5 and lc.th_expected_iou("two_fifths") == np.float32(0.4)
        # anchors and box corners are small integers but for the one scaled edge
        special = c.anchors[0, c.first:c.first + len(c.kinds)]
        assert torch.equal(special, special.round()) and float(special.max()) < 4096


def test_clamp_edges_cover_every_place():
    for c in lc.family("clamp_edges"):
        vals = lc.clamp_values()
        seen = {(where, v) for where, _, _, _, v in c.plan}
        assert seen == {(w, v) for w in lc.CLAMP_WHERE for v in range(len(vals))}
        ref, orc = lc.reference(c), lc.oracle32(c)
        st = _states(c)
        for where, j, a, col, v in c.plan:
            assert c.cls[j, a, col].numpy() == vals[v]
            assert st[j][a] == (1 if where.startswith("positive") else 0)
            assert bool(lc.plain_units(lc.assignment(c)[j][2])[a]) == (where == "fast_path")
            passes = v in (0, 2, 3, 4)                                  # the bounds themselves and one ulp inside
            assert (ref.dcls[j, a, col] != 0) == passes and (orc.dcls[j, a, col] != 0) == passes, (where, v)


def test_full_size_and_big_batches_reach_the_epilogue_loops():
    c = lc.family("one_image_full_size")[0]
    assert c.B == 1 and c.A == 389205 and c.C == 8 and c.N == 10 and lc.focal_groups(1, c.A) == 768 > 2 * lc.NTHR
    big = {c.name: c for c in lc.family("big_batch")}
    for name in ("batch_B300_A128_dir", "batch_B300_A128_2d"):
        c = big[name]
        assert c.B == 300 > lc.NTHR and c.A == 128 and c.C == 8 and lc.focal_groups(c.B, c.A) == 1
        has = [a is not None for a in lc.assignment(c)]
        assert 0 < sum(has) < c.B                                       # vp_images < B
    c = big["batch_B97_A3969_dir"]
    assert c.B > 96 and (lc.RESIDENT // c.B) & ~7 == 0 and lc.focal_groups(c.B, c.A) == 8   # the G < 8 floor decides


def test_golden_case_is_mostly_fast_path():
    for c in lc.family("fast_path_values"):
        plain = np.stack([np.ones(c.A, bool) if a is None else lc.plain_units(a[2]).numpy() for a in lc.assignment(c)])
        print(c.name, "share of dcls written by the fast path: %.3f" % plain.mean())
        assert plain.mean() > 0.25 and plain[2].all()


# ------------------------------------------------------------------------------------------------ wrong kernels
def _plain_mask(case):
    """[B,A] bool: the anchor's unit takes the packed fast path."""
    return np.stack([np.ones(case.A, bool) if a is None else lc.plain_units(a[2]).numpy() for a in lc.assignment(case)])


def wrong_kernel(case, kind):
    """(losses, dcls, dreg) of a kernel with one mistake: the float64 reference on other integer decisions, or its
    outputs altered afterwards, so that nothing but the mistake separates it from the reference.
      ge_to_gt      ``best >= 0.5f`` became ``>``            lt_to_le     ``best < 0.4f`` became ``<=``
      no_lds_rows   the ``c0 = 64`` loops are gone: label rows past 63 are never seen
      clamp_passes  ``p01.x == x.x`` became ``true``: the fast path passes the gradient at the clamped p outside the clamp
      fast_weight   -0.75f became -0.7501f in the fast path (backward only)"""
    ref, asg = lc.reference(case), lc.assignment(case)
    if kind in ("ge_to_gt", "lt_to_le"):
        moved = []
        for a in asg:
            if a is not None:
                st = a[2].clone()
                if kind == "ge_to_gt":
                    st[a[0] == 0.5] = -1
                else:
                    st[a[0] == float(np.float32(0.4))] = 0
                a = (a[0], a[1], st) + a[3:]
            moved.append(a)
        r = lc.reference_with(case, moved)
        return r.losses, r.dcls, r.dreg
    if kind == "no_lds_rows":
        r = lc.reference_with(case, lc.assign_images(case, case.ann[:, :64]))
        return r.losses, r.dcls, r.dreg
    plain = _plain_mask(case)[:, :, None]
    if kind == "fast_weight":
        return ref.losses, np.where(plain, ref.dcls * (0.7501 / 0.75), ref.dcls), ref.dreg
    if kind == "clamp_passes":
        x = case.cls.double().numpy()
        p = np.clip(x, lc.LO, lc.HI)
        npos = np.array([1 if a is None else max(int((a[2] == 1).sum()), 1) for a in asg], dtype=np.float64)
        g = lc.W_LOSS[0] / (case.B * npos[:, None, None]) * 0.75 * (-2.0 * p * np.log(1.0 - p) + p * p / (1.0 - p))
        inside = plain & (x >= lc.LO) & (x <= lc.HI)
        assert np.allclose(g[inside], ref.dcls[inside], rtol=1e-12, atol=0)      # the formula is the reference's where both apply
        return ref.losses, np.where(plain & (p != x), g, ref.dcls), ref.dreg
    raise KeyError(kind)


@pytest.mark.parametrize("kind,fam,name", [
    ("ge_to_gt", "thresholds", "thresholds_dir"), ("ge_to_gt", "thresholds", "thresholds_2d"),
    ("lt_to_le", "thresholds", "thresholds_dir"), ("lt_to_le", "thresholds", "thresholds_2d"),
    ("no_lds_rows", "many_labels", "labels_N65_dir"), ("no_lds_rows", "many_labels", "labels_N256_2d"),
    ("clamp_passes", "clamp_edges", "clamp_dir"), ("clamp_passes", "clamp_edges", "clamp_2d"),
    ("fast_weight", "fast_path_values", "golden_dir"), ("fast_weight", "fast_path_values", "golden_2d"),
    ("fast_weight", "one_image_full_size", "one_image_1080p")])
def test_the_comparison_rejects_a_wrong_kernel(kind, fam, name):
    case = lc.get(fam, name)
    good = lc.reference(case)
    assert lc.check((good.losses, good.dcls, good.dreg), case, fam)[0] == []
    orc = lc.oracle32(case)
    assert lc.check((orc.losses, orc.dcls, orc.dreg), case, fam)[0] == []
    bad, fig = lc.check(wrong_kernel(case, kind), case, fam)
    print(kind, name, bad)
    assert bad


@pytest.mark.parametrize("name", ["golden_dir", "golden_2d"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_the_comparison_rejects_what_is_not_a_number(name, value):
    """NaN or infinity in the losses, in dcls or in dreg alone -- everywhere the reference is not 0, or at one element --
    fails the comparison: what an overrun queue, a stale scale or 0/0 in the epilogue would most likely leave behind."""
    fam = "fast_path_values"
    case = lc.get(fam, name)
    o = lc.oracle32(case)
    ref = lc.reference(case)
    for k in range(3):
        for everywhere in (True, False):
            got = [o.losses.copy(), o.dcls.astype(np.float64), o.dreg.astype(np.float64)]
            if k == 0:
                got[0][:] = value
                if not everywhere:
                    got[0] = o.losses.copy()
                    got[0][-1] = value
            else:
                at = np.argwhere(ref.dcls != 0 if k == 1 else ref.dreg != 0)
                idx = tuple(at.T) if everywhere else tuple(at[len(at) // 2])
                got[k][idx] = value
            bad, fig = lc.check(got, case, fam)
            assert bad, (k, everywhere, fig)
            if k:                                               # the measure itself, without the finiteness line, says no
                meas = lc.dcls_excess(got[1], case)[0] if k == 1 else lc.dreg_metrics(got[2], case)[0]
                assert not np.all(meas <= 1.0)
            else:
                assert not np.all(lc.loss_rel(got[0], case) <= 1.0)

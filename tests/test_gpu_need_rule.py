"""The need sets of the regression tower's forward (rn_reg_need_tiles, csrc/anchor_match.hip) held to the matching rule at its edges,
together with the two other users of the rule (csrc/anchor_match_dev.h): rn_assign and the fused loss (csrc/focal_loss.hip).  If the need
sets and the loss disagree about one positive anchor, the sparse forward hands the loss a tile nobody computed and nothing
raises; tests/test_gpu_sparse_reg_fwd.py places every label exactly on an anchor (IoU 1), so it cannot see such a disagreement.

Cases of tests/loss_cases.py: IoU exactly 0.5, one ulp below, exactly 0.4f and one ulp below that (thresholds); more than 64 label rows
with a tie across rows 63 / 64, an image whose only valid row is the last and an image without a positive (many_labels, on the pyramid of
the 96x128 anchor table: the level decode of need_p0_kernel); A = 3969, no multiple of 4, as one row of tiles (the last tile is partial).
Every expectation comes from the CPU assignment lc.assignment(case), which tests/test_loss_cases_host.py pins to oracle/losses.py; none
from a kernel.  Everything is exact."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import reg_need_cases as rc
from test_gpu_loss_edges import check_assign

pytestmark = pytest.mark.gpu

ML_EMPTY_IMAGE = 2                                      # many_labels: every row valid, all outside the anchors' window

CASES = [("thresholds", n, None, 1) for n in lc.names("thresholds")]
CASES += [("many_labels", "labels_N%d_%s" % (N, v), lc.ML_HW, 9) for N in (65, 256) for v in ("dir", "2d")]
CASES += [("tail_sizes", "tail_A3969_dir_C%d" % C, None, 1) for C in (8, 3, 4)]


def levels_of(case, hw):
    """The pyramid of an anchor table, or the anchors as one row of pixels with one anchor each: a tile is four consecutive anchors."""
    if hw is None:
        return [(1, case.A)]
    from retinanet_mi355x import arch
    return arch.pyramid_shapes(*hw)


def to_levels(per_anchor, hws, per_pixel):
    """[B, A] bool -> per level [B, H, W] bool: some anchor of the pixel is set."""
    out, off = [], 0
    for H, W in hws:
        cnt = H * W * per_pixel
        out.append(per_anchor[:, off:off + cnt].reshape(-1, H, W, per_pixel).any(axis=3))
        off += cnt
    assert off == per_anchor.shape[1]
    return out


def anchors_in_tiles(flags, hws, B, per_pixel):
    """Flag bytes in the tile order of rc.flat -> [B, A] bool: the anchor's pixel lies in a flagged tile."""
    out, off = [], 0
    for H, W in hws:
        TH, TW = rc.grid((H, W))
        m = flags[off:off + B * TH * TW].reshape(B, TH, TW) != 0
        off += B * TH * TW
        px = np.repeat(np.repeat(m, 4, axis=1), 4, axis=2)[:, :H, :W]
        out.append(np.repeat(px.reshape(B, H * W), per_pixel, axis=1))
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("fam,name,hw,per_pixel", CASES, ids=[c[1] for c in CASES])
def test_need_sets_hold_the_rule(dev, fam, name, hw, per_pixel):
    from retinanet_mi355x import conv, ops, _hip
    assert _hip.load().rn_check_device() == 0
    case = lc.get(fam, name)
    B, A = case.B, case.A
    hws = levels_of(case, hw)
    state = np.zeros((B, A), dtype=np.int64)            # the CPU assignment; an image without a valid row is all negative
    for j, asg in enumerate(lc.assignment(case)):
        if asg is not None:
            state[j] = asg[2].numpy()
    positive = state == 1
    want = rc.tiles_of_pixels(to_levels(positive, hws, per_pixel))
    T = sum(m.size for m in want)
    # the expectation is not vacuous: flagged and unflagged tiles in every image (but the one that is empty by design)
    per_image = sum(m.reshape(B, -1).sum(1) for m in want)
    for j in range(B):
        if fam == "many_labels" and j == ML_EMPTY_IMAGE:
            assert per_image[j] == 0
        else:
            assert 0 < per_image[j] < T // B, (name, j, per_image[j])
    if hw is None:
        assert (A % 4 != 0) == (fam == "tail_sizes") and T == B * ((A + 3) // 4)
    if fam == "tail_sizes":
        assert want[0][0, 0, -1]                        # the partial last tile holds a positive (the last anchor of image 0)

    anc, ann = case.anchors.to(dev), case.ann.to(dev)
    # 1. P0 of the need sets is the tiles that hold a positive anchor of the CPU assignment
    need = conv.reg_need_tiles(anc, ann, case.directional, B, hws, per_pixel)
    got = need.flags[0].cpu().numpy()
    assert np.array_equal(got[:T], rc.flat(want, T)), "%s: %d tiles differ" % (name, int((got[:T] != rc.flat(want, T)).sum()))
    # 2. rn_assign gives the CPU states
    check_assign(ops, dev, case)
    # 3. / 4. the fused loss writes a regression gradient at every positive anchor and nowhere outside the tiles of P0
    c = case.cls.to(dev).requires_grad_(True)
    r = case.reg.to(dev).requires_grad_(True)
    out = ops.focal_loss(c, r, anc, ann, case.directional)
    sum(w * o for w, o in zip(lc.W_LOSS, out)).sum().backward()
    touched = (r.grad != 0).any(dim=2).cpu().numpy()
    assert not (touched & ~anchors_in_tiles(got, hws, B, per_pixel)).any(), "%s: the loss reads outside P0" % name
    assert not (positive & ~touched).any(), "%s: a positive anchor without a regression gradient" % name

"""CPU: the containments the sparse forward of the regression tower rests on, on the numpy restatement of
tests/reg_need_cases.py.  A layer computed on a set S of tiles reads its input inside D(S); the backward's flags obey B[0] within D(P0) and
B[k+1] within D(B[k]); so with F[0] = P0, F[k] = D^(k+1)(P0) and E = D(P0):

  forward   D(F[0]) within F[1] (through E: the output layer's transform runs on E, D(E) = F[1]), D(F[k]) within F[k+1];
  backward  B[0] within E (the output layer's kept transform), B[k] within F[k] for k >= 1 (the kept transforms of conv4 .. conv1, the ReLU
            masks of their results).

Random positive sets on ragged grids -- (5 x 7), (3 x 3), (2 x 2), (1 x 1) tiles -- three images, one of them empty."""
import numpy as np
import pytest

import reg_need_cases as rc

GRIDS = [(5, 7), (3, 3), (2, 2), (1, 1)]


def random_p0(seed, density):
    rng = np.random.RandomState(seed)
    p0 = [rng.rand(3, th, tw) < density for th, tw in GRIDS]
    for m in p0:
        m[1] = False                                             # the image without positives
    return p0


def within(a, b):
    return all(not (x & ~y).any() for x, y in zip(a, b))


@pytest.mark.parametrize("seed,density", [(1, 0.05), (2, 0.15), (3, 0.4), (4, 1.0)])
def test_containments(seed, density):
    p0 = random_p0(seed, density)
    if density < 1.0:
        assert any(m.any() for m in p0) and not all(m[[0, 2]].all() for m in p0)
    F, E = rc.need_sets(p0)
    assert within(p0, E) and within(rc.dilate(E), F[1]) and within(F[1], rc.dilate(E))       # F[1] = D(E) = D^2(P0)
    for k in range(1, 4):
        assert within(rc.dilate(F[k]), F[k + 1])
    B = rc.backward_flags(p0)
    assert within(B[0], E)
    for k in range(1, 5):
        assert within(B[k], rc.dilate(B[k - 1]))
        assert within(B[k], F[k])
    for k in range(5):                                           # nothing crosses into the empty image
        assert not any(m[1].any() for m in F[k]) and not any(m[1].any() for m in B[k])


def test_dilation_stays_on_its_grid():
    p0 = [np.zeros((3, th, tw), dtype=bool) for th, tw in GRIDS]
    p0[0][0, 4, 6] = True                                        # the last tile of image 0 of the first level
    F, E = rc.need_sets(p0)
    assert E[0][0].sum() == 4 and not E[0][1].any() and not any(m.any() for m in E[1:])
    assert F[4][0][0].sum() == 30 and not F[4][0][1:].any()      # D^5 from a corner of 5 x 7: rows 0..4 x columns 1..6
    flat = rc.flat(F[0], 256)
    assert flat.sum() == 1 and flat[4 * 7 + 6] == 1


def test_tiles_of_pixels_on_a_ragged_map():
    m = np.zeros((1, 10, 14), dtype=bool)
    m[0, 9, 13] = m[0, 0, 4] = True
    t = rc.tiles_of_pixels([m])[0]
    assert t.shape == (1, 3, 4) and t.sum() == 2 and t[0, 2, 3] and t[0, 0, 1]

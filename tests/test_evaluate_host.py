"""CPU: the restatement of the scoring (tests/evaluate_restate.py) pinned -- the cell counts to an enumeration with Python sets, the
Betti numbers to shapes whose topology is known, the surface distances to scipy.ndimage.distance_transform_edt, the degenerate cases to
what the contract fixes, and all of it to known answers."""
import itertools
import math

import numpy as np
import pytest
import scipy.ndimage as ndi

import evaluate_restate as R
import skeleton_restate as S


def _cells_by_sets(m):
    """every cell of the closed cubical complex as a tuple of doubled coordinates: a voxel p is (2 p + 1) on every axis, and its faces,
    edges and vertices are the points at offsets -1 / 0 / +1 from it"""
    found = [set(), set(), set(), set()]
    for p in zip(*np.nonzero(m)):
        for off in itertools.product((-1, 0, 1), repeat=3):
            cell = tuple(2 * int(c) + 1 + o for c, o in zip(p, off))
            found[sum(c & 1 for c in cell)].add(cell)
    n = [len(s) for s in found]
    return n[0], n[1], n[2], n[3], n[0] - n[1] + n[2] - n[3]


def test_cells_of_every_2x2x2_mask():
    for bits in range(256):
        m = np.array([(bits >> i) & 1 for i in range(8)], np.uint8).reshape(2, 2, 2)
        assert R.cells(m) == _cells_by_sets(m), bits


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 4), (3, 1, 2), (2, 3, 4), (4, 4, 4)])
def test_cells_of_small_random_masks(shape):
    for p in (0.0, 0.2, 0.5, 0.8, 1.0):
        for seed in range(4):
            m = S.bernoulli(shape, p, seed)
            assert R.cells(m) == _cells_by_sets(m), (shape, p, seed)
    one = np.zeros(shape, np.uint8)
    one[-1, -1, -1] = 1
    assert R.cells(one) == (8, 12, 6, 1, 1)                          # a voxel in the high corner: the cells on the high faces count


KNOWN = [
    (S.torus, (1, 1, 0), 0), (S.hollow_shell, (1, 0, 1), 2), (S.tubes_and_torus, (2, 1, 0), 1),
    (lambda: S.bernoulli((9, 10, 129), 0.3), (8, 825, 3), -814), (lambda: S.bernoulli((9, 10, 129), 0.5), (1, 863, 44), -818),
    (lambda: S.bernoulli((9, 10, 129), 0.9), (1, 0, 492), 493), (lambda: S.bernoulli((17, 9, 65), 0.3), (11, 728, 3), -714),
]


@pytest.mark.parametrize('case', range(len(KNOWN)))
def test_betti_numbers_and_euler_of_known_shapes(case):
    make, betti, chi = KNOWN[case]
    m = make()
    assert R.betti(m) == betti and R.euler(m) == chi
    assert betti[1] == betti[0] + betti[2] - chi


def test_betti_numbers_of_simple_solids():
    solid = np.ones((3, 4, 5), np.uint8)
    assert R.betti(solid) == (1, 0, 0) and R.euler(solid) == 1
    two = np.zeros((3, 3, 5), np.uint8)
    two[1, 1, 0] = two[1, 1, 4] = 1
    assert R.betti(two) == (2, 0, 0)
    diag = np.zeros((2, 2, 2), np.uint8)
    diag[0, 0, 0] = diag[1, 1, 1] = 1                                # joined through a corner: one 26-component, and the complex agrees
    assert R.betti(diag) == (1, 0, 0) and R.euler(diag) == 1
    ring = np.ones((3, 3, 1), np.uint8)
    ring[1, 1, 0] = 0                                                # the hole reaches the faces z = 0 and z = 0: a tunnel, not a cavity
    assert R.betti(ring) == (1, 1, 0)
    assert R.betti(np.zeros((2, 3, 4), np.uint8)) == (0, 0, 0) and R.euler(np.zeros((2, 3, 4), np.uint8)) == 0


def test_surface_is_the_mask_without_its_erosion():
    m = S.bernoulli((9, 10, 129), 0.3)
    assert int(R.surface(m).sum()) == 3409
    box = np.ones((4, 5, 6), np.uint8)
    s = R.surface(box)
    assert int(s.sum()) == 4 * 5 * 6 - 2 * 3 * 4 and not s[1:-1, 1:-1, 1:-1].any()       # a solid volume: the faces of the volume are surface


def test_surface_distances_against_scipy():
    P, T = R.shifted_pair()
    for sampling in (None, (0.5, 1.0, 2.5)):
        got = R.surface_distances(P, T, sampling)
        sp, st = R.surface(P) != 0, R.surface(T) != 0
        d_pt = ndi.distance_transform_edt(~st, sampling)[sp]
        d_tp = ndi.distance_transform_edt(~sp, sampling)[st]
        if sampling is not None:
            d_pt, d_tp = d_pt.astype(np.float32).astype(np.float64), d_tp.astype(np.float32).astype(np.float64)
        for d, side in ((d_pt, got['pred_to_truth']), (d_tp, got['truth_to_pred'])):
            assert side['count'] == len(d)
            assert side['max'] == pytest.approx(d.max(), rel=1e-6) and side['mean'] == pytest.approx(d.mean(), rel=1e-6)
            assert side['percentile'] == pytest.approx(np.sort(d)[int(np.ceil(0.95 * len(d))) - 1], rel=1e-6)
        assert got['hausdorff'] == pytest.approx(max(d_pt.max(), d_tp.max()), rel=1e-6)
        assert got['assd'] == pytest.approx((d_pt.sum() + d_tp.sum()) / (len(d_pt) + len(d_tp)), rel=1e-6)


def test_known_answers_of_the_shifted_pair():
    P, T = R.shifted_pair()
    f = R.evaluate(P, T)
    assert (f['tp'], f['fp'], f['fn'], f['tn']) == (856, 362, 401, 21421) and f['dice'] == 1712 / 2475
    assert (f['surface_truth'], f['surface_pred']) == (862, 838)
    assert (f['truth_to_pred']['max_key'], f['pred_to_truth']['max_key']) == (10, 2)
    assert (f['truth_to_pred']['mean'], f['pred_to_truth']['mean']) == (0.7204904825988472, 0.6675587274013999)
    assert f['truth_to_pred']['percentile_key'] == 1 and f['pred_to_truth']['percentile_key'] == 1
    assert (f['tprec'], f['tsens'], f['cldice']) == (0.9795918367346939, 0.9504950495049505, 0.964824120603015)
    assert f['betti_truth'] == (2, 1, 0) and f['euler_truth'] == 1


def test_ranks():
    assert [R.rank(q, 20) for q in (0.5, 0.95, 1.0, 0.05, 0.04)] == [9, 18, 19, 0, 0]
    assert R.rank(0.95, 0) == 0 and R.rank(1.0, 1) == 0
    assert R.rank(0.07, 100) == 7                                    # 0.07 * 100 is 7.000000000000001 in fp64: the ceiling is 8


def test_degenerate_cases():
    z, m = np.zeros((3, 4, 5), np.uint8), S.bernoulli((3, 4, 5), 0.4)
    both = R.evaluate(z, z)
    assert all(both[k] == 1.0 for k in ('dice', 'iou', 'precision', 'recall', 'cldice', 'tprec', 'tsens'))
    assert both['hausdorff'] == both['hausdorff_percentile'] == both['assd'] == 0.0 and both['specificity'] == 1.0
    for p, t in ((z, m), (m, z)):
        one = R.evaluate(p, t)
        assert all(one[k] == 0.0 for k in ('dice', 'iou', 'precision', 'recall', 'cldice'))
        assert one['hausdorff'] == one['hausdorff_percentile'] == one['assd'] == math.inf
    full = np.ones((3, 4, 5), np.uint8)
    assert math.isnan(R.evaluate(full, full)['specificity']) and R.evaluate(full, full)['dice'] == 1.0
    a, b = np.zeros((3, 3, 9), np.uint8), np.zeros((3, 3, 9), np.uint8)
    a[1, 1, 0:3] = 1
    b[1, 1, 6:9] = 1
    apart = R.evaluate(a, b)
    assert apart['dice'] == 0.0 and apart['tprec'] == apart['tsens'] == 0.0 and math.isnan(apart['cldice'])

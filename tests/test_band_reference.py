"""tests/band_reference.py, the statement ensemble_band_kernel is compared with on the device (tests/test_ensemble_band_gpu.py),
pinned without one: the mean's summation tree against math.fsum, the bounds on rows with NaN, +-inf and ties, and the
kernel's sorting network restated in numpy -- with the NaN members counted and kept out of the list it gives np.sort's
bounds on every designed row; with a NaN in the list, as the kernel once had it, even the finite bounds are out of place."""
import math

import numpy as np
import pytest

from band_reference import (EDGE_ROWS, FINITE_ROWS, band_rows, bitonic_rows, designed_row, mean_rows, same_rows)
from fokl_gpy_amd.GP_Integrate import bounds_cut

COUNTS = (2, 3, 70, 255, 256, 257, 1024, 1025)


def _cuts(E):
    return sorted({1, bounds_cut(E), E - 1} & set(range(1, E)))


@pytest.mark.parametrize('E', COUNTS + (4097, 16384))
def test_mean_rows_is_within_the_rounding_of_a_sum(E):
    """E - 1 additions, each rounding by at most 2^-53 of a partial sum that never exceeds E max|x|: the tree's mean is
    within E 2^-52 max|x| of the exact mean (math.fsum), for every column."""
    rng = np.random.default_rng(E)
    members = np.stack([rng.standard_normal(E), 1e6 + rng.random(E), rng.standard_normal(E) * 10.0 ** rng.integers(-8, 8, E)],
                       axis=1)
    got = mean_rows(members)
    assert got.shape == (3,)
    for c in range(3):
        exact = math.fsum(members[:, c].tolist()) / E
        assert abs(got[c] - exact) <= E * 2.0 ** -52 * np.max(np.abs(members[:, c]))


def test_mean_rows_follows_the_kernels_order_of_additions():
    # 2^53 + 1 + 1: left to right the ones are lost one by one, in another order they are not -- the order is the kernel's
    big = 2.0 ** 53
    members = np.zeros(513)
    members[0], members[256], members[512] = big, 1.0, 1.0            # one thread's stride: (0 + big + 1) + 1 = big
    assert mean_rows(members) == big / 513
    members = np.zeros(513)
    members[0], members[1], members[129] = big, 1.0, 1.0              # threads 1 and 129 meet in the tree first: big + 2
    assert mean_rows(members) == (big + 2.0) / 513
    # exact on integers, whatever the order; the shape of a block of rows is kept
    block = np.random.default_rng(0).permutation(3 * 700).astype(np.float64).reshape(700, 3)
    assert np.array_equal(mean_rows(block), block.sum(0) / 700) and mean_rows(block[:, :, None]).shape == (3, 1)
    # NaN, and inf - inf, are NaN; inf alone stays inf; -0.0 joins the 0.0 a partial sum starts from
    assert np.isnan(mean_rows(np.array([1.0, np.nan, 2.0]))) and np.isnan(mean_rows(np.array([np.inf, -np.inf])))
    assert mean_rows(np.array([np.inf, 1.0])) == np.inf
    assert not np.signbit(mean_rows(np.array([-0.0, -0.0])))


def test_band_rows_on_nan_inf_and_ties():
    nan, inf = np.nan, np.inf
    row = np.array([0.0, nan, 2.0] + [float(v) for v in range(3, 70)])
    assert band_rows(row, 2) == (3.0, 69.0)                          # the NaN is the largest value: sorted[68] is 69
    assert band_rows(row, 1)[0] == 2.0 and np.isnan(band_rows(row, 1)[1])
    lo, hi = band_rows(np.array([inf, nan, -inf, 1.0, nan]), 2)
    assert lo == inf and np.isnan(hi)                                # -inf, 1, inf, nan, nan
    lo, hi = band_rows(np.array([inf, nan, -inf, 1.0, inf]), 1)
    assert lo == 1.0 and np.isnan(hi)
    lo, hi = band_rows(np.array([inf, nan, -inf, 1.0, inf]), 2)
    assert lo == inf and hi == inf                                   # NaN sorts after +inf
    lo, hi = band_rows(np.full(4, nan), 1)
    assert np.isnan(lo) and np.isnan(hi)
    assert band_rows(np.array([2.0, 2.0, 1.0, 2.0, 1.0]), 2) == (2.0, 2.0)
    lo, hi = band_rows(np.array([0.0, -0.0, -0.0, 0.0]), 1)
    assert lo == 0.0 and hi == 0.0 and same_rows(np.array([lo]), np.array([-0.0]))
    # a block of rows: axis 0 is the members
    block = np.array([[3.0, nan], [1.0, 5.0], [2.0, 4.0]])
    lo, hi = band_rows(block, 1)
    assert same_rows(lo, np.array([2.0, 5.0])) and same_rows(hi, np.array([3.0, nan]))
    assert not same_rows(np.array([1.0, nan]), np.array([1.0, 2.0])) and not same_rows(np.zeros(2), np.zeros(3))
    for bad in (0, 3, -1):
        with pytest.raises(ValueError):
            band_rows(block, bad)


@pytest.mark.parametrize('E', COUNTS)
def test_the_network_with_counted_nan_gives_numpys_bounds(E):
    rng = np.random.default_rng(1000 + E)
    for cut in _cuts(E):
        for kind in FINITE_ROWS + EDGE_ROWS:
            row = designed_row(kind, E, cut, rng)
            assert row.shape == (E,)
            want = band_rows(row, cut)
            got = bitonic_rows(row, cut)
            assert same_rows(np.array(got), np.array(want)), (kind, cut, got, want)
            if kind in FINITE_ROWS:                                  # finite rows never needed the count: both networks agree
                assert same_rows(np.array(bitonic_rows(row, cut, count_nan=False)), np.array(want)), (kind, cut)


def test_a_nan_in_the_list_misplaces_finite_bounds():
    """What the count is for: members 0, NaN, 2, 3, ..., 69 with cut 2.  np.sort gives (3, 69); the network with the NaN in
    its list gives (2, 68), both finite and both wrong."""
    row = np.array([0.0, np.nan, 2.0] + [float(v) for v in range(3, 70)])
    assert bitonic_rows(row, 2, count_nan=False) == (2.0, 68.0)
    assert bitonic_rows(row, 2) == band_rows(row, 2) == (3.0, 69.0)

"""fokl_predict on NaN and infinite draws: the three prediction kernels (csrc/fokl_predict.inc) against numpy's order.

The statement is the reference's (FR:966-978): ``np.sort`` along the draws puts NaN last, the bounds are
``(sorted[cut], sorted[draws - cut])`` and the mean is ``np.mean``.  For a row with D NaN predictions among ``draws``:
  * lower bound: NaN iff draws - D <= cut, else the (cut + 1)-th smallest number (-inf is a number);
  * upper bound: NaN iff D >= cut, else the (cut - D)-th largest number (+inf is a number);
  * mean: NaN with any NaN or with both infinities, +-inf with one of them, else the exact mean.
Columns and coefficients are small integers with chosen coefficients overwritten by NaN, +inf or -inf: every finite
prediction is an exact integer and the kind of every other one does not depend on the order of summation, so every
comparison is ``np.array_equal(..., equal_nan=True)``.  The reference product is formed element by element (a BLAS may
skip zero operands, and 0 x inf must be NaN).  Every path runs 70 rows: two 64-row blocks and five 16-row tiles, the last of
each ragged.
"""
import warnings

import numpy as np
import pytest

from fokl_gpy_amd import _capi, getKernels
from oracle import fokl_oracle as O
from test_predict_device import stage, run, expected_kernel, evaluate_cut, integer_case, check_exact, _model, _oracle_bound

gpu = pytest.mark.gpu

N = 70
# name -> (nc, draws, cut, valu forced)
PATHS = {
    'mfma': (5, 80, 3, False),
    'mfma_long_lists': (5, 100, 40, False),              # klo > PM_CAP: the buffers are as long as the lists
    'valu_forced': (5, 80, 3, True),
    'valu_under_the_hand_over': (5, 40, 2, False),
    'valu_global_lists': (5, 200, 160, False),
    'valu_wide': (301, 40, 2, False),
    'mean_only': (5, 80, None, False),
}
KERNELS = {
    'mfma': (_capi.PREDICT_MFMA, False), 'mfma_long_lists': (_capi.PREDICT_MFMA, False),
    'valu_forced': (_capi.PREDICT_VALU_LDS, False), 'valu_under_the_hand_over': (_capi.PREDICT_VALU_LDS, False),
    'valu_global_lists': (_capi.PREDICT_VALU_GLOBAL, False), 'valu_wide': (_capi.PREDICT_VALU_LDS, True),
    'mean_only': (_capi.PREDICT_VALU_LDS, False),
}


def reference(X, betas, cut):
    """(predictions, mean, bounds) as numpy has them: the product element by element, np.mean, np.sort."""
    draws = betas.shape[0]
    with np.errstate(all='ignore'):
        mod = (X[:, None, :] * betas[None, :, :]).sum(axis=2)
        mean = np.mean(mod, axis=1)
    finite = np.isfinite(mod)
    assert np.array_equal(mod[finite], np.rint(mod[finite])) and np.max(np.abs(mod[finite]), initial=0.0) * draws < 2.0 ** 52
    if cut is None:
        return mod, mean, None
    srt = np.sort(mod, axis=1)
    return mod, mean, np.stack([srt[:, cut], srt[:, draws - cut]], axis=1)


def same(got, want):
    return np.array_equal(got, want, equal_nan=True)


def check(name, X, betas, mean, bounds):
    cut = PATHS[name][2]
    mod, want_mean, want_bounds = reference(X, betas, cut)
    assert same(mean, want_mean), name
    if cut is not None:
        assert same(bounds[:, 0], want_bounds[:, 0]), name
        assert same(bounds[:, 1], want_bounds[:, 1]), name
    return mod, want_mean, want_bounds


def call(ctx, name, slots, betas, monkeypatch):
    nc, draws, cut, valu = PATHS[name]
    assert betas.shape == (draws, nc) and expected_kernel(nc, draws, cut, valu) == KERNELS[name]
    return run(ctx, slots, betas, cut, valu=valu, monkeypatch=monkeypatch)


def draw_order(draws):
    """Every draw once, in an order whose beginning holds draw 0 and the last draw (next to the padding draws), then one draw
    of every residue mod 16 (so of every four-draw group position and every quarter of the matrix-pipe kernel), then the
    whole 16-draw tile 16 .. 31, then the rest."""
    first = [0, draws - 1] + [r + 16 * (r % 2) for r in range(1, 16)] + list(range(16, 32))
    seen, order = set(), []
    for d in first + list(range(draws)):
        if d not in seen:
            seen.add(d)
            order.append(d)
    assert sorted(order) == list(range(draws))
    return np.array(order)


def kind(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))


# ---------------------------------------------------------------------------------------------------------
# 8. the rule of this file's docstring is numpy's order (no device)
# ---------------------------------------------------------------------------------------------------------

def rank_rule(row, cut):
    draws = row.shape[0]
    numbers = sorted(float(v) for v in row if v == v)
    D = draws - len(numbers)
    low = np.nan if draws - D <= cut else numbers[cut]
    high = np.nan if D >= cut else numbers[len(numbers) - (cut - D)]
    if D or (np.inf in numbers and -np.inf in numbers):
        mean = np.nan
    elif np.inf in numbers or -np.inf in numbers:
        mean = np.inf if np.inf in numbers else -np.inf
    else:
        mean = sum(numbers) / draws
    return mean, low, high


def test_the_rank_rule_is_numpys_order():
    rng = np.random.default_rng(8)
    seen = set()
    for _ in range(4000):
        draws = int(rng.integers(2, 13))
        cut = int(rng.integers(1, draws))
        row = rng.integers(-3, 4, draws).astype(np.float64)
        special = rng.random(draws)
        level = rng.choice([0.0, 0.2, 0.6, 1.0])
        row[special < level] = rng.choice([np.nan, np.inf, -np.inf], size=int((special < level).sum()))
        srt = np.sort(row)
        with np.errstate(all='ignore'):
            want = (np.mean(row), srt[cut], srt[draws - cut])
        got = rank_rule(row, cut)
        assert same(np.array(got), np.array(want)), (row, cut)
        seen.add(tuple(int(k) for k in kind(want)))
    assert len(seen) >= 12                                   # finite, NaN and both infinities occur in every place


# ---------------------------------------------------------------------------------------------------------
# 1. the same number of NaN predictions in every row
# ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', list(PATHS))
def test_nan_draws_at_both_seams_of_both_bounds(device_ctx, name, monkeypatch):
    nc, draws, cut, valu = PATHS[name]
    rng = np.random.default_rng(100 + draws + nc)
    cols, clean = integer_case(rng, N, nc, draws)
    slots, X = stage(device_ctx, cols)
    order = draw_order(draws)
    if cut is None:
        counts = [1, draws - 1, draws]
    else:
        counts = sorted({1, cut - 1, cut, cut + 1, draws - cut - 2, draws - cut - 1, draws - cut, draws - 1, draws} - {0})
    assert all(1 <= D <= draws for D in counts)
    for D in counts:
        betas = clean.copy()
        betas[order[:D], 0] = np.nan                         # the intercept: every row holds D NaN predictions
        mean, bounds = call(device_ctx, name, slots, betas, monkeypatch)
        mod, want_mean, want_bounds = check(name, X, betas, mean, bounds)
        assert np.all(np.isnan(mod).sum(axis=1) == D) and np.all(np.isnan(want_mean))
        if cut is not None:                                  # (the reference really crosses the seams)
            assert np.all(np.isnan(want_bounds[:, 0]) == (draws - D <= cut)) and np.all(np.isnan(want_bounds[:, 1]) == (D >= cut))
        if name == 'mfma':
            mean_v, bounds_v = call(device_ctx, 'valu_forced', slots, betas, monkeypatch)
            assert same(mean, mean_v) and same(bounds, bounds_v)


# ---------------------------------------------------------------------------------------------------------
# 2. infinities only: numbers like any other, at, below and above both ranks
# ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', list(PATHS))
def test_infinite_draws_are_numbers_at_both_ranks(device_ctx, name, monkeypatch):
    nc, draws, cut, valu = PATHS[name]
    rng = np.random.default_rng(200 + draws + nc)
    cols, clean = integer_case(rng, N, nc, draws)
    cols[:, :2] = rng.integers(1, 4, size=(N, 2))             # X columns 1 and 2 strictly positive: no 0 x inf
    slots, X = stage(device_ctx, cols)
    order = draw_order(draws)
    if cut is None:
        pairs = [(1, 0), (0, 1), (1, 1), (draws, 0)]
    else:
        few_p, few_m = (cut - 1, cut, cut + 1), (cut, cut + 1, cut + 2)                     # the upper / lower rank from outside
        many_p, many_m = (draws - cut - 1, draws - cut, draws - cut + 1), (draws - cut, draws - cut + 1, draws - cut + 2)
        pairs = [(p, m) for p in few_p for m in few_m]
        pairs += [pm for p in many_p for pm in ((p, 0), (p, draws - p))] + [pm for m in many_m for pm in ((0, m), (draws - m, m))]
        pairs = sorted({(p, m) for p, m in pairs if 0 <= p <= draws and 0 <= m <= draws and p + m <= draws and p + m > 0})
        assert any(p > draws - cut - 1 for p, m in pairs)
    for P, M in pairs:
        betas = clean.copy()
        betas[order[:P], 1] = np.inf
        betas[order[P:P + M], 2] = -np.inf
        mean, bounds = call(device_ctx, name, slots, betas, monkeypatch)
        mod, want_mean, want_bounds = check(name, X, betas, mean, bounds)
        assert not np.isnan(mod).any() and np.all((mod == np.inf).sum(axis=1) == P) and np.all((mod == -np.inf).sum(axis=1) == M)
        if cut is not None:
            assert not np.isnan(want_bounds).any()
            assert np.all((want_bounds[:, 1] == np.inf) == (P >= cut)) and np.all((want_bounds[:, 0] == -np.inf) == (M >= cut + 1))
            assert np.all((want_bounds[:, 0] == np.inf) == (P >= draws - cut))
            assert np.all((want_bounds[:, 1] == -np.inf) == (M >= draws - cut + 1))
        if name == 'mfma':
            mean_v, bounds_v = call(device_ctx, 'valu_forced', slots, betas, monkeypatch)
            assert same(mean, mean_v) and same(bounds, bounds_v)


# ---------------------------------------------------------------------------------------------------------
# 3. the NaN count differs from row to row: 0 x inf and inf - inf depend on the row's basis values
# ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', list(PATHS))
def test_nan_counts_that_differ_within_a_tile_and_a_block(device_ctx, name, monkeypatch):
    nc, draws, cut, valu = PATHS[name]
    rng = np.random.default_rng(1)
    cols, clean = integer_case(rng, N, nc, draws)
    slots, X = stage(device_ctx, cols)
    plus, minus = [0, 17, 34, draws - 1], [5, 17, draws - 17]
    k = cut if cut is not None else 3
    nans = [d for d in [21, draws - 2] + list(range(draws)) if d not in plus + minus]
    nans = list(dict.fromkeys(nans))[:k - 1]                 # cut - 1 NaN in every row; the infinities add 0 .. 6 by the row
    for with_nan in (True, False):
        betas = clean.copy()
        betas[plus, 2] = np.inf
        betas[minus, 3] = -np.inf
        if with_nan:
            betas[nans, 1] = np.nan
        mean, bounds = call(device_ctx, name, slots, betas, monkeypatch)
        mod, want_mean, want_bounds = check(name, X, betas, mean, bounds)
        D = np.isnan(mod).sum(axis=1)
        if with_nan and cut is not None:
            for rows in (16, 64):                            # one tile and one block hold D < cut, == cut and > cut together
                assert any(all(np.any(op(D[r0:r0 + rows], cut)) for op in (np.less, np.equal, np.greater))
                           for r0 in range(0, N, rows)), (rows, D)
            assert np.array_equal(np.isnan(want_bounds[:, 1]), D >= cut)
        if not with_nan:                                     # means of every kind
            assert set(np.unique(kind(want_mean))) >= {1, 2, 3}
        if name == 'mfma':
            mean_v, bounds_v = call(device_ctx, 'valu_forced', slots, betas, monkeypatch)
            assert same(mean, mean_v) and same(bounds, bounds_v)


# ---------------------------------------------------------------------------------------------------------
# 4. overflow from finite arguments
# ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', list(PATHS))
def test_overflow_from_finite_arguments(device_ctx, name, monkeypatch):
    nc, draws, cut, valu = PATHS[name]
    rng = np.random.default_rng(400 + draws + nc)
    cols, betas = integer_case(rng, N, nc, draws)
    big = (np.arange(N) % 3 == 0) & ~((np.arange(N) >= 32) & (np.arange(N) < 48))            # (one tile without such a row)
    cols[:, 3] = np.where(big, 1e200, 0.0)                   # X column 4
    slots, X = stage(device_ctx, cols)
    order = draw_order(draws)
    k = min(cut if cut is not None else 3, draws // 4)
    betas[:, 4] = 0.0
    betas[order[:k], 4] = 1e200                              # k draws overflow upwards, k + 1 downwards, in such a row
    betas[order[k:2 * k + 1], 4] = -1e200
    mean, bounds = call(device_ctx, name, slots, betas, monkeypatch)
    mod, want_mean, want_bounds = check(name, X, betas, mean, bounds)
    assert np.all(np.isfinite(mod[~big])) and np.all((mod[big] == np.inf).sum(axis=1) == k)
    assert np.all((mod[big] == -np.inf).sum(axis=1) == k + 1) and not np.isnan(mod).any()
    # rows of a zero are what they are without the column, whatever their tile mates overflow to
    keep = np.arange(nc) != 4
    check_exact(X[~big][:, keep], betas[:, keep], cut, mean[~big], None if cut is None else bounds[~big])
    assert np.all(np.isnan(mean[big]))
    if cut is not None:
        assert np.all((bounds[big, 1] == np.inf) == (k >= cut)) and np.all((bounds[big, 0] == -np.inf) == (k + 1 >= cut + 1))


# ---------------------------------------------------------------------------------------------------------
# 5. which pass ran
# ---------------------------------------------------------------------------------------------------------

@gpu
def test_a_non_finite_coefficient_sends_every_tile_through_the_fallback(device_ctx, monkeypatch):
    """As before the fix, and still true: the matrix-pipe kernel itself is unchanged.  With any coefficient that is not finite
    the host's mean and covariance of the draws are NaN, no value passes the filter, and every tile takes the fallback.  The
    rows come out right because a mean that is not finite sends the call through predict_kernel's repair pass afterwards,
    which counts each row's NaN predictions; the report stays the matrix-pipe kernel's."""
    for name in ('mfma', 'mfma_long_lists'):
        nc, draws, cut, valu = PATHS[name]
        rng = np.random.default_rng(500 + draws)
        cols, clean = integer_case(rng, N, nc, draws)
        slots, X = stage(device_ctx, cols)
        for value, column in ((np.nan, 0), (np.inf, 0), (-np.inf, 3), (np.nan, 4)):
            betas = clean.copy()
            betas[draws // 2, column] = value
            mean, bounds = call(device_ctx, name, slots, betas, monkeypatch)
            ran = device_ctx.predict_report()
            assert ran['kernel'] == _capi.PREDICT_MFMA and ran['tiles'] == 5 and ran['tiles_fallback'] == 5, ran
            check(name, X, betas, mean, bounds)


# ---------------------------------------------------------------------------------------------------------
# 6. nothing is left over
# ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name', list(PATHS))
def test_a_second_call_returns_the_same_bits_and_a_finite_call_is_exact_afterwards(device_ctx, name, monkeypatch):
    nc, draws, cut, valu = PATHS[name]
    rng = np.random.default_rng(600 + draws + nc)
    cols, clean = integer_case(rng, N, nc, draws)
    slots, X = stage(device_ctx, cols)
    betas = clean.copy()
    betas[draw_order(draws)[:(cut or 3) + 1], 0] = np.nan
    betas[[3, 20], 2] = np.inf
    betas[[7, 20], 3] = -np.inf
    first = call(device_ctx, name, slots, betas, monkeypatch)
    check(name, X, betas, *first)
    second = call(device_ctx, name, slots, betas, monkeypatch)
    assert same(first[0], second[0]) and (cut is None or same(first[1], second[1]))
    mean, bounds = call(device_ctx, name, slots, clean, monkeypatch)
    check_exact(X, clean, cut, mean, bounds)
    assert np.all(np.isfinite(mean)) and (cut is None or np.all(np.isfinite(bounds)))


# ---------------------------------------------------------------------------------------------------------
# 7. through the class
# ---------------------------------------------------------------------------------------------------------

@gpu
def test_evaluate_and_coverage3_with_a_flagged_chains_draws():
    rng = np.random.default_rng(700)
    phis = getKernels.bernoulli()
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        model = _model(rng, 4, 12, 3, 100)
        flagged = [7, 50, 99]
        model.betas[flagged] = np.nan                        # as resample leaves a flagged chain's rows: 3 = cut of 100 draws
        model.setnos = setnos = np.arange(100)
        x = rng.random((203, 4))
        assert evaluate_cut(100) == 3
        mean, bounds = model.evaluate(x, ReturnBounds=True)
        want = O.evaluate(x, model.betas, model.mtx, phis, O.KERNEL_BERNOULLI, 100, setnos, return_bounds=True)
        tol = _oracle_bound(model, x, np.abs(np.delete(model.betas, flagged, axis=0)).max(axis=0))
        assert np.all(np.isnan(want[0])) and np.all(np.isnan(want[1][:, 1])) and np.all(np.isfinite(want[1][:, 0]))
        assert np.array_equal(kind(mean), kind(want[0])) and np.array_equal(kind(bounds), kind(want[1]))
        assert np.all(np.abs(bounds[:, 0] - want[1][:, 0]) <= tol)

        data = rng.standard_normal(203)
        model.inputs, model.data = x, data
        mean_c, bounds_c, rmse = model.coverage3()
        assert same(mean_c, mean) and same(bounds_c, bounds)
        assert np.isnan(rmse) and np.isnan(O.coverage_rmse(want[0], data))

        # one flagged row fewer: the upper bound is a number again, one rank further in
        model.betas[99] = model.betas[98]
        mean, bounds = model.evaluate(x, ReturnBounds=True)
        want = O.evaluate(x, model.betas, model.mtx, phis, O.KERNEL_BERNOULLI, 100, setnos, return_bounds=True)
        assert np.all(np.isnan(want[0])) and np.all(np.isfinite(want[1]))
        assert np.array_equal(kind(mean), kind(want[0])) and np.array_equal(kind(bounds), kind(want[1]))
        assert np.all(np.abs(bounds - want[1]) <= tol[:, None])

        # the mean-draw shortcut of ReturnBounds=False: integer coefficients, infinities and a NaN
        for with_nan in (False, True):
            model = _model(rng, 4, 12, 3, 100)
            model.betas = rng.integers(-3, 4, size=model.betas.shape).astype(np.float64)
            model.betas[[0, 17], 2] = np.inf
            model.betas[[5, 40], 5] = -np.inf
            if with_nan:
                model.betas[21, 1] = np.nan
            model.setnos = setnos
            got = model.evaluate(x, ReturnBounds=False)
            want = O.evaluate(x, model.betas, model.mtx, phis, O.KERNEL_BERNOULLI, 100, setnos, return_bounds=False)
            assert np.array_equal(kind(got), kind(want))
            assert set(np.unique(kind(want))) == ({1} if with_nan else {1, 2, 3})

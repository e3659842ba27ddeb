"""The multistart optimiser on the MI355X: every solve of the kernel against the host statement (optimize.solve_host),
the assembled results, the native refusals, and the feature from a device fit to the optimum."""
import warnings

import numpy as np
import pytest

from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd import optimize as opt

PHIS = getKernels.bernoulli()
TABLE = getKernels.pack_phis(PHIS, getKernels.KERNEL_BERNOULLI)[0]
MAX_ITER, TOL = 60, 1e-10


def family(name):
    """(mtx, mean coefficients) of the three model families: 2 inputs; 8 inputs, two-way; 16 inputs with two orders
    per input, three-factor terms, one four-factor term and a row of zeros (the entries with a side list)."""
    rng = np.random.default_rng({'two': 1, 'eight': 2, 'sixteen': 3}[name])
    if name == 'two':
        mtx = np.array([[1, 0], [0, 1], [2, 0], [0, 2], [1, 1], [3, 0], [0, 3], [2, 1], [1, 2], [4, 0], [0, 4], [3, 2]])
        return mtx, np.array([0.3, 0.8, -0.5, 1.5, -1.2, 0.9, 0.7, -0.6, 0.5, 0.4, -2.0, 1.6, 0.8])
    m, orders, pairs, triples = (8, 3, 24, 0) if name == 'eight' else (16, 2, 40, 24)
    rows = []
    for j in range(m):
        for order in range(1, orders + 1):
            row = np.zeros(m, dtype=int)
            row[j] = order
            rows.append(row)
    for width, count in ((2, pairs), (3, triples)):
        for _ in range(count):
            row = np.zeros(m, dtype=int)
            row[rng.choice(m, width, replace=False)] = rng.integers(1, orders + 1, width)
            rows.append(row)
    if name == 'sixteen':
        rows.append(np.zeros(m, dtype=int))
        row = np.zeros(m, dtype=int)
        row[[1, 4, 9, 14]] = [1, 2, 1, 2]
        rows.append(row)
    mtx = np.array(rows)
    width = (mtx > 0).sum(axis=1)
    mean = rng.standard_normal(mtx.shape[0] + 1) * np.concatenate([[1.0], np.where(width <= 1, 1.0, 1.5)])
    # a negative coefficient on every second-order main effect: the model is not dominated by its corners
    for t, row in enumerate(mtx):
        if width[t] == 1 and row.max() == 2:
            mean[t + 1] = -abs(mean[t + 1]) - 0.5
    return mtx, mean


def draws_of(mean, count, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(mean * (1 + 0.1 * rng.standard_normal((count, mean.shape[0]))))


def projected_gradient(mtx, betas, x, sign, lo, hi):
    """max_j |P(x - g)_j - x_j| of every solve, with the host statement's value / gradient evaluation."""
    E, S, m = x.shape
    tt = opt.TermTable(np.ascontiguousarray(mtx, dtype=np.int32))
    _, _, g, _ = opt._evaluate(tt, TABLE, x.reshape(E * S, m), np.repeat(betas, S, axis=0), sign, 2)
    xt = x.reshape(E * S, m).T
    return np.max(np.abs(np.clip(xt - g, lo[:, None], hi[:, None]) - xt), axis=0).reshape(E, S)


def check_against_host(dev, host, mtx, betas, sign, lo, hi, label=''):
    """Whole solves by their results: the orders of the sums differ, which may flip a line-search test.  The iterates
    are compared one iteration at a time in test_optimize_step_gpu.py and test_optimize_system_step_gpu.py."""
    x, f, it, st = dev
    hx, hf, hit, hst = host
    assert x.shape == hx.shape and f.shape == hf.shape and st.dtype == np.int32 and it.dtype == np.int32
    assert np.all(x >= lo) and np.all(x <= hi)
    early = hit <= MAX_ITER - 2
    # status: equal wherever the host stopped two iterations short of the limit (a stalled solve has its projected
    # gradient at the rounding level of the tolerance: it may come out converged on the other side)
    settled = np.isin(hst, (opt.CONVERGED, opt.STALLED))
    assert np.array_equal(st[early & (hst == opt.NON_FINITE)], hst[early & (hst == opt.NON_FINITE)])
    assert np.all(np.isin(st[early & settled], (opt.CONVERGED, opt.STALLED)))
    agree = np.mean(st[early] == hst[early]) if early.any() else 1.0
    assert agree >= 0.995, (label, agree)
    assert np.all(np.isin(st[~early], (opt.CONVERGED, opt.ITERATION_LIMIT, opt.STALLED)))
    # the same optimum where both converged into the same basin -- and that is all but a few solves
    both = (st == opt.CONVERGED) & (hst == opt.CONVERGED)
    apart = np.max(np.abs(x - hx), axis=-1)
    same = both & (apart <= 1e-3)
    assert same.sum() >= 0.98 * both.sum(), (label, same.sum(), both.sum())
    scale = max(1.0, float(np.max(np.abs(hf[both])))) if both.any() else 1.0
    worst_f = float(np.max(np.abs(f - hf)[same])) if same.any() else 0.0
    worst_x = float(np.max(apart[same])) if same.any() else 0.0
    print(f"\n{label}: {st.size} solves, {int(both.sum())} converged on both sides ({int(same.sum())} in the same basin), "
          f"status agrees on {agree:.4f}, max |f - f_host| {worst_f:.2e}, max |x - x_host| {worst_x:.2e}, "
          f"iterations mean {it.mean():.1f} max {it.max()}")
    assert worst_f <= 1e-10 * scale and worst_x <= 1e-7
    # every converged end point passes the projected-gradient test when the host evaluates it
    pg = projected_gradient(mtx, betas, x, sign, lo, hi)
    assert np.all(pg[st == opt.CONVERGED] <= 1e-8), (label, pg[st == opt.CONVERGED].max())
    assert np.all(np.isfinite(f[st != opt.NON_FINITE]))


SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 64), (40, 32), (1000, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['two', 'eight', 'sixteen'])
def test_every_solve_matches_the_host_statement(device_ctx, name):
    mtx, mean = family(name)
    mtx32 = np.ascontiguousarray(mtx, dtype=np.int32)
    m = mtx.shape[1]
    lo, hi = np.zeros(m), np.ones(m)
    for E, S in SIZES:
        betas = draws_of(mean, E, 100 * E + S)
        starts = opt.start_points(S, lo, hi)
        args = (mtx32, betas, TABLE, lo, hi, starts, -1.0, MAX_ITER, TOL)
        dev = device_ctx.model_optimize(*args)
        check_against_host(dev, opt.solve_host(*args), mtx, betas, -1.0, lo, hi, f"{name} {E} x {S}")
        if (E, S) in ((1, 65), (40, 32)):
            again = device_ctx.model_optimize(*args)               # bit for bit
            assert all(np.array_equal(a, b) for a, b in zip(dev, again))


@pytest.mark.gpu
def test_assembled_results(device_ctx):
    mtx, mean = family('eight')
    betas = draws_of(mean, 120, 9)
    minmax = [[-2.0 + j, 3.0 + 2 * j] for j in range(8)]
    res = opt.optimize(betas, mtx, PHIS, minmax, starts=64, ReturnAll=True, device=device_ctx)
    E = 120
    assert res.x.shape == (E, 8) and res.f.shape == (E,) and res.x_all.shape == (E, 64, 8)
    assert np.array_equal(res.best_start, np.argmax(res.f_all, axis=1)) and np.array_equal(res.f, res.f_all.max(axis=1))
    assert np.array_equal(res.x, res.x_all[np.arange(E), res.best_start])
    assert np.array_equal(res.status, res.status_all[np.arange(E), res.best_start])
    cut = opt.bounds_cut(E)
    assert np.array_equal(res.f_bounds, np.sort(res.f)[[cut, E - cut]])
    assert np.array_equal(res.x_bounds, np.sort(res.x, axis=0)[[cut, E - cut]].T)
    assert res.f_mean == res.f.mean() and np.array_equal(res.x_mean, res.x.mean(axis=0))
    low, high = np.array(minmax).T
    assert np.all(res.x_all >= low) and np.all(res.x_all <= high)
    again = opt.optimize(betas, mtx, PHIS, minmax, starts=64, ReturnAll=True, device=device_ctx)
    for key in res:
        assert np.array_equal(res[key], again[key]), key
    plain = opt.optimize(betas, mtx, PHIS, minmax, starts=64, ReturnBounds=False, device=device_ctx)
    assert sorted(plain) == ['f', 'status', 'x'] and np.array_equal(plain.x, res.x)
    # 'mean' is 'draws' with the single averaged row
    mean_res = opt.optimize(betas, mtx, PHIS, minmax, starts=64, objective='mean', device=device_ctx)
    one = opt.optimize(betas.mean(axis=0), mtx, PHIS, minmax, starts=64, device=device_ctx)
    assert mean_res.x.shape == (8,) and np.array_equal(mean_res.x, one.x[0]) and mean_res.f == one.f[0]
    assert mean_res.status == one.status[0] and 'f_bounds' not in mean_res
    # the host statement finds the same best optimum for the mean
    host = opt.optimize_host(betas, mtx, PHIS, minmax, starts=64, objective='mean')
    assert abs(host.f - mean_res.f) <= 1e-10 * max(1.0, abs(host.f))


@pytest.mark.gpu
def test_fixed_input_minimum_user_starts_and_the_indefinite_hessian(device_ctx):
    mtx, mean = family('two')
    minmax = [[0.0, 2.0], [-1.0, 3.0]]
    betas = draws_of(mean, 5, 4)
    # one input fixed, minimised, from starts on the faces, in the corners and outside the box (clipped to it)
    box = [[0.25, 1.75], [1.0, 1.0]]
    starts = [[0.25, 1.0], [1.75, 1.0], [1.0, 1.0], [0.0, -1.0], [2.0, 3.0], [0.3, 2.9], [1.2, 0.0]]
    kw = dict(bounds=box, starts=starts, sense='min', ReturnAll=True)
    dev = opt.optimize(betas, mtx, PHIS, minmax, device=device_ctx, **kw)
    host = opt.optimize_host(betas, mtx, PHIS, minmax, **kw)
    assert np.all(dev.x_all[..., 1] == 1.0) and np.all(dev.x_all[..., 0] >= 0.25) and np.all(dev.x_all[..., 0] <= 1.75)
    assert np.array_equal(dev.status_all, host.status_all) and np.all(dev.status_all == opt.CONVERGED)
    assert np.max(np.abs(dev.x_all - host.x_all)) <= 1e-7 and np.max(np.abs(dev.f_all - host.f_all)) <= 1e-10
    assert np.array_equal(dev.f, dev.f_all.min(axis=1))
    # the product term: a saddle in the middle of the box, maxima in two opposite corners; starts beside the saddle
    # meet an indefinite Hessian (the modified pivot), the start on it stays (the gradient is zero there)
    saddle_mtx, saddle_betas = np.array([[1, 1]]), np.array([0.0, 1.0])
    starts = [[1.2, 1.1], [0.9, 0.8], [1.9, -0.9], [1.0, 2.0], [1.3, 0.6], [1.0, 1.0]]
    dev = opt.optimize(saddle_betas, saddle_mtx, PHIS, minmax, starts=starts, ReturnAll=True, device=device_ctx)
    host = opt.optimize_host(saddle_betas, saddle_mtx, PHIS, minmax, starts=starts, ReturnAll=True)
    assert np.array_equal(dev.x_all, host.x_all) and np.array_equal(dev.status_all, host.status_all)
    assert dev.x_all[0, 0].tolist() == [2.0, 3.0] and dev.x_all[0, 1].tolist() == [0.0, -1.0]
    assert dev.x_all[0, 5].tolist() == [1.0, 1.0] and dev.iterations_all[0, 5] == 0
    assert all(e.tolist() in ([2.0, 3.0], [0.0, -1.0]) for e in dev.x_all[0, :5])
    assert abs(dev.f[0] - np.polynomial.Polynomial(PHIS[0])(1.0) ** 2) <= 1e-14
    # the iteration limit is reported, not exceeded
    short = opt.optimize(betas, mtx, PHIS, minmax, starts=32, max_iter=2, ReturnAll=True, device=device_ctx)
    assert np.all(short.iterations_all <= 2) and opt.ITERATION_LIMIT in short.status_all


@pytest.mark.gpu
def test_native_refusals_launch_nothing(device_ctx):
    mtx, mean = family('two')
    mtx32 = np.ascontiguousarray(mtx, dtype=np.int32)
    betas = draws_of(mean, 2, 1)
    lo, hi, starts = np.zeros(2), np.ones(2), opt.start_points(4, np.zeros(2), np.ones(2))
    good = device_ctx.model_optimize(mtx32, betas, TABLE, lo, hi, starts, -1.0, MAX_ITER, TOL)
    assert np.all(good[3] == opt.CONVERGED)

    def refused(text, *args):
        with pytest.raises(_capi.FoklNativeError) as err:
            device_ctx.model_optimize(*args)
        assert err.value.code == -2 and text in str(err.value), str(err.value)
        report = device_ctx.optimize_report()
        assert report.pop('instance') == 'none' and set(report.values()) == {0}

    wide = np.zeros((1, 17), dtype=np.int32)
    wide[0, 0] = 1
    refused('at most 16', wide, np.ones((1, 2)), TABLE, np.zeros(17), np.ones(17), np.zeros((1, 17)), -1.0, 5, TOL)
    # 16 inputs x 3 orders: 48 factors need 144 + 136 + 48 values per solve, the LDS of a wavefront holds 288
    many = np.zeros((48, 16), dtype=np.int32)
    for j in range(16):
        for order in range(3):
            many[3 * j + order, j] = order + 1
    refused('a wavefront\'s LDS holds 288', many, np.ones((1, 49)), TABLE, np.zeros(16), np.ones(16), np.zeros((1, 16)),
            -1.0, 5, TOL)
    beyond = mtx32.copy()
    beyond[0, 0] = 21
    refused('outside the coefficient table', beyond, betas, TABLE, lo, hi, starts, -1.0, MAX_ITER, TOL)
    refused('inverted box', mtx32, betas, TABLE, np.array([0.6, 0.0]), np.array([0.4, 1.0]), starts, -1.0, MAX_ITER, TOL)
    refused('inverted box', mtx32, betas, TABLE, np.array([np.nan, 0.0]), hi, starts, -1.0, MAX_ITER, TOL)
    refused('one call runs at most', mtx32, np.ones((1 << 14, 13)), TABLE, lo, hi, opt.start_points(65, lo, hi), -1.0,
            MAX_ITER, TOL)
    refused('sign must be', mtx32, betas, TABLE, lo, hi, starts, 0.5, MAX_ITER, TOL)
    # the context is as it was: the same call, the same bits
    again = device_ctx.model_optimize(mtx32, betas, TABLE, lo, hi, starts, -1.0, MAX_ITER, TOL)
    assert all(np.array_equal(a, b) for a, b in zip(good, again))


@pytest.mark.gpu
def test_from_a_fit_to_the_optimum_and_back(device_ctx):
    """A small Bernoulli fit on the device, its posterior optimised through the method of the class, the optimum
    re-evaluated by `evaluate`; then the same backend fits again, bit for bit as before."""
    from fokl_gpy_amd import FoKLRoutines
    rng = np.random.default_rng(17)
    n = 500
    x = rng.random((n, 2)) * np.array([4.0, 2.0]) + np.array([-1.0, 10.0])
    u, v = (x[:, 0] + 1.0) / 4.0, (x[:, 1] - 10.0) / 2.0
    y = np.sin(3.0 * u) + 0.8 * v * (1.0 - v) * 4.0 - 0.5 * u * v + 0.02 * rng.standard_normal(n)

    def fit():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', burnin=60, draws=60, tolerance=2,
                                      UserWarnings=False, ConsoleOutput=False)
            np.random.seed(23)
            betas, mtx, _ = model.fit(x, y, clean=True)
        return model, np.array(betas), np.array(mtx)

    model, betas, mtx = fit()
    res = model.optimize(starts=64, ReturnAll=True)
    E = betas.shape[0]
    assert res.x.shape == (E, 2) and np.all(np.isin(res.status, (opt.CONVERGED, opt.STALLED)))
    low, high = np.array(model.minmax, dtype=float).T
    assert np.all(res.x >= low) and np.all(res.x <= high)
    # the data's maximum lies near u = 0.5, v = 0.5: the posterior of the optimum covers it
    assert res.x_bounds[0, 0] <= 1.2 <= res.x_bounds[0, 1] + 0.4 and res.f_bounds[0] <= res.f_mean <= res.f_bounds[1]
    # the host statement agrees on every draw's best value
    host = opt.optimize_host(betas, mtx, model.phis, model.minmax, starts=64)
    assert np.max(np.abs(host.f - res.f)) <= 1e-10 * max(1.0, np.max(np.abs(host.f)))
    # evaluate() at the optimum of the mean model reproduces its value
    best = model.optimize(objective='mean', starts=64)
    normalised = lambda point: np.tile((point - low) / (high - low), (3, 1))      # three rows: unmistakably [n, m]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        value = np.ravel(model.evaluate(normalised(best.x)))[0]
    assert abs(value - best.f) <= 1e-10 * max(1.0, abs(best.f)), (value, best.f)
    # ... and of single draws: evaluate with that draw as the only row
    for e in (0, E // 2, E - 1):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            single = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', UserWarnings=False, ConsoleOutput=False)
            single.minmax, single.betas, single.mtx, single.draws = model.minmax, betas[e:e + 1], mtx, 1
            value = np.ravel(single.evaluate(normalised(res.x[e])))[0]
        assert abs(value - res.f[e]) <= 1e-10 * max(1.0, abs(res.f[e])), (e, value, res.f[e])
    # the backend still fits, with unchanged results
    _, betas_again, mtx_again = fit()
    assert np.array_equal(mtx_again, mtx) and np.array_equal(betas_again, betas)

"""Constrained optimisation over a system of models on the MI355X: every solve of the kernel against the host statement
(optimize.solve_system_host), the optimality conditions recomputed without it, the reduction to `optimize`, the native
refusals, and the feature from two device fits of the JANAF CO2 table to the constrained optimum."""
import os
import warnings

import numpy as np
import pytest

from helpers import ROOT
from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd import optimize as opt

PHIS = getKernels.bernoulli()
BERN = 'Bernoulli Polynomials'
MAX_ITER, TOL, CTOL = 150, 1e-9, 1e-8


def random_model(rng, m, orders, pairs, triples=0):
    """(mtx, mean coefficients): main effects of every order, `pairs` two-factor and `triples` three-factor terms; the
    second-order main effects are negative, so the model is not dominated by its corners."""
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
    mtx = np.array(rows)
    width = (mtx > 0).sum(axis=1)
    mean = rng.standard_normal(mtx.shape[0] + 1) * np.concatenate([[1.0], np.where(width <= 1, 1.0, 1.5)])
    for t, row in enumerate(mtx):
        if width[t] == 1 and row.max() == 2:
            mean[t + 1] = -abs(mean[t + 1]) - 0.5
    return mtx, mean


def with_draws(mtx, mean, minmax, count, seed):
    rng = np.random.default_rng(seed)
    betas = mean * (1 + 0.1 * rng.standard_normal((count, mean.shape[0])))
    return dict(betas=np.ascontiguousarray(betas), mtx=mtx, phis=PHIS, minmax=minmax, kernel=BERN)


def system(name, draws):
    """The arguments of optimize_system for three seeded families:
    'two'      1 model over 2 variables, its output pinned (an equality), the objective a variable;
    'eight'    2 models over 8 variables that share three of them under different training ranges, a two-sided range
               on the second model's output, the first model's output maximised;
    'sixteen'  3 models over 16 variables: the first model's output is the sixteenth variable (an intermediate) read by
               the third, whose output is minimised under a ceiling on the second's; three-factor terms."""
    rng = np.random.default_rng({'two': 21, 'eight': 22, 'sixteen': 23}[name])
    if name == 'two':
        mtx = np.array([[1, 0], [0, 1], [2, 0], [0, 2], [1, 1], [3, 0], [0, 3], [2, 1], [1, 2], [4, 0], [0, 4], [3, 2]])
        mean = np.array([0.3, 0.8, -0.5, 1.5, -1.2, 0.9, 0.7, -0.6, 0.5, 0.4, -2.0, 1.6, 0.8])
        model = with_draws(mtx, mean, [[0.0, 2.0], [-1.0, 3.0]], draws, 31)
        return ([model], [['u', 'v']], ['y'], 'u'), dict(sense='max', constraints={'y': (0.2, 0.2)})
    if name == 'eight':
        names = [f'x{j}' for j in range(8)]
        first = with_draws(*random_model(rng, 6, 3, 10), [[0.0, 1.0 + j] for j in range(6)], draws, 32)
        second = with_draws(*random_model(rng, 5, 2, 6), [[-0.5, 2.5 + j] for j in range(3, 6)] + [[0.0, 1.0]] * 2, draws, 33)
        level = float(np.mean(second['betas'][:, 0]))
        return ([first, second], [names[:6], names[3:]], ['gain', 'load'], 'gain'), \
            dict(sense='max', constraints={'load': (level - 0.4, level + 0.2)})
    names = [f'x{j}' for j in range(15)]
    first = with_draws(*random_model(rng, 6, 2, 6, 3), [[0.0, 1.0]] * 6, draws, 34)
    first['betas'] *= 0.25                                            # 'w' stays inside the range the third model reads it in
    second = with_draws(*random_model(rng, 11, 1, 10, 4), [[0.0, 2.0]] * 11, draws, 35)
    third = with_draws(*random_model(rng, 6, 2, 8, 2), [[-1.0, 3.0]] * 5 + [[-4.0, 4.0]], draws, 36)
    ceiling = float(np.mean(second['betas'][:, 0])) + 0.3
    return ([first, second, third], [names[:6], names[4:], names[10:] + ['w']], ['w', 'load', 'cost'], 'cost'), \
        dict(sense='min', constraints={'load': (None, ceiling)})


def check_against_host(dev, host, label):
    """Whole solves by their results: the orders of the sums differ, which may flip a line-search test.  The iterates
    are compared one iteration at a time in test_optimize_step_gpu.py and test_optimize_system_step_gpu.py."""
    x, f, viol, y, mu, it, st = dev
    hx, hf, hviol, hy, hmu, hit, hst = host
    assert x.shape == hx.shape and y.shape == hy.shape and mu.shape == hmu.shape and st.dtype == np.int32
    early = hit <= MAX_ITER - 2
    agree = float(np.mean(st[early] == hst[early])) if early.any() else 1.0
    both = (st == opt.CONVERGED) & (hst == opt.CONVERGED)
    apart = np.max(np.abs(x - hx), axis=-1)
    same = both & (apart <= 1e-3)
    flips = int(np.sum(early & (st != hst)))
    worst = lambda a, b: float(np.max(np.abs(a - b)[same])) if same.any() else 0.0
    print(f"\n{label}: {st.size} solves, host statuses {np.bincount(hst.ravel(), minlength=5).tolist()}, device "
          f"{np.bincount(st.ravel(), minlength=5).tolist()}, {int(both.sum())} converged on both sides ({int(same.sum())} in "
          f"the same basin), {flips} status flips, max |x - x_host| {worst(x, hx):.2e}, |f - f_host| {worst(f, hf):.2e}, "
          f"|violation - host's| {worst(viol, hviol):.2e}, iterations mean {it.mean():.1f} max {it.max()}")
    # statuses: equal except where the host statement itself sits within rounding of a line-search or tolerance decision
    assert agree >= 0.99 and flips <= max(2, st.size // 100), (label, agree, flips)
    assert np.array_equal(st[early & (hst == opt.NON_FINITE)], hst[early & (hst == opt.NON_FINITE)])
    assert both.sum() >= 0.5 * st.size and same.sum() >= 0.98 * both.sum(), (label, both.sum(), same.sum())
    assert worst(x, hx) <= 1e-7 and worst(f, hf) <= 1e-7 * max(1.0, float(np.max(np.abs(hf[same])))) and worst(viol, hviol) <= 1e-7
    assert worst(y, hy) <= 1e-7 * max(1.0, float(np.max(np.abs(hy[same]))))
    assert np.all(viol[st == opt.CONVERGED] <= CTOL) and np.all(viol[st == opt.INFEASIBLE] > CTOL)
    assert np.all(np.isfinite(f[st != opt.NON_FINITE]))


def prepared(name, E, S):
    args, kw = system(name, E)
    return opt._prepare_system(*args, kw['sense'], kw['constraints'], None, 'paired', S, MAX_ITER, TOL, CTOL, None)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['two', 'eight', 'sixteen'])
def test_every_solve_matches_the_host_statement(device_ctx, name):
    for E, S in ((200, 32), (50, 64)):
        p = prepared(name, E, S)
        dev = device_ctx.system_optimize(p)
        lo, hi = p['lo'], p['hi']
        assert np.all(dev[0] >= lo) and np.all(dev[0] <= hi)
        check_against_host(dev, opt.solve_system_host(p), f"{name} {E} x {S}")
        if S == 32:
            again = device_ctx.system_optimize(p)                      # bit for bit
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(dev, again))


def numpy_value_and_gradient(model, row, x_true):
    """A model's value and true-scale gradient at one point from betas / mtx / phis by numpy's polynomial class."""
    betas, mtx = model['betas'][row], model['mtx']
    low = np.array([mm[0] for mm in model['minmax']], dtype=float)
    span = np.array([mm[1] for mm in model['minmax']], dtype=float) - low
    xn = (x_true - low) / span
    basis = lambda order, x, d: np.polynomial.Polynomial(PHIS[order - 1]).deriv(d)(x) if d else \
        np.polynomial.Polynomial(PHIS[order - 1])(x)
    value, grad = betas[0], np.zeros(len(low))
    for t, orders in enumerate(mtx):
        used = [(j, int(o)) for j, o in enumerate(orders) if o]
        value += betas[t + 1] * np.prod([basis(o, xn[j], 0) for j, o in used])
        for j, o in used:
            rest = np.prod([basis(oo, xn[jj], 0) for jj, oo in used if jj != j])
            grad[j] += betas[t + 1] * rest * basis(o, xn[j], 1) / span[j]
    return value, grad


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['two', 'eight', 'sixteen'])
def test_converged_points_satisfy_the_optimality_conditions(device_ctx, name):
    """Not through the host statement: residuals, multiplier signs and the projected gradient of the Lagrangian with the
    RETURNED multipliers, recomputed from betas / mtx / phis."""
    E, S = 24, 32
    args, kw = system(name, E)
    models, xvars, yvars, objective = args
    res = opt.optimize_system(*args, starts=S, max_iter=MAX_ITER, tol=TOL, ctol=CTOL, ReturnAll=True, device=device_ctx, **kw)
    p = prepared(name, E, S)
    index = {v: i for i, v in enumerate(res.variables)}
    sign = -1.0 if kw['sense'] == 'max' else 1.0
    picked = np.argwhere(res.status_all == opt.CONVERGED)[::5][:120]
    assert len(picked) >= 20
    worst_pg = worst_res = 0.0
    for e, s in picked:
        x = res.x_all[e, s]
        vals, grads = {}, {}
        for k, model in enumerate(models):
            cols = [index[v] for v in xvars[k]]
            vals[yvars[k]], g = numpy_value_and_gradient(model, e, x[cols])
            grads[yvars[k]] = np.zeros(len(x))
            grads[yvars[k]][cols] = g
            assert abs(vals[yvars[k]] - res.y_all[e, s, k]) <= 1e-9 * max(1.0, abs(vals[yvars[k]]))
        if objective in index:
            lagr = np.zeros(len(x))
            lagr[index[objective]] = sign
        else:
            lagr = sign * grads[objective]
        for i, c in enumerate(p['cons']):
            mu = res.multipliers_all[e, s, i]
            out = yvars[c['model']]
            if c['var'] >= 0:                                          # the tie: output - variable = 0
                residual = abs(vals[out] - x[c['var']]) / c['scale']
                lagr = lagr + mu * grads[out]
                lagr[c['var']] -= mu
            else:
                lo_c, hi_c = c['lo'], c['hi']
                residual = max(vals[out] - hi_c, lo_c - vals[out], 0.0) / c['scale']
                lagr = lagr + mu * grads[out]
                if lo_c < hi_c:                                        # an inequality: the sign names the side, 0 when inactive
                    if mu > 0.0:
                        assert hi_c < np.inf and abs(vals[out] - hi_c) <= 10 * CTOL * c['scale']
                    if mu < 0.0:
                        assert lo_c > -np.inf and abs(vals[out] - lo_c) <= 10 * CTOL * c['scale']
                    if lo_c + 1e-3 * c['scale'] < vals[out] < hi_c - 1e-3 * c['scale']:
                        assert mu == 0.0
            worst_res = max(worst_res, residual)
        z = (x - p['vmin']) / p['vspan']
        gz = lagr * p['vspan']                                         # the gradient in the common normalised coordinates
        pg = float(np.max(np.abs(np.clip(z - gz, p['lo'], p['hi']) - z)))
        worst_pg = max(worst_pg, pg)
    print(f"\n{name}: {len(picked)} converged points, largest scaled residual {worst_res:.2e}, largest projected gradient "
          f"of the Lagrangian {worst_pg:.2e}")
    assert worst_res <= CTOL * (1 + 1e-6) + 1e-12 and worst_pg <= 10 * TOL


@pytest.mark.gpu
def test_one_model_without_constraints_is_optimize_on_the_device(device_ctx):
    rng = np.random.default_rng(41)
    mtx, mean = random_model(rng, 8, 3, 24)
    minmax = [[-2.0 + j, 3.0 + 2 * j] for j in range(8)]
    model = with_draws(mtx, mean, minmax, 100, 42)
    for S, sense in ((32, 'max'), (64, 'min')):
        one = opt.optimize(model['betas'], mtx, PHIS, minmax, sense=sense, starts=S, max_iter=60, tol=1e-10,
                           ReturnAll=True, device=device_ctx)
        both = opt.optimize_system([model], [[f'x{j}' for j in range(8)]], ['y'], 'y', sense=sense, starts=S, max_iter=60,
                                   tol=1e-10, ReturnAll=True, device=device_ctx)
        assert np.array_equal(both.status_all, one.status_all) and np.array_equal(both.status, one.status)
        assert np.max(np.abs(both.x_all - one.x_all)) <= 1e-10 and np.max(np.abs(both.f_all - one.f_all)) <= 1e-10
        assert np.max(np.abs(both.x_array - one.x)) <= 1e-10 and np.array_equal(both.f_bounds, one.f_bounds)
        assert np.all(both.violation_all == 0.0) and both.multipliers_all.shape == (100, S, 0)


@pytest.mark.gpu
def test_native_refusals_launch_nothing(device_ctx):
    p = prepared('eight', 3, 8)
    device_ctx.timing_enable(True)
    good = device_ctx.system_optimize(p)
    assert np.all(np.isin(good[6], (opt.CONVERGED, opt.STALLED, opt.INFEASIBLE)))
    launched = device_ctx.timing_get(_capi.K_OPTIMIZE_SYSTEM)['launches']
    assert launched >= 1

    def refused(text, **changes):
        with pytest.raises(_capi.FoklNativeError) as err:
            device_ctx.system_optimize(dict(p, **changes))
        assert err.value.code == -2 and text in str(err.value), str(err.value)
        report = device_ctx.system_optimize_report()
        assert report.pop('instance') == 'none' and set(report.values()) == {0}

    refused('sign must be', sign=0.5)
    refused('sign must be', ctol=-1.0)
    refused('the objective is one model', obj_model=-1)
    refused('the objective is one model', obj_model=2)
    refused('inverted box', lo=np.where(np.arange(8) == 2, 0.7, p['lo']), hi=np.where(np.arange(8) == 2, 0.6, p['hi']))
    refused('inverted box', lo=np.where(np.arange(8) == 0, np.nan, p['lo']))
    beyond = [m.copy() for m in p['mtxs']]
    beyond[1][0, 0] = 21
    refused('outside the coefficient table', mtxs=beyond)
    refused('reads a variable outside the system, or twice', var_of=[p['var_of'][0], np.array([3, 3, 5, 6, 7], dtype=np.int32)])
    refused('reads a variable outside the system, or twice', var_of=[p['var_of'][0], np.array([3, 4, 5, 6, 8], dtype=np.int32)])
    tie = dict(p['cons'][0], var=0, lo=0.0, hi=0.0)
    refused('ordered by model', cons=[dict(p['cons'][0]), dict(p['cons'][0], model=0)])
    refused('ordered by model', cons=[tie, dict(p['cons'][0])])
    refused('positive scale', cons=[dict(p['cons'][0], scale=0.0)])
    refused('needs lo <= hi', cons=[dict(p['cons'][0], lo=1.0, hi=0.0)])
    refused('a tie is the equality', cons=[dict(p['cons'][0], var=0)])
    refused('one call runs at most', coef=np.ones((1 << 14, p['coef'].shape[1])), starts=opt.start_points(65, p['lo'], p['hi']))
    # 16 variables x 3 orders: 3 x 48 + 136 + 48 + 2 values per solve, the LDS of a wavefront holds 288
    many = np.zeros((48, 16), dtype=np.int32)
    for j in range(16):
        for order in range(3):
            many[3 * j + order, j] = order + 1
    big = dict(p, n=16, K=1, mtxs=[many], var_of=[np.arange(16, dtype=np.int32)], shift=[np.zeros(16)], slope=[np.ones(16)],
               coef=np.ones((1, 49)), lo=np.zeros(16), hi=np.ones(16), starts=np.zeros((1, 16)), obj_model=0, cons=[],
               vmin=np.zeros(16), vspan=np.ones(16))
    with pytest.raises(_capi.FoklNativeError) as err:
        device_ctx.system_optimize(big)
    assert err.value.code == -2 and '330 values per solve, a wavefront\'s LDS holds 288' in str(err.value)
    with pytest.raises(_capi.FoklNativeError) as err:
        device_ctx.system_optimize(dict(big, n=17, mtxs=[np.ones((1, 17), dtype=np.int32)], var_of=[np.arange(17, dtype=np.int32)],
                                        shift=[np.zeros(17)], slope=[np.ones(17)], coef=np.ones((1, 2)), lo=np.zeros(17),
                                        hi=np.ones(17), starts=np.zeros((1, 17)), vmin=np.zeros(17), vspan=np.ones(17)))
    assert err.value.code == -2 and 'at most 16' in str(err.value)
    assert device_ctx.timing_get(_capi.K_OPTIMIZE_SYSTEM)['launches'] == launched
    # the context is as it was: the same call, the same bits; and it still optimises a single model
    again = device_ctx.system_optimize(p)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(good, again))
    one = opt.optimize(p['coef'][:, :p['mtxs'][0].shape[0] + 1], p['mtxs'][0], PHIS, [[0.0, 1.0 + j] for j in range(6)],
                       starts=8, device=device_ctx)
    assert np.all(np.isin(one.status, (opt.CONVERGED, opt.STALLED)))
    # the launches are sliced: no launch is asked for more than ITERATION_CAP solve-iterations
    device_ctx.timing_reset()
    sliced = device_ctx.system_optimize(dict(prepared('two', 40, 64), max_iter=4096))
    per_launch = max(64, opt.ITERATION_CAP // 4096 // 64 * 64)
    assert device_ctx.timing_get(_capi.K_OPTIMIZE_SYSTEM)['launches'] == -(-40 * 64 // per_launch) == 3
    device_ctx.timing_enable(False)
    whole = device_ctx.system_optimize(prepared('two', 40, 64))       # one launch
    ended = whole[5] < MAX_ITER
    assert ended.mean() > 0.9 and all(np.array_equal(a[ended], b[ended]) for a, b in zip(sliced, whole))


def janaf_co2():
    """T (K), Cp (J / mol K) and the Gibbs energy of formation (kJ / mol) of CO2 from the NIST-JANAF table (the rows
    above 0 K)."""
    rows = [line.split('\t') for line in open(os.path.join(ROOT, 'tests', 'golden', 'janaf_co2_C-095.txt')).read().splitlines()[3:]]
    table = np.array([[float(row[0]), float(row[1]), float(row[6])] for row in rows if len(row) >= 7])
    return table[:, 0], table[:, 1], table[:, 2]


@pytest.mark.gpu
def test_from_two_fits_to_the_constrained_optimum(device_ctx):
    """Cp = f(T) and G = f(T, Cp) fitted on the device from the JANAF table; Cp is the intermediate.  G minimised under a
    ceiling on Cp, then the lowest T found for a pinned G: the device equals the host statement, the point is inside
    every training range, and `evaluate` reproduces the returned outputs."""
    from fokl_gpy_amd import FoKLRoutines
    T, Cp, G = janaf_co2()
    assert T.shape == (61,) and T[0] == 100.0 and T[-1] == 6000.0

    def fit(inputs, data, seed):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = FoKLRoutines.FoKL(kernel=BERN, burnin=60, draws=60, tolerance=2, UserWarnings=False, ConsoleOutput=False)
            np.random.seed(seed)
            model.fit(inputs, data, clean=True)
        return model

    model_cp, model_g = fit(T, Cp, 5), fit([T, Cp], G, 6)
    models, xvars, yvars = [model_cp, model_g], [['T'], ['T', 'Cp']], ['Cp', 'G']
    # G falls to its minimum near 1800 K, where Cp is 59.7: under a ceiling of 58 the ceiling binds (the table's largest
    # G lies at its ends, where a draw of Cp = f(T) may leave the range G = f(T, Cp) was trained on: no place for a test);
    # G = -395 is reached twice, the colder point is asked for.  The table has 61 rows and the posterior is wide: in
    # part of the draws Cp = f(T) leaves the range G = f(T, Cp) was trained on and the pinned value cannot be met;
    # those draws must come back as infeasible, from the device as from the host statement
    ceiling, pinned = 58.0, -395.0
    cases = [('G', dict(sense='min', constraints={'Cp': (None, ceiling)})),
             ('T', dict(sense='min', constraints={'G': (pinned, pinned)}))]
    E = np.asarray(model_cp.betas).shape[0]
    size_g = float(np.mean(np.sum(np.abs(np.asarray(model_g.betas)), axis=1)))
    for objective, kw in cases:
        kw.update(starts=16, max_iter=MAX_ITER)
        dev = opt.optimize_system(models, xvars, yvars, objective, device=device_ctx, **kw)
        host = opt.optimize_system_host(models, xvars, yvars, objective, **kw)
        done = np.isin(dev.status, (opt.CONVERGED, opt.STALLED))
        print(f"\n{objective}: device statuses {np.bincount(dev.status, minlength=5).tolist()}, host "
              f"{np.bincount(host.status, minlength=5).tolist()}, T {np.percentile(dev.x['T'][done], [5, 50, 95]).round(1).tolist()}")
        assert dev.f.shape == (E,) and done.mean() >= 0.4 and np.mean(dev.status == host.status) >= 0.95
        assert np.all(dev.violation[dev.status == opt.INFEASIBLE] > 1e-8)
        both = (dev.status == opt.CONVERGED) & (host.status == opt.CONVERGED)
        assert np.max(np.abs(dev.f - host.f)[both]) <= 1e-7 * np.max(np.abs(host.f[both]))
        assert np.max((np.abs(dev.x_array - host.x_array) / [T[-1] - T[0], np.ptp(Cp)])[both]) <= 1e-6
        assert np.all(dev.x['T'] >= T.min()) and np.all(dev.x['T'] <= T.max())
        assert np.all(dev.x['Cp'] >= Cp.min()) and np.all(dev.x['Cp'] <= Cp.max())
        assert np.all(dev.violation[done] <= 1e-8) and dev.f_bounds[0] <= dev.f_bounds[1]
        if objective == 'G':
            assert np.all(dev.y['Cp'][done] <= ceiling + 1e-5) and np.all(dev.multipliers['Cp'][done] >= 0.0)
        else:
            assert np.max(np.abs(dev.y['G'][done] - pinned)) <= 1.01e-8 * size_g and np.array_equal(dev.f, dev.x['T'])
        # the mean models: evaluate() at the returned inputs reproduces the returned outputs
        mean = opt.optimize_system(models, xvars, yvars, objective, draws='mean', device=device_ctx, **kw)
        assert mean.status in (opt.CONVERGED, opt.STALLED) and isinstance(mean.f, float)
        for model, names, out in ((model_cp, ['T'], 'Cp'), (model_g, ['T', 'Cp'], 'G')):
            low, high = np.array(model.minmax, dtype=float).T
            point = np.array([mean.x[name] for name in names])
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                value = np.ravel(model.evaluate(np.tile((point - low) / (high - low), (3, 1))))[0]
            assert abs(value - mean.y[out]) <= 1e-9 * max(1.0, abs(mean.y[out])), (out, value, mean.y[out])
        assert abs(mean.y['Cp'] - mean.x['Cp']) <= 1e-8 * 2 * np.sum(np.abs(np.mean(model_cp.betas, axis=0)))
        if objective == 'G':
            assert 1000.0 < mean.x['T'] < 1800.0 and abs(mean.y['Cp'] - ceiling) <= 1e-5 and mean.multipliers['Cp'] > 0.0
        else:
            assert 150.0 < mean.x['T'] < 1000.0 and abs(mean.y['G'] - pinned) <= 1.01e-8 * size_g

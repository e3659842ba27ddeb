"""infer.infer_inputs_host, the statement of the ensemble sampler over unknown inputs (fokl_gpy_amd/infer.py): its random
numbers, the split of a model into known and unknown factors, the posterior it samples against exact references, its
bookkeeping and its refusals.  No device (the cross-compiled library only for fokl_infer_rng)."""
import math

import numpy as np
import pytest

from fokl_gpy_amd import FoKLRoutines, _capi, getKernels, infer
from fokl_gpy_amd.embedded import basis_matrix

KERNEL = 'Bernoulli Polynomials'
PHIS = getKernels.bernoulli()
E = 16                          # ensembles per statistical case, keyed independently: their spread is the standard error
SIGMAS = 4.0


# ---------------------------------------------------------------------------------------------------------
# random numbers
# ---------------------------------------------------------------------------------------------------------

def test_rng_uniforms_lie_in_the_unit_interval_and_repeat():
    for purpose in (_capi.INFER_U1, _capi.INFER_U2, _capi.INFER_U3):
        u = _capi.infer_rng(11, 3, 7, purpose, 4096)
        assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.03
        assert np.array_equal(u, _capi.infer_rng(11, 3, 7, purpose, 4096))
        assert np.array_equal(u[:64], _capi.infer_rng(11, 3, 7, purpose, 64))
    n = _capi.infer_rng(11, 3, 7, _capi.INFER_JITTER, 4096)
    assert abs(n.mean()) < 0.08 and abs(n.std() - 1.0) < 0.05
    streams = [_capi.infer_rng(*key, 0, 8) for key in ((11, 3, 7), (12, 3, 7), (11, 4, 7), (11, 3, 8))]
    streams.append(_capi.infer_rng(11, 3, 7, 1, 8))
    for a in range(len(streams)):
        for b in range(a):
            assert not np.any(streams[a] == streams[b])


def test_rng_streams_are_apart_from_the_embedded_ones():
    """The fourth counter word: the same (seed, chain, draw, purpose, index) gives other numbers than fokl_embedded_rng."""
    for purpose in (0, 1, 2, 3):
        assert not np.any(_capi.infer_rng(5, 2, 9, purpose, 64) == _capi.embedded_rng(5, 2, 9, purpose, 64))
    with pytest.raises(_capi.FoklNativeError):
        _capi.infer_rng(5, 2, 9, 4, 1)
    with pytest.raises(_capi.FoklNativeError):
        _capi.infer_rng(5, 2, 9, -1, 1)


# ---------------------------------------------------------------------------------------------------------
# _prepare: known x unknown
# ---------------------------------------------------------------------------------------------------------

MTX6 = np.array([[1, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0], [0, 0, 0, 3, 0, 0], [1, 1, 0, 0, 0, 0], [0, 2, 0, 0, 1, 0],
                 [1, 0, 2, 0, 0, 3], [2, 1, 0, 1, 3, 0], [0, 0, 1, 0, 2, 0], [0, 0, 3, 0, 0, 0], [3, 0, 0, 2, 0, 1],
                 [0, 1, 0, 1, 0, 0]])                                  # one- to four-way terms; terms 7, 8: no unknown factor
MINMAX6 = [[0.0, 2.0], [-1.0, 1.0], [0.0, 1.0], [10.0, 20.0], [0.0, 1.0], [-3.0, 0.0]]
UNKNOWN6 = [0, 1, 3, 5]                                                # knowns: inputs 2 and 4


def test_prepare_splits_every_term_into_known_and_unknown_factors():
    rng = np.random.default_rng(3)
    betas = rng.standard_normal((3, MTX6.shape[0] + 1))
    known = rng.random((7, 2))
    p = infer._prepare(betas, np.ones(3), MTX6, PHIS, MINMAX6, KERNEL, ['x1', 1, 'x4', 5], known, rng.standard_normal(7))
    assert p['cols'] == UNKNOWN6 and p['P'].shape == (7, MTX6.shape[0] + 1) and np.all(p['P'][:, 0] == 1.0)
    from fokl_gpy_amd.optimize import TermTable
    tt = TermTable(p['mtx_u'])
    theta = rng.random((5, 4))
    U = np.concatenate([np.ones((1, 5)), infer.unknown_products(tt, p['table'], theta)])      # [T + 1, points]
    for k in range(7):
        full = np.zeros((5, 6))
        full[:, UNKNOWN6] = theta
        full[:, [2, 4]] = known[k]
        X = basis_matrix(full, MTX6, PHIS, KERNEL)
        for e in range(3):
            split = (betas[e][:, None] * p['P'][k][:, None] * U).sum(axis=0)
            scale = (np.abs(betas[e]) * np.abs(X)).sum(axis=1)
            assert np.max(np.abs(split - X @ betas[e]) / scale) <= 1e-13


def test_prepare_scales_prior_bounds_and_known_inputs():
    betas = np.ones((2, MTX6.shape[0] + 1))
    known_true = np.array([[0.25, 0.5], [1.0, 0.0]])
    p = infer._prepare(betas, None, MTX6, PHIS, MINMAX6, KERNEL, UNKNOWN6, known_true, [0.0, 1.0], clean=True, noise=0.5,
                       prior={3: (12.0, 2.0), 'x1': (1.0, 4.0)}, bounds={'x6': (-2.0, -1.0)})
    assert np.allclose(p['h'], 0.5 / 0.25) and p['draw_ids'].tolist() == [0, 1]
    assert np.allclose(p['prior_mean'], [0.5, 0.0, 0.2, 0.0]) and np.allclose(p['prior_prec'], [0.25, 0.0, 25.0, 0.0])
    assert np.allclose(p['lo'], [0, 0, 0, 1 / 3]) and np.allclose(p['hi'], [1, 1, 1, 2 / 3])
    assert np.all((p['starts'] > p['lo']) & (p['starts'] < p['hi'])) and p['starts'].shape == (64, 4)
    q = infer._prepare(betas, None, MTX6, PHIS, MINMAX6, KERNEL, UNKNOWN6, known_true, [0.0, 1.0], noise=0.5)
    assert np.array_equal(q['P'], p['P'])                              # inputs 2 and 4 span [0, 1]: true scale = normalised
    one = infer._prepare(betas, [1.0, 3.0], MTX6, PHIS, MINMAX6, KERNEL, UNKNOWN6, known_true, [0.0, 1.0], objective='mean')
    assert one['E'] == 1 and np.allclose(one['sigsqd'], 2.0)
    last = infer._prepare(np.arange(3)[:, None] * betas[:1], [1.0, 2.0, 3.0], MTX6, PHIS, MINMAX6, KERNEL, UNKNOWN6,
                          known_true, [0.0, 1.0], posterior=[2, 0])
    assert last['draw_ids'].tolist() == [2, 0] and np.allclose(last['sigsqd'], [3.0, 1.0])


def test_prepare_refusals():
    betas = np.ones((2, MTX6.shape[0] + 1))
    known = np.full((2, 2), 0.5)
    args = lambda **kw: infer._prepare(*[kw.pop(k, v) for k, v in (('betas', betas), ('sigsqd', np.ones(2)), ('mtx', MTX6),
                                                                   ('phis', PHIS), ('minmax', MINMAX6), ('kernel', KERNEL),
                                                                   ('unknown', UNKNOWN6), ('known', known),
                                                                   ('data', [0.0, 1.0]))], **kw)
    args()
    with pytest.raises(ValueError, match="resample.*noise="):
        args(sigsqd=None)
    with pytest.raises(ValueError, match="Cubic Splines"):
        args(kernel='Cubic Splines')
    for bad in (dict(unknown=[]), dict(unknown=[0, 0]), dict(unknown=['nope']), dict(unknown=[6]), dict(known=None),
                dict(known=np.full((2, 2), 1.5)), dict(known=np.full((3, 2), 0.5)), dict(data=[0.0, np.nan]),
                dict(bounds={'x1': (1.0, 1.0)}), dict(bounds={'x1': (-1.0, 1.0)}), dict(bounds={'x3': (0.1, 0.2)}),
                dict(prior={'x1': (0.0, 0.0)}), dict(prior={'x5': (0.0, 1.0)}), dict(starts=np.zeros((64, 4))),
                dict(starts=np.full((63, 4), 0.5)), dict(thin=0), dict(draws=0), dict(burnin=-1), dict(jump_every=-1),
                dict(noise=0.0), dict(keep='y'), dict(objective='median'), dict(posterior=5), dict(sigsqd=[1.0, -1.0]),
                dict(betas=np.array([[1.0] * 12, [np.nan] * 12]))):
        with pytest.raises(ValueError):
            args(**bad)
    wide = np.zeros((48, 16), dtype=int)                              # 16 unknowns x 5 orders: 80 factors, 304 values
    for t in range(48):
        wide[t, t % 16] = 1 + t // 16
        wide[t, (t + 1) % 16] = 3 + t // 16
    with pytest.raises(ValueError, match="LDS"):
        infer._prepare(np.ones((1, 49)), [1.0], wide, PHIS, [[0, 1]] * 16, KERNEL, list(range(16)), None, [0.0])


# ---------------------------------------------------------------------------------------------------------
# the posterior against exact references (E = 16 ensembles; 4 standard errors, the standard error capped)
# ---------------------------------------------------------------------------------------------------------

def per_ensemble(res, stat):
    """stat(rows [n, d]) of every ensemble's own rows -> [E, ...]."""
    rows = res.x.reshape(res.draws, -1, res.x.shape[1])
    return np.array([stat(r) for r in rows])


def check(estimates, exact, caps):
    """The mean over the ensembles against ``exact`` within SIGMAS standard errors, the standard error (the spread of the
    independently keyed ensembles) below its cap.  Returns the standard errors (the cap-measuring script prints them)."""
    estimates, exact, caps = np.atleast_2d(np.asarray(estimates).T).T, np.atleast_1d(exact), np.atleast_1d(caps)
    se = estimates.std(axis=0, ddof=1) / math.sqrt(estimates.shape[0])
    print('estimate', estimates.mean(axis=0), 'exact', exact, 'se', se, 'caps', caps)
    assert np.all(se <= caps), (se, caps)
    assert np.all(np.abs(estimates.mean(axis=0) - exact) <= SIGMAS * se), (estimates.mean(axis=0), exact, se)
    return se


def truncated_normal(mu, sd, lo=0.0, hi=1.0):
    """Mean and standard deviation of N(mu, sd) cut to [lo, hi]."""
    a, b = (lo - mu) / sd, (hi - mu) / sd
    pdf = lambda t: math.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
    cdf = lambda t: 0.5 * (1.0 + math.erf(t / math.sqrt(2.0)))
    Z = cdf(b) - cdf(a)
    mean = mu + sd * (pdf(a) - pdf(b)) / Z
    var = sd * sd * (1.0 + (a * pdf(a) - b * pdf(b)) / Z - ((pdf(a) - pdf(b)) / Z) ** 2)
    return mean, math.sqrt(var)


def linear_case(mode, seed=0):
    """d = 1, f = phi_1(x) = c0 + c1 x, one observation with noise 0.05 c1: the posterior is N(mode, 0.05) cut to the box."""
    c0, c1 = float(PHIS[0][0]), float(PHIS[0][1])
    res = infer.infer_inputs_host(np.tile([0.0, 1.0], (E, 1)), None, np.array([[1]]), PHIS, [[0.0, 1.0]], KERNEL, [0], None,
                                  [c0 + c1 * mode], noise=0.05 * c1, burnin=200, draws=600, thin=1, seed=seed)
    est = np.stack([per_ensemble(res, lambda r: r[:, 0].mean()), per_ensemble(res, lambda r: r[:, 0].std())], axis=1)
    return est, np.array(truncated_normal(mode, 0.05))


TWO_ROOT_BETAS = np.array([0.0, 0.2, 1.0, 1.0])                        # f = 0.2 phi_1 + phi_2 + phi_3: a valley inside the box
TWO_ROOT_MTX = np.array([[1], [2], [3]])


def two_root_case(seed=0, jump_every=8):
    """d = 1, two roots of unequal slope: the mass left of the hump between them against a 1-D quadrature."""
    y, sd = -0.02, 0.01                                                # roots near 0.15 (slope -0.37) and 0.71 (slope 0.6)
    grid = (np.arange(200000) + 0.5) / 200000
    f = basis_matrix(grid[:, None], TWO_ROOT_MTX, PHIS, KERNEL) @ TWO_ROOT_BETAS
    dens = np.exp(-0.5 * ((y - f) / sd) ** 2)
    cut = grid[np.argmin(f)]                                           # the bottom of the valley between the roots
    exact = dens[grid < cut].sum() / dens.sum()
    res = infer.infer_inputs_host(np.tile(TWO_ROOT_BETAS, (E, 1)), None, TWO_ROOT_MTX, PHIS, [[0.0, 1.0]], KERNEL, [0], None,
                                  [y], noise=sd, burnin=300, draws=600, thin=1, seed=seed, jump_every=jump_every)
    return per_ensemble(res, lambda r: np.mean(r[:, 0] < cut)), exact


CORR_MTX = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 1], [0, 2, 1]])
CORR_BETAS = np.array([0.1, 1.0, 0.8, 1.5, -0.7])


def correlated_case(seed=0):
    """d = 2 of m = 3, two observations at different known x3: means and covariance against a 2-D grid quadrature."""
    truth, x3, sd = np.array([0.45, 0.55]), np.array([0.15, 0.9]), 0.04
    at = lambda a, b, c: basis_matrix(np.stack([a, b, np.full_like(a, c)], axis=1), CORR_MTX, PHIS, KERNEL) @ CORR_BETAS
    y = np.array([at(truth[:1], truth[1:], c)[0] for c in x3])
    g = (np.arange(600) + 0.5) / 600
    A, B = (v.ravel() for v in np.meshgrid(g, g, indexing='ij'))
    logp = sum(-0.5 * ((y[k] - at(A, B, x3[k])) / sd) ** 2 for k in range(2))
    wgt = np.exp(logp - logp.max())
    wgt /= wgt.sum()
    ma, mb = (wgt * A).sum(), (wgt * B).sum()
    exact = np.array([ma, mb, (wgt * (A - ma) ** 2).sum(), (wgt * (B - mb) ** 2).sum(), (wgt * (A - ma) * (B - mb)).sum()])
    res = infer.infer_inputs_host(np.tile(CORR_BETAS, (E, 1)), None, CORR_MTX, PHIS, [[0.0, 1.0]] * 3, KERNEL, ['x1', 'x2'],
                                  x3[:, None], y, noise=sd, burnin=300, draws=600, thin=1, seed=seed)

    def stat(r):
        c = np.cov(r, rowvar=False, bias=True)
        return np.array([r[:, 0].mean(), r[:, 1].mean(), c[0, 0], c[1, 1], c[0, 1]])
    return per_ensemble(res, stat), exact


# The caps: twice the largest standard error seen over seeds 0 .. 7 of the host statement (measured on the CPU with the
# case functions above; the largest values seen are quoted in the docstrings).

def test_linear_model_mid_box_gives_the_normal_posterior():
    """Largest standard errors over seeds 0..7: mean 0.00036, sd 0.00016."""
    check(*linear_case(0.6), caps=[2 * 0.00036, 2 * 0.00016])


def test_linear_model_with_the_mode_next_to_a_wall_gives_the_truncated_normal():
    """The mode 0.3 sd below the upper wall.  Largest standard errors over seeds 0..7: mean 0.00025, sd 0.00015."""
    check(*linear_case(1.0 - 0.3 * 0.05), caps=[2 * 0.00025, 2 * 0.00015])


def test_two_roots_of_unequal_slope_get_their_masses_through_the_jump_move():
    """Largest standard error of the left-mode mass over seeds 0..7: 0.0046 (exact mass 0.6386; without the
    jump move the statement gives 0.479: a walker never changes mode)."""
    check(*two_root_case(), caps=2 * 0.0046)


def test_correlated_posterior_in_two_dimensions():
    """Largest standard errors over seeds 0..7: means 0.00033, 0.00056; variances 1.7e-5, 3.3e-5; covariance 2.1e-5."""
    check(*correlated_case(), caps=[2 * 0.00033, 2 * 0.00056, 2 * 1.7e-5, 2 * 3.3e-5, 2 * 2.1e-5])


# ---------------------------------------------------------------------------------------------------------
# bookkeeping
# ---------------------------------------------------------------------------------------------------------

def small_problem(Edraws=5, seed=2):
    rng = np.random.default_rng(seed)
    betas = CORR_BETAS * (1.0 + 0.05 * rng.standard_normal((Edraws, CORR_BETAS.shape[0])))
    args = (betas, 0.002 * (1.0 + rng.random(Edraws)), CORR_MTX, PHIS, [[0.0, 2.0], [1.0, 3.0], [0.0, 1.0]], KERNEL,
            ['x1', 'x2'], np.array([[0.2], [0.8], [0.5]]), [0.1, 0.3, 0.2])
    return args


def test_thinned_rows_are_the_subset_rows():
    args = small_problem()
    every = infer.infer_inputs_host(*args, burnin=5, draws=20, thin=1, jump_every=3, seed=4)
    third = infer.infer_inputs_host(*args, burnin=5, draws=20, thin=3, jump_every=3, seed=4)
    x1, x3 = every.x.reshape(5, 20, 64, 2), third.x.reshape(5, 7, 64, 2)
    assert np.array_equal(x3, x1[:, ::3]) and np.array_equal(third.lp.reshape(5, 7, 64), every.lp.reshape(5, 20, 64)[:, ::3])
    assert np.array_equal(third.accept, every.accept) and np.array_equal(third.evals, every.evals)
    assert np.array_equal(third.draw.reshape(5, -1)[:, 0], np.arange(5)) and every.quantiles.shape == (2, 2)
    assert np.all(every.evals <= 64 * (1 + 25)) and np.all(every.evals > 64)
    assert np.all((every.x > [0.0, 1.0]) & (every.x < [2.0, 3.0]))


def test_an_ensemble_alone_is_the_ensemble_among_many():
    args = small_problem()
    many = infer.infer_inputs_host(*args, burnin=4, draws=12, thin=2, jump_every=2, seed=9)
    alone = infer.infer_inputs_host(*args, burnin=4, draws=12, thin=2, jump_every=2, seed=9, posterior=[3])
    assert np.array_equal(alone.x, many.x.reshape(5, -1, 2)[3]) and np.array_equal(alone.lp, many.lp.reshape(5, -1)[3])
    assert np.array_equal(alone.accept[0], many.accept[3]) and alone.draw_ids.tolist() == [3] and np.all(alone.draw == 3)
    other = infer.infer_inputs_host(*args, burnin=4, draws=12, thin=2, jump_every=2, seed=10, posterior=[3])
    assert not np.array_equal(other.x, alone.x)


def test_sums_without_rows_are_the_sums_of_the_rows():
    args = small_problem()
    p = infer._prepare(*args, burnin=3, draws=9, thin=1, jump_every=4, seed=1)
    run = lambda rows: infer.sample_host(p['mtx_u'], p['betas'], p['h'], p['table'], p['lo'], p['hi'], p['prior_mean'],
                                         p['prior_prec'], p['y'], p['P'], p['starts'], 3, 9, 1, 4, 1, rows=rows)
    x, lp, sums, accepted, evals = run(True)
    none = run(False)
    assert none[0] is None and none[1] is None and np.array_equal(none[2], sums) and np.array_equal(none[3], accepted)
    c = x - 0.5 * (p['lo'] + p['hi'])                                  # [E, 9, 64, d]
    for seg, part in ((0, c[:, :4]), (1, c[:, 4:])):
        s1, s2 = np.zeros_like(c[:, 0]), np.zeros_like(c[:, 0])
        for r in range(part.shape[1]):
            s1, s2 = s1 + part[:, r], s2 + part[:, r] * part[:, r]
        assert np.array_equal(sums[:, :, seg, 0], s1) and np.array_equal(sums[:, :, seg, 1], s2)
    res = infer.infer_inputs_host(*args, burnin=3, draws=9, thin=1, jump_every=4, seed=1, keep=None)
    full = infer.infer_inputs_host(*args, burnin=3, draws=9, thin=1, jump_every=4, seed=1)
    assert res.x is None and res.cov is None and np.allclose(res.mean, full.mean, rtol=1e-12)
    assert np.array_equal(res.rhat, full.rhat) and res.rhat.shape == (5, 2)


def test_the_statement_keeps_its_flags_when_the_terms_are_summed_in_reverse():
    """What the GPU test's flag rule rests on: a reordered term sum (a few ulp of lp) flips no acceptance of the chains it
    compares, on the reference alone."""
    args = small_problem()
    p = infer._prepare(*args, burnin=0, draws=40, thin=1, jump_every=2, seed=6)
    run = lambda rev: infer.sample_host(p['mtx_u'], p['betas'], p['h'], p['table'], p['lo'], p['hi'], p['prior_mean'],
                                        p['prior_prec'], p['y'], p['P'], p['starts'], 0, 40, 1, 2, 6, reverse_terms=rev,
                                        flags=True)
    a, b = run(False), run(True)
    assert not np.array_equal(a[1], b[1])                              # the sums do differ in their last bits
    same = [e for e in range(5) if np.array_equal(a[5][e], b[5][e])]
    assert len(same) >= 4
    assert np.max(np.abs(a[6][same] - b[6][same])) <= 1e-9


def test_the_method_refuses_a_fit_without_sigma_and_double_posteriors():
    model = FoKLRoutines.FoKL(kernel=KERNEL, UserWarnings=False, ConsoleOutput=False)
    model.betas, model.mtx, model.minmax = np.tile(CORR_BETAS, (3, 1)), CORR_MTX, [[0.0, 1.0]] * 3
    with pytest.raises(ValueError, match="resample.*noise="):
        model.infer_inputs(unknown=['x1', 'x2'], known=[[0.2], [0.8]], data=[0.1, 0.3])
    with pytest.raises(ValueError, match="not both"):
        model.infer_inputs(dict(betas=model.betas, sigsqd=np.ones(3)), betas=model.betas, unknown=[0], data=[0.0])

"""robust.pass_host / step_host / robust_host, the statement of the robust resampler (fokl_gpy_amd/robust.py): its gamma
variate per row, its Gaussian limit against resample_host, the algebra of a step, what Student-t noise does to planted gross
errors, given row weights, its bookkeeping and its refusals.  No device."""
import numpy as np
import pytest
import scipy.stats

from fokl_gpy_amd import FoKLRoutines, _capi, getKernels, resample as R, robust as RB
from test_resample_host import assert_same_distribution

KERNEL = 'Bernoulli Polynomials'
BETA_TRUE = np.array([1.0, 2.0, -1.0, 3.0, 0.5])


def columns(x):
    a, b = x[:, 0] - 0.5, x[:, 1] - 0.5
    return np.stack([np.ones(x.shape[0]), a, b, a * a - 1.0 / 12.0, a * b], axis=1)


def planted(n=2000, bad=100):
    """The issue's case: 100 gross errors of 10-30 sigma among 2 000 rows -> X, y, the planted rows."""
    rng = np.random.default_rng(1)
    X = columns(rng.uniform(size=(n, 2)))
    y = X @ BETA_TRUE + 0.05 * rng.standard_normal(n)
    rows = rng.choice(n, bad, replace=False)
    y[rows] += rng.choice([-1.0, 1.0], bad) * rng.uniform(0.5, 1.5, bad)
    return X, y, rows


def hyper(n, p1, b=0.01, btau=1.0):
    return RB.hyper_of(4.0, b, 4.0, btau, n, p1 - 1)


def run(X, y, nu, seed, w=None, chains=1, burnin=100, draws=400, thin=1, b=0.01, btau=1.0, sig0=None, tau0=None, **kw):
    h = hyper(X.shape[0], X.shape[1], b, btau)
    G0 = RB.pass_host(X, y, w, None, 1.0, np.inf, 0, 0, 0)[0]
    p1 = X.shape[1]
    shift = np.linalg.solve(G0[:p1, :p1] + np.eye(p1) * 5.0 / btau, G0[:p1, p1])
    sig0 = np.full(chains, b / 5.0) if sig0 is None else sig0
    tau0 = np.full(chains, btau / 5.0) if tau0 is None else tau0
    return RB.robust_host(X, y, w, nu, h, shift, sig0, tau0, burnin, draws, thin, seed, **kw)


@pytest.mark.parametrize('shape', [1.0, 2.5, 16.5])
def test_the_lam_variate_is_a_gamma(shape):
    """beta = 0, y = 0: lam_i = g_i / (nu / 2), g_i a standard gamma of shape (nu + 1) / 2."""
    n, nu = 100_000, 2.0 * shape - 1.0
    G, lam, attempts = RB.pass_host(np.ones((n, 1)), np.zeros(n), None, [0.0], 1.0, nu, 23, 1, 5)
    g = lam * (nu / 2.0)
    stat = scipy.stats.kstest(g, scipy.stats.gamma(shape).cdf)
    print(f"shape {shape}: KS distance {stat.statistic:.5f}, p = {stat.pvalue:.3f}; {attempts.mean():.4f} attempts per variate")
    assert stat.pvalue > 1e-3
    assert attempts.min() >= 1 and attempts.mean() < 1.1
    assert G.shape == (2, 2) and abs(G[0, 0] - lam.sum()) <= 1e-12 * lam.sum()
    g2, att2 = RB.row_gamma(shape, 23, 1, 5, n)
    assert np.array_equal(g2, g * 1.0) or np.allclose(g2, g, rtol=1e-15, atol=0.0)
    assert np.array_equal(att2, attempts)


def test_iteration_zero_and_nu_inf_draw_nothing():
    X, y, _ = planted(200, 10)
    for nu, k in ((4.0, 0), (np.inf, 3)):
        G, lam, attempts = RB.pass_host(X, y, None, BETA_TRUE, 0.01, nu, 1, 0, k)
        Z = np.concatenate([X, y[:, None]], axis=1)
        assert np.array_equal(lam, np.ones(200)) and not attempts.any() and np.allclose(G, Z.T @ Z, rtol=1e-14)


def test_gaussian_limit_is_resamples_posterior():
    rng = np.random.default_rng(3)
    n = 400
    inputs = rng.uniform(size=(n, 2))
    mtx = np.array([[1, 0], [0, 1], [2, 0], [1, 1], [0, 2]])
    phis = getKernels.bernoulli()
    from fokl_gpy_amd.embedded import basis_matrix
    X = basis_matrix(inputs, mtx, phis, KERNEL)
    data = X @ np.array([0.5, 1.0, -0.7, 0.3, 0.4, -0.2]) + 0.1 * rng.standard_normal(n)
    args = (mtx, phis, KERNEL, inputs, data, 4.0, 0.8, 4.0, 3.0)
    ours = RB.resample_robust_host(*args, nu=np.inf, chains=4, draws=2000, burnin=200, seed=2)
    theirs = R.resample_host(*args, chains=4, draws=2000, burnin=200, seed=7)
    assert ours.noise == 'gaussian' and np.isinf(ours.nu) and not ours.flagged.any()
    assert np.array_equal(ours.weight_mean, np.ones(n)) and np.array_equal(ours.noise_var, ours.sigsqd)
    assert_same_distribution(ours.betas, 4, theirs.betas, 'betas, nu = inf against resample')
    assert_same_distribution(ours.sigsqd[:, None], 4, theirs.sigsqd[:, None], 'sigsqd, nu = inf against resample')
    assert max(ours.rhat['betas'].max(), ours.rhat['sigsqd'], ours.rhat['tausqd']) < 1.02


def quiet_z(monkeypatch):
    real = _capi.robust_rng

    def rng(seed, chain, iteration, purpose, count, attempt=0, first=0):
        out = real(seed, chain, iteration, purpose, count, attempt, first)
        return np.zeros_like(out) if purpose == _capi.ROB_BETA else out
    monkeypatch.setattr(_capi, 'robust_rng', rng)


def test_a_step_solves_the_weighted_normal_equations(monkeypatch):
    quiet_z(monkeypatch)
    rng = np.random.default_rng(8)
    for p1 in (1, 5, 40, 127):
        n = 4 * p1 + 50
        X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, p1 - 1))], axis=1)
        y = X @ rng.standard_normal(p1) + 0.1 * rng.standard_normal(n)
        w = rng.uniform(0.5, 2.0, n)
        tausqd = 0.7
        G = RB.pass_host(X, y, w, None, 1.0, np.inf, 0, 0, 0)[0]
        beta, sig, tau, flag = RB.step_host(G, 0.01, tausqd, hyper(n, p1), 4, 0, 1)
        expect = np.linalg.solve(X.T @ (X * w[:, None]) + np.eye(p1) / tausqd, X.T @ (w * y))
        assert flag == RB.FLAG_NONE and sig > 0 and tau > 0
        assert np.max(np.abs(beta - expect) / np.maximum(np.abs(expect), np.max(np.abs(expect)) * 1e-3)) < 1e-12, p1


def test_the_residual_sum_from_the_gram():
    """y'y / S about 1e4: the three terms of S cancel four digits and S still holds to 1e-9."""
    rng = np.random.default_rng(9)
    n, p1 = 3000, 12
    X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, p1 - 1))], axis=1)
    truth = rng.standard_normal(p1)
    y = X @ truth + 0.01 * np.linalg.norm(truth) * rng.standard_normal(n)
    w, lam = rng.uniform(0.5, 2.0, n), rng.gamma(2.0, 0.5, n)
    Z = np.concatenate([X, y[:, None]], axis=1)
    G = Z.T @ (Z * (w * lam)[:, None])
    beta = truth + 1e-3 * rng.standard_normal(p1)
    S, q_bb = RB.residual_form(G, beta)
    direct = float(np.sum(w * lam * (y - X @ beta) ** 2))
    print(f"y'y / S = {G[p1, p1] / direct:.3g}; S relative gap {abs(S - direct) / direct:.2e}")
    assert 3e3 < G[p1, p1] / direct < 3e4
    assert abs(S - direct) <= 1e-9 * direct and abs(q_bb - beta @ beta) <= 1e-14 * q_bb


_PLANTED = {}


def planted_runs(seed):
    if seed not in _PLANTED:
        X, y, rows = planted()
        _PLANTED[seed] = (rows, run(X, y, 4.0, seed), run(X, y, np.inf, seed))
    return _PLANTED[seed]


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_planted_gross_errors(seed):
    rows, student, gauss = planted_runs(seed)
    assert student['counts'][0, 0] < 0 and gauss['counts'][0, 0] < 0
    sd_t, sd_g = np.sqrt(student['sigsqd'].mean()), np.sqrt(gauss['sigsqd'].mean())
    weight_mean = student['lam_sum'][0] / 400
    clean = np.ones(weight_mean.shape[0], dtype=bool)
    clean[rows] = False
    err_t = np.max(np.abs(student['betas'][0].mean(axis=0) - BETA_TRUE))
    err_g = np.max(np.abs(gauss['betas'][0].mean(axis=0) - BETA_TRUE))
    print(f"seed {seed}: sd {sd_t:.4f} (nu = 4), {sd_g:.4f} (nu = inf); planted rows' weight_mean at most "
          f"{weight_mean[rows].max():.4f}, clean rows average {weight_mean[clean].mean():.3f}, {int((weight_mean[clean] < 0.3).sum())} "
          f"below 0.3; largest coefficient error {err_t:.4f} against {err_g:.4f}")
    assert abs(sd_t - 0.05) <= 0.1 * 0.05
    assert sd_g > 3 * 0.05
    assert np.all(weight_mean[rows] < 0.1)
    assert (weight_mean[clean] < 0.3).sum() <= 0.01 * clean.sum()
    assert err_t < 0.5 * err_g
    assert np.array_equal(gauss['lam_sum'][0], np.full(2000, 400.0))


def test_constant_weights_rescale_the_chain():
    """w = c: sigsqd -> c sigsqd and tausqd -> tausqd / c with b -> c b, btau -> btau / c; the betas are the unweighted
    chain's (c = 4: every scaled quantity is the same mantissa)."""
    X, y, _ = planted(300, 15)
    base = run(X, y, 4.0, 5, burnin=3, draws=20)
    scaled = run(X, y, 4.0, 5, w=np.full(300, 4.0), burnin=3, draws=20, b=0.04, btau=0.25)
    assert np.allclose(scaled['betas'], base['betas'], rtol=1e-10, atol=0.0)
    assert np.allclose(scaled['sigsqd'], 4.0 * base['sigsqd'], rtol=1e-10) and np.allclose(scaled['tausqd'], base['tausqd'] / 4.0, rtol=1e-10)
    assert np.array_equal(scaled['attempts'], base['attempts'])
    assert np.allclose(scaled['lam_sum'], base['lam_sum'], rtol=1e-10)


def test_doubling_a_rows_weight_moves_the_mean_by_the_closed_form(monkeypatch):
    quiet_z(monkeypatch)
    X, y, _ = planted(300, 15)
    n, p1, tausqd, i = 300, 5, 0.3, 17
    w = np.ones(n)
    G = RB.pass_host(X, y, w, None, 1.0, np.inf, 0, 0, 0)[0]
    m = RB.step_host(G, 0.01, tausqd, hyper(n, p1), 1, 0, 1)[0]
    w[i] = 2.0
    G2 = RB.pass_host(X, y, w, None, 1.0, np.inf, 0, 0, 0)[0]
    m2 = RB.step_host(G2, 0.01, tausqd, hyper(n, p1), 1, 0, 1)[0]
    Ainv_x = np.linalg.solve(X.T @ X + np.eye(p1) / tausqd, X[i])      # Sherman-Morrison: one more copy of row i
    expect = m + Ainv_x * (y[i] - X[i] @ m) / (1.0 + X[i] @ Ainv_x)
    assert np.max(np.abs(m2 - m)) > 1e-6
    assert np.max(np.abs(m2 - expect)) < 1e-12 * np.max(np.abs(m))


def test_chains_are_independent_and_thin_selects_rows():
    X, y, _ = planted(200, 10)
    sig0, tau0 = 0.002 * (1.0 + 0.1 * np.arange(3)), 0.2 * (1.0 + 0.2 * np.arange(3))
    three = run(X, y, 4.0, 6, chains=3, burnin=2, draws=9, sig0=sig0, tau0=tau0)
    alone = run(X, y, 4.0, 6, chains=1, burnin=2, draws=9, sig0=sig0[2:], tau0=tau0[2:], chain_ids=[2])
    for key in three:
        assert np.array_equal(three[key][2:], alone[key]), key
    assert not np.array_equal(three['betas'][0], three['betas'][1])
    thinned = run(X, y, 4.0, 6, chains=3, burnin=2, draws=9, thin=3, sig0=sig0, tau0=tau0)
    assert thinned['betas'].shape == (3, 3, 5)
    for key in ('betas', 'sigsqd', 'tausqd', 'attempts'):
        assert np.array_equal(thinned[key], three[key][:, ::3]), key
    for key in ('sums', 'counts', 'lam_sum'):
        assert np.array_equal(thinned[key], three[key]), key
    none = run(X, y, 4.0, 6, chains=3, burnin=2, draws=9, sig0=sig0, tau0=tau0, rows=False)
    assert none['betas'] is None and np.array_equal(none['sums'], three['sums']) and np.array_equal(none['lam_sum'], three['lam_sum'])


def test_a_flagged_chain_is_nan_from_there_on_and_alone():
    """bstar < 0 through b = -0.45 y'y: a chain started at tausqd = 1e-12 draws beta ~ 0, sees the whole of y'y in bstar and
    passes iteration 0; chain 1, started with a flat prior, sees the residual sum only and does not."""
    X, y, _ = planted(200, 10)
    b = -0.45 * float(y @ y)
    sig0, tau0 = np.full(3, 0.01), np.array([1e-12, 1e6, 1e-12])
    out = run(X, y, 4.0, 2, chains=3, burnin=0, draws=4, b=b, sig0=sig0, tau0=tau0)
    assert out['counts'][1, 0] == 0 and np.all(out['counts'][[0, 2], 0] == 1) and np.all(out['counts'][:, 1] == RB.FLAG_BSTAR_NEGATIVE)
    assert np.isnan(out['sigsqd'][1]).all() and np.isnan(out['betas'][1, 1:]).all() and np.isfinite(out['betas'][1, 0]).all()
    assert np.isfinite(out['betas'][[0, 2], 0]).all()
    tau0[1] = 1e-12
    twin = run(X, y, 4.0, 2, chains=3, burnin=0, draws=4, b=b, sig0=sig0, tau0=tau0)
    for key in out:
        assert np.array_equal(twin[key][[0, 2]], out[key][[0, 2]], equal_nan=True), key
    # a pivot that is not positive flags too, with its own reason
    G = RB.pass_host(X, y, None, None, 1.0, np.inf, 0, 0, 0)[0]
    G[2, 2] = -100.0
    beta, sig, tau, flag = RB.step_host(G, 0.01, 0.2, hyper(200, 5), 0, 0, 1)
    assert flag == RB.FLAG_PIVOT and np.isnan(beta).any() and np.isnan(sig)


def small_model():
    rng = np.random.default_rng(4)
    inputs = rng.uniform(size=(60, 2))
    mtx = np.array([[1, 0], [0, 1]])
    data = 1.0 + inputs[:, 0] - inputs[:, 1] + 0.05 * rng.standard_normal(60)
    return [mtx, getKernels.bernoulli(), KERNEL, inputs, data, 4.0, 0.1, 4.0, 1.0]


def test_the_result_of_one_call():
    res = RB.resample_robust_host(*small_model(), nu=4.0, chains=2, draws=30, burnin=5, thin=2, seed=3)
    assert res.betas.shape == (30, 3) and res.sigsqd.shape == (30,) and res.kept == 15 and res.noise == 'student' and res.nu == 4.0
    assert np.array_equal(res.chain, np.repeat(np.arange(2), 15)) and res.weight_mean.shape == (60,)
    assert np.allclose(res.noise_var, 2.0 * res.sigsqd) and not res.flagged.any() and res.attempts_total > 35 * 60 * 2
    assert res.rhat['betas'].shape == (3,) and res.ess['betas'].shape == (3,) and res.chain_mean['betas'].shape == (2, 3)
    none = RB.resample_robust_host(*small_model(), nu=4.0, chains=2, draws=30, burnin=5, thin=2, seed=3, keep=None)
    assert none.betas is None and none.ess is None and np.array_equal(none.sums, res.sums)
    assert np.array_equal(none.weight_mean, res.weight_mean)
    assert np.all(np.isinf(RB.resample_robust_host(*small_model(), nu=1.5, chains=1, draws=4, burnin=0).noise_var))


def test_refusals_name_the_limit():
    args = small_model()
    for kw, text in ((dict(nu=0.5), 'nu = 0.5 < 1'), (dict(nu=np.nan), 'NaN'), (dict(weights=np.ones(59)), 'one value per row'),
                     (dict(weights=np.r_[np.ones(59), np.inf]), 'finite and > 0'), (dict(weights=np.r_[np.ones(59), 0.0]), 'drop a row'),
                     (dict(keep='w'), 'keep must be'), (dict(chains=0), 'chains must be'), (dict(init='x'), 'init must be'),
                     (dict(thin=0), 'thin must be'), (dict(seed=0.5), 'seed must be')):
        with pytest.raises(ValueError, match=text):
            RB.resample_robust_host(*args, **kw)
    wide = list(args)
    wide[0] = np.stack([np.arange(127) % 12 + 1, np.arange(127) // 12 + 1], axis=1)
    with pytest.raises(ValueError, match='at most 127'):
        RB.resample_robust_host(*wide)
    wide[0] = wide[0][:126]                                              # 127 columns are taken
    RB._prepare(*wide, 4.0, None, 1, 1, 0, 1, 0, 'reference', 'betas')
    for i, text in ((0, 'fitted model'), (6, 'hyper-parameter b')):
        broken = list(args)
        broken[i] = None
        with pytest.raises(ValueError, match=text):
            RB.resample_robust_host(*broken)
    broken = list(args)
    broken[4] = args[4][:-1]
    with pytest.raises(ValueError, match='one finite value per row'):
        RB.resample_robust_host(*broken)


def test_score_and_predictive_refuse_student_noise():
    mtx, phis, kernel, inputs, data, a, b, atau, btau = small_model()
    res = RB.resample_robust_host(mtx, phis, kernel, inputs, data, a, b, atau, btau, nu=4.0, chains=1, draws=30, burnin=0)
    model = FoKLRoutines.FoKL(kernel=kernel, phis=phis, UserWarnings=False, ConsoleOutput=False)
    model.mtx, model.inputs, model.data = mtx, inputs, data
    for call in (model.score, model.predictive):
        with pytest.raises(ValueError, match='Gaussian likelihood'):
            call(res)
        with pytest.raises(ValueError, match='Gaussian likelihood'):
            call(dict(betas=res.betas, sigsqd=res.sigsqd, nu=4.0))


def test_numpys_stream_is_left_alone():
    np.random.seed(5)
    state = np.random.get_state()
    RB.resample_robust_host(*small_model(), chains=1, draws=3, burnin=1)
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]

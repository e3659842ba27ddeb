"""predictive.py's host statement (predictive_rows_host, predictive_host) against independent definitions; no device.

What the statement is checked against:
  * one draw and identical draws, where quantiles and PIT have closed forms;
  * an independent solver: scipy.optimize.brentq on a separately written F (a plain loop over math.erfc) on seven cases
    regenerated from fixed seeds (``CASES``), with the bound |F_independent(q) - p| <= ftol + E 2^-53 (the rounding of the
    independent sum of E terms of at most 1/2 each, divided by E, is below E 2^-53) and no pair unresolved;
  * a step-like CDF, where pairs end on the width test and are counted;
  * the pass-0 bracket; calibration of data drawn from the predictive itself, against the band of the mean;
  * its rounding sensitivity (``rounding_sensitivity``, which test_predictive_gpu.py turns into the device tolerances);
  * every refusal, ``draws`` and the fields of a PredictiveResult.
"""
import math

import numpy as np
import pytest
from scipy.optimize import brentq

import helpers  # noqa: F401  (puts the repository on sys.path)
from fokl_gpy_amd import predictive as pd, getKernels, FoKLRoutines
from fokl_gpy_amd.embedded import basis_matrix

P7 = np.array([0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999])
Z7 = np.array([pd.normal_quantile(v) for v in P7])
ROUND = 2.0 ** -53


def case(name):
    """(X [S, 2], betas [E, 2], sigsqd [E]) of a named case: mu[i, d] = c_d + a_i w_d, four rows that shift and stretch the
    same mixture.  Regenerated from a fixed seed per case."""
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    E = CASES[name]
    a = np.array([0.0, 0.3, 1.0, 2.5])
    if name == 'unimodal':
        c, w, sd = rng.standard_normal(E), 0.2 * rng.standard_normal(E), 0.5 + rng.random(E)
    elif name == 'two_modes':
        c, w, sd = np.where(rng.random(E) < 0.3, 0.0, 100.0) + 0.01 * rng.standard_normal(E), 0.01 * rng.standard_normal(E), \
            np.full(E, 0.05)
    elif name == 'narrow':
        c, w = rng.random(E), 0.1 * rng.random(E)
        sd = np.full(E, 1e-4 * (c.max() - c.min()))
    elif name == 'four_decades':
        c, w, sd = rng.standard_normal(E), 0.1 * rng.standard_normal(E), 10.0 ** (-4.0 + 4.0 * rng.random(E))
    elif name == 'model_like':
        c, w, sd = 1.0 + 0.005 * rng.standard_normal(E), 0.002 * rng.standard_normal(E), 0.1 * (1.0 + 0.05 * rng.random(E))
    elif name == 'one_draw':
        c, w, sd = np.array([0.7]), np.array([-0.4]), np.array([0.3])
    elif name == 'identical':
        c, w, sd = np.full(E, 0.7), np.full(E, -0.4), np.full(E, 0.3)
    elif name == 'steps':
        c, w = rng.random(E), 0.1 * rng.random(E)
        sd = np.full(E, 1e-9 * (c.max() - c.min()))
    return np.stack([np.ones(4), a], axis=1), np.stack([c, w], axis=1), sd * sd


CASES = dict(unimodal=1000, two_modes=1000, narrow=25, four_decades=64, model_like=1000, one_draw=1, identical=100, steps=25)
SEVEN = ('unimodal', 'two_modes', 'narrow', 'four_decades', 'model_like', 'one_draw', 'identical')


def solved(name, y=None, p=P7, z=Z7, **kw):
    X, betas, sigsqd = case(name)
    sd, rinv = pd.scales(sigsqd)
    return X @ betas.T, sd, rinv, pd.predictive_rows_host(X, betas, sd, rinv, y, p, z, **kw)


def F_independent(mu_row, rinv, q):
    total = 0.0
    for m, r in zip(mu_row, rinv):
        total += 0.5 * math.erfc(-(q - m) * r)
    return total / len(mu_row)


def test_the_normal_quantiles_by_newton_steps_on_erfc():
    from scipy.special import ndtri
    for v in (1e-300, 1e-12, 0.001, 0.025, 0.1, 0.3, 0.5, 0.75, 0.975, 0.999, 1 - 1e-12):
        assert pd.normal_quantile(v) == pytest.approx(float(ndtri(v)), rel=4e-15, abs=1e-16)
    assert pd.normal_quantile(0.975) == pytest.approx(1.959963984540054, rel=1e-15)
    assert pd.normal_quantile(0.975) == -pd.normal_quantile(1.0 - 0.975)        # the upper half by symmetry


def test_one_draw_and_identical_draws_have_closed_forms():
    y = np.array([0.1, 0.5, 1.0, -2.0])
    for name in ('one_draw', 'identical'):
        mu, sd, rinv, block = solved(name, y)
        per = block[:, 6:].reshape(4, 7, 5)
        assert np.array_equal(per[:, :, 0], mu[:, :1] + sd[0] * Z7)
        pit = np.array([0.5 * math.erfc((m - v) * rinv[0]) for m, v in zip(mu[:, 0], y)])
        assert np.allclose(block[:, 5], pit, rtol=4e-15, atol=0.0)   # two erfc implementations and a sum of equal terms
        assert np.all(per[:, :, 4] == 1) and np.all(np.abs(per[:, :, 1]) <= 1e-13)
        assert np.array_equal(per[:, :, 2], per[:, :, 3])            # the bracket is a point
    one, many = solved('one_draw', y)[3], solved('identical', y)[3]
    assert np.allclose(one[:, 6:].reshape(4, 7, 5)[:, :, 0], many[:, 6:].reshape(4, 7, 5)[:, :, 0], rtol=1e-15, atol=1e-16)
    assert np.allclose(one[:, 5], many[:, 5], rtol=1e-13, atol=0.0)


@pytest.mark.parametrize('name', SEVEN)
def test_every_quantile_against_an_independent_solver(name):
    """brentq (xtol 1e-15) on F_independent inside the pass-0 bracket.  Passes used at most, as run here: unimodal 6,
    two_modes 18, narrow 18, four_decades 13, model_like 4, one_draw 1, identical 1."""
    mu, sd, rinv, block = solved(name)
    E = mu.shape[1]
    bound = pd.FTOL + E * ROUND
    per = block[:, 6:].reshape(4, 7, 5)
    first = solved(name, max_passes=0)[3][:, 6:].reshape(4, 7, 5)
    print(f"{name}: most passes {int(per[:, :, 4].max())}, largest |r| {np.abs(per[:, :, 1]).max():.2e}")
    assert np.all(np.abs(per[:, :, 1]) <= pd.FTOL)                   # no pair unresolved: the condition the prototype met
    for i in range(4):
        for j in range(7):
            q = per[i, j, 0]
            assert abs(F_independent(mu[i], rinv, q) - P7[j]) <= bound, (i, j)
            lo, hi = first[i, j, 2], first[i, j, 3]
            if hi > lo:
                root = brentq(lambda v: F_independent(mu[i], rinv, v) - P7[j], lo, hi, xtol=1e-15)
                assert abs(F_independent(mu[i], rinv, q) - F_independent(mu[i], rinv, root)) <= 2.0 * bound, (i, j)
            else:
                assert q == lo


def test_step_like_cdfs_end_on_the_width_test_and_are_counted():
    """sd = 1e-9 of the spread, 25 draws.  Between the steps the density underflows and the passes bisect: about 30 to reach
    a step, a few Newton steps on it, and once the residual stops halving (one ulp of q moves F by 1e-9) bisection again
    down to the width -- more than the default 32 passes, which would report the same pairs as unresolved for running out.
    128 passes let them end on the width test; as run here the most any pair used was 54, and 24 of the 28 pairs ended unresolved (p = 0.5 sits on a step's middle)."""
    mu, sd, rinv, block = solved('steps', max_passes=128)
    per = block[:, 6:].reshape(4, 7, 5)
    first = solved('steps', max_passes=0)[3][:, 6:].reshape(4, 7, 5)
    unresolved = np.abs(per[:, :, 1]) > pd.FTOL
    width = block[:, 4] - block[:, 3] + sd.max()
    print('most passes', per[:, :, 4].max(), 'unresolved', int(unresolved.sum()))
    assert unresolved.any() and np.all(per[:, :, 4] < 128)                 # stopped, not run out
    assert np.all((per[:, :, 3] - per[:, :, 2])[unresolved] <= (pd.XTOL * width)[:, None].repeat(7, axis=1)[unresolved])
    bound = 25 * ROUND
    for i in range(4):
        for j in range(7):
            lo, hi = per[i, j, 2], per[i, j, 3]
            assert F_independent(mu[i], rinv, lo) - P7[j] <= bound and F_independent(mu[i], rinv, hi) - P7[j] >= -bound
            root = brentq(lambda v: F_independent(mu[i], rinv, v) - P7[j], first[i, j, 2], first[i, j, 3], xtol=1e-15)
            slack = 1e-15 + 4.0 * np.finfo(float).eps * abs(root)                    # brentq's own xtol + rtol |root|
            assert lo - slack <= root <= hi + slack, (i, j)


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_pass_zero_bracket_is_exact(name):
    mu, sd, rinv, block = solved(name, max_passes=0)
    per = block[:, 6:].reshape(4, 7, 5)
    assert np.all(per[:, :, 4] == 0) and np.all(np.isinf(per[:, :, 1]))
    slack = mu.shape[1] * ROUND
    for i in range(4):
        for j in range(7):
            assert F_independent(mu[i], rinv, per[i, j, 2]) <= P7[j] + slack
            assert F_independent(mu[i], rinv, per[i, j, 3]) >= P7[j] - slack
            assert per[i, j, 2] <= per[i, j, 0] <= per[i, j, 3]


# ---------------------------------------------------------------------------------------------------------
# predictive_host: the public surface without a device
# ---------------------------------------------------------------------------------------------------------

MTX = np.array([[1, 0], [0, 1], [2, 0], [1, 1]])


def model_case(S=50, E=120, seed=6, from_predictive=False):
    rng = np.random.default_rng(seed)
    phis = getKernels.bernoulli()
    x = rng.random((S, 2))
    X = basis_matrix(x, MTX, phis, 'Bernoulli Polynomials')
    mean = rng.standard_normal(5)
    betas = mean + 0.02 * rng.standard_normal((E, 5))
    sig = 0.04 * (1 + 0.3 * rng.random(E))
    if from_predictive:                                              # y_i from draw d_i of the mixture itself
        pick = rng.integers(0, E, size=S)
        y = np.einsum('ik,ik->i', X, betas[pick]) + np.sqrt(sig[pick]) * rng.standard_normal(S)
    else:
        y = X @ mean + 0.2 * rng.standard_normal(S)
    return dict(betas=betas, sigsqd=sig, mtx=MTX, phis=phis, kernel='Bernoulli Polynomials', inputs=x, data=y), X


def test_calibration_has_meaning():
    """S = 4 000 rows drawn from the predictive itself (seed 6, 200 draws).  Observed here: pit_ks 0.0096 against the 1 %
    Kolmogorov critical value 1.63 / sqrt(S) = 0.0258; the (0.025, 0.975) interval covers 0.9435, within 4 binomial
    standard deviations (0.0138) of 0.95; the band of the MEAN alone (the order statistics evaluate / coverage3 take: sorted
    X betas' at cut = floor(0.025 E) + 1 and E - cut) covers 0.1610 of the same rows.  That is why this exists."""
    S, E = 4000, 200
    kw, X = model_case(S, E, seed=6, from_predictive=True)
    res = pd.predictive_host(quantiles=(0.025, 0.5, 0.975), **kw)
    band = 4.0 * math.sqrt(0.95 * 0.05 / S)
    cover = res.coverage[0]
    mu = np.sort(X @ kw['betas'].T, axis=1)
    cut = int(np.floor(E * 0.025) + 1)
    mean_band = float(np.mean((mu[:, cut] <= kw['data']) & (kw['data'] <= mu[:, E - cut])))
    print(f"pit_ks {res.pit_ks:.4f} (critical {1.63 / math.sqrt(S):.4f}), coverage {cover['observed']:.4f}, the mean's band "
          f"{mean_band:.4f}, unresolved {res.unresolved}, most passes {res.passes.max()}")
    assert res.unresolved == 0
    assert res.pit_ks < 1.63 / math.sqrt(S)
    assert (cover['lower'], cover['upper']) == (0.025, 0.975) and cover['nominal'] == pytest.approx(0.95)
    assert abs(cover['observed'] - 0.95) <= band
    assert mean_band < 0.95 - band
    assert res.pit_hist.shape == (20,) and res.pit_hist.sum() == pytest.approx(1.0) and np.abs(res.pit_hist - 0.05).max() < 0.02


def rounding_sensitivity(X, betas, sigsqd, y, p, seed=0, rel=1e-15):
    """How far a perturbation of every mu_id by ``rel`` x sum_k |X_ik beta_dk| with random signs (what another order of the
    product's sum may do, a few times over) moves the statement: the largest movement of (pit, mean, var, F(q) - p at the
    statement's own q)."""
    rng = np.random.default_rng(seed)
    sd, rinv = pd.scales(sigsqd)
    p = np.asarray(p, dtype=np.float64)
    z = np.array([pd.normal_quantile(v) for v in p])
    mu = X @ betas.T
    mu2 = mu + rel * (np.abs(X) @ np.abs(betas).T) * rng.choice([-1.0, 1.0], size=mu.shape)
    E = mu.shape[1]
    a = pd.predictive_rows_from_means(mu, sd, rinv, y, p, z)
    b = pd.predictive_rows_from_means(mu2, sd, rinv, y, p, z, max_passes=0)
    moments = lambda blk: (blk[:, 0] + blk[:, 1] / E, (blk[:, 2] - blk[:, 1] ** 2 / E) / E)
    moved_F = 0.0
    for j in range(p.shape[0]):
        q = a[:, 6 + 5 * j]
        moved_F = max(moved_F, float(np.abs(pd.mixture_cdf(mu2, rinv, q) - pd.mixture_cdf(mu, rinv, q)).max()))
    return np.array([np.abs(a[:, 5] - b[:, 5]).max(), np.abs(moments(a)[0] - moments(b)[0]).max(),
                     np.abs(moments(a)[1] - moments(b)[1]).max(), moved_F])


def test_rounding_sensitivity_of_the_statement():
    """On the model case (50 rows, 120 draws, |mu| about 1, sd 0.2) a perturbation of 1e-15 moved pit by 3.3e-16, mean by
    3.3e-16, var by 1.1e-17 and F by 6.7e-16: a few ulp each.  test_predictive_gpu.py's tolerances are this measurement, on
    the case under test, times 100."""
    kw, X = model_case()
    moved = rounding_sensitivity(X, kw['betas'], kw['sigsqd'], kw['data'], (0.025, 0.5, 0.975))
    print("moved by", moved)
    assert np.all(moved > 0.0) and moved[0] < 1e-13 and moved[1] < 1e-14 and moved[2] < 1e-14 and moved[3] < 1e-13


def test_predictive_host_fields_and_consistency():
    kw, X = model_case()
    res = pd.predictive_host(quantiles=(0.05, 0.25, 0.5, 0.75, 0.95, 0.9), **kw)
    S, E = 50, 120
    mu = X @ kw['betas'].T
    assert res.rows == S and res.draws == E and np.array_equal(res.p, [0.05, 0.25, 0.5, 0.75, 0.95, 0.9])
    assert np.allclose(res.mean, mu.mean(axis=1), rtol=1e-13) and np.allclose(res.sd ** 2, mu.var(axis=1) + kw['sigsqd'].mean(), rtol=1e-12)
    assert res.quantiles.shape == res.residual.shape == res.passes.shape == (S, 6) and res.brackets.shape == (S, 6, 2)
    assert res.unresolved == 0 and res.unresolved_rows.shape == (0,) and res.passes.min() >= 1
    assert np.all(np.diff(res.quantiles[:, [0, 1, 2, 3, 5, 4]], axis=1) > 0.0)
    assert np.all(res.brackets[:, :, 0] <= res.quantiles) and np.all(res.quantiles <= res.brackets[:, :, 1])
    assert [(c['lower'], c['upper']) for c in res.coverage] == [(0.05, 0.95), (0.25, 0.75)]          # 0.9 has no partner
    assert res.inside.shape == (S, 2) and res.inside.dtype == bool
    y = kw['data']
    assert np.array_equal(res.inside[:, 0], (res.quantiles[:, 0] <= y) & (y <= res.quantiles[:, 4]))
    assert res.coverage[1]['observed'] == res.inside[:, 1].mean() and res.coverage[1]['nominal'] == 0.5
    assert res.pit_ks == pytest.approx(np.max(np.abs(np.sort(res.pit) - (np.arange(S) + 0.5) / S)) + 0.5 / S)
    assert np.array_equal(np.round(res.pit_hist * S), np.histogram(res.pit, bins=20, range=(0.0, 1.0))[0])
    assert res['pit'] is res.pit
    with pytest.raises(AttributeError):
        res.nothing
    only = pd.predictive_host(quantiles=(), **kw)                   # the PIT alone, from pass 0
    assert np.array_equal(only.pit, res.pit) and only.quantiles.shape == (S, 0) and only.coverage == [] and only.unresolved == 0
    bare = pd.predictive_host(**dict(kw, data=None))                # quantiles alone
    assert 'pit' not in bare and 'coverage' not in bare and np.array_equal(bare.p, pd.DEFAULT_QUANTILES)
    assert np.array_equal(bare.quantiles[:, 1], res.quantiles[:, 2])
    last = pd.predictive_host(draws=50, **kw)
    ref = pd.predictive_host(**dict(kw, betas=kw['betas'][70:], sigsqd=kw['sigsqd'][70:]))
    assert last.draws == 50 and np.array_equal(last.quantiles, ref.quantiles) and np.array_equal(last.pit, ref.pit)
    state = np.random.get_state()[1].copy()
    pd.predictive_host(draws=np.arange(0, 120, 3), **kw)
    assert np.array_equal(np.random.get_state()[1], state)


def test_unresolved_pairs_are_reported():
    kw, _ = model_case()
    res = pd.predictive_host(max_passes=1, quantiles=(0.1, 0.9), **kw)
    bad = np.abs(res.residual) > pd.FTOL
    assert res.unresolved == int(bad.sum()) > 0 and np.array_equal(res.unresolved_rows, np.flatnonzero(bad.any(axis=1)))
    none = pd.predictive_host(max_passes=0, quantiles=(0.1, 0.9), **kw)
    assert none.unresolved == 100 and np.all(np.isinf(none.residual)) and np.all(none.passes == 0)
    pr = dict(S=1500, E=2, p=np.array([0.5]), data=None, sd=np.ones(2), ftol=pd.FTOL)
    block = np.zeros((1500, 11))
    block[:1200, 7] = 1.0
    many = pd._assemble(pr, block)
    assert many.unresolved == 1200 and np.array_equal(many.unresolved_rows, np.arange(1000))


def test_refusals_name_the_limit():
    kw, _ = model_case()
    with pytest.raises(ValueError, match='sigsqd holds 119 values, betas has 120 rows'):
        pd.predictive_host(**dict(kw, sigsqd=kw['sigsqd'][:119]))
    nan = kw['betas'].copy()
    nan[40:80] = np.nan
    with pytest.raises(ValueError, match='40 of the 120 draws are NaN.*flagged.*drop them'):
        pd.predictive_host(**dict(kw, betas=nan))
    assert pd.predictive_host(draws=np.r_[0:40, 80:120], **dict(kw, betas=nan)).draws == 80
    with pytest.raises(ValueError, match='positive'):
        pd.predictive_host(**dict(kw, sigsqd=-kw['sigsqd']))
    with pytest.raises(ValueError, match='resample'):
        pd.predictive_host(**dict(kw, sigsqd=None))
    with pytest.raises(ValueError, match='inputs'):
        pd.predictive_host(**dict(kw, inputs=None))
    with pytest.raises(ValueError, match='data must hold one finite value per row'):
        pd.predictive_host(**dict(kw, data=kw['data'][:-1]))
    with pytest.raises(ValueError, match='betas have 5 columns'):
        pd.predictive_host(**dict(kw, mtx=MTX[:2]))
    for bad in (0, 121, 2.5, np.array([0, 120]), np.zeros(0, dtype=int)):
        with pytest.raises(ValueError, match='draws'):
            pd.predictive_host(draws=bad, **kw)
    with pytest.raises(ValueError, match='9 quantiles are asked for, one call takes at most 8'):
        pd.predictive_host(quantiles=np.linspace(0.1, 0.9, 9), **kw)
    assert pd.predictive_host(quantiles=np.linspace(0.1, 0.9, 8), **kw).quantiles.shape == (50, 8)
    for bad in ((0.0, 0.5), (0.5, 1.0), (0.5, np.nan), (-0.1,), (np.inf,)):
        with pytest.raises(ValueError, match=r'strictly inside \(0, 1\)'):
            pd.predictive_host(quantiles=bad, **kw)
    with pytest.raises(ValueError, match='repeat'):
        pd.predictive_host(quantiles=(0.1, 0.5, 0.1), **kw)
    with pytest.raises(ValueError, match='max_passes must be an integer >= 0'):
        pd.predictive_host(max_passes=-1, **kw)
    for name in ('ftol', 'xtol'):
        for bad in (-1e-13, np.nan, np.inf):
            with pytest.raises(ValueError, match=f'{name} must be finite and >= 0'):
                pd.predictive_host(**{name: bad}, **kw)
    with pytest.raises(ValueError, match='neither data nor quantiles'):
        pd.predictive_host(quantiles=(), **dict(kw, data=None))


def test_a_fit_alone_is_refused_with_a_pointer_to_resample():
    model = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', UserWarnings=False, ConsoleOutput=False)
    model.betas, model.mtx = np.zeros((10, 5)), MTX
    with pytest.raises(ValueError, match='sigma\\^2.*resample'):
        model.predictive()
    with pytest.raises(ValueError, match='resample'):
        model.predictive(betas=model.betas)
    with pytest.raises(ValueError, match='not both'):
        model.predictive(dict(betas=model.betas, sigsqd=np.ones(10)), betas=model.betas)
    with pytest.raises(ValueError, match='kept no rows'):
        model.predictive(dict(betas=None, sigsqd=None))

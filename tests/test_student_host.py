"""score and predictive under Student-t noise and row weights: the host statement (score.log_likelihood / score_rows_host and
predictive.student_terms / student_quantile / predictive_rows_host with ``nu`` and ``sw``) against scipy, which none of
them uses for the t distribution; what the t likelihood is worth on planted gross errors and on t noise; the defaults, which
are the calls as they were; the refusals.  No device."""
import numpy as np
import pytest
import scipy.special
import scipy.stats
from scipy.optimize import brentq

from fokl_gpy_amd import FoKLRoutines, predictive as pd, robust as RB, score as sc
from test_robust_host import BETA_TRUE, columns, planted_runs, planted, run, small_model

EPS = np.finfo(float).eps
NUS = (1.0, 1.5, 2.0, 3.0, 4.0, 7.3, 30.0, 64.0, float(pd.NU_MAX))
P7 = np.array([0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999])


def cdf_points():
    rng = np.random.default_rng(0)
    mag = 10.0 ** rng.uniform(-8.0, 6.0, 2000)
    return np.concatenate([np.linspace(-50.0, 50.0, 20001), np.where(rng.random(2000) < 0.5, -mag, mag)])


# ---------------------------------------------------------------------------------------------------------
# 1. the t CDF, density and quantile
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nu', NUS)
def test_student_cdf_against_stdtr(nu):
    """Absolute error <= 1e-14 over 20 001 points on [-50, 50] and 2 000 of magnitude 1e-8 .. 1e6, at every nu up to NU_MAX,
    with every point converged inside the fixed iteration bound.  In the lower tail (t < 0, stdtr >= 1e-300) the RELATIVE
    error is bounded by 20 times what was measured when the statement was written: 2.3e-15 (nu = 1), 5.8e-15 (1.5), 4.9e-15
    (2), 6.2e-15 (3), 1.6e-14 (4), 2.5e-14 (7.3), 7.6e-14 (30), 1.7e-13 (64); it grows with nu as the argument of the one
    exp, (nu + 1) / 2 log1p(t^2 / nu), does, each unit of which carries an ulp.  The largest measured, 1.7e-13, stands for
    all: the bound is 20 x 1.7e-13 = 3.4e-12."""
    t = cdf_points()
    ours, ref = pd.student_cdf(t, nu), scipy.special.stdtr(nu, t)
    err = np.abs(ours - ref).max()
    low = (t < 0.0) & (ref >= 1e-300)
    rel = (np.abs(ours - ref)[low] / ref[low]).max()
    print(f"nu {nu:g}: absolute {err:.2e}, relative in the lower tail {rel:.2e}")
    assert err <= 1e-14
    assert rel <= 20.0 * 1.7e-13
    assert np.all(np.diff(pd.student_cdf(np.sort(t), nu)) >= -4.0 * EPS)             # monotone to rounding
    # every argument has converged inside the bound: twice the bound changes no bit
    bound = pd.STUDENT_ITERATIONS
    try:
        pd._STUDENT.clear()
        pd.STUDENT_ITERATIONS = 2 * bound
        longer = pd.student_cdf(t, nu)
    finally:
        pd.STUDENT_ITERATIONS = bound
        pd._STUDENT.clear()
    assert np.array_equal(longer, ours)


@pytest.mark.parametrize('nu', NUS)
def test_student_pdf_against_scipy(nu):
    """1e-14 relative where (nu + 1) / 2 log1p(t^2 / nu) <= 16, i.e. down to 1e-7 of the peak: the density is exp of minus
    that number on both sides, and an exp returns its argument's rounding, half an ulp per unit, as relative error; 16 units
    on our side (product and log1p) and as many on scipy's are 16 x 2 x 2.2e-16 = 7e-15, the rest is the constant's."""
    t = np.linspace(-50.0, 50.0, 20001)
    t = t[0.5 * (nu + 1.0) * np.log1p(t * t / nu) <= 16.0]
    assert t.shape[0] >= 300
    rel = np.abs(pd.student_pdf(t, nu) / scipy.stats.t.pdf(t, nu) - 1.0).max()
    print(f"nu {nu:g}: {t.shape[0]} points, relative {rel:.2e}")
    assert rel <= 1e-14


def test_gamma_ratio_does_not_cancel():
    for a in (0.5, 1.0, 2.0, 31.7, 79.9, 80.0, 128.0, 5e3, 5e8):
        ref = np.exp(scipy.special.gammaln(a + 0.5) - scipy.special.gammaln(a)) if a < 100 else \
            np.sqrt(a) * np.exp(-1.0 / (8.0 * a) + 1.0 / (192.0 * a ** 3))
        assert abs(sc.gamma_ratio(a) / ref - 1.0) <= (1e-13 if a < 100 else 1e-15 + 1.0 / (640.0 * a ** 5)), a


@pytest.mark.parametrize('nu', NUS)
def test_student_quantile_is_the_root_of_our_own_cdf(nu):
    """|student_cdf(student_quantile(p)) - p| <= 4e-16 max(p, 1 - p) + eps |z| f(z): a few ulp of the larger of the two tails,
    which is what the kernel's absolute residual sees, and the CDF's own granularity at z (one ulp of z moves it by eps |z| f)."""
    p = np.concatenate([10.0 ** np.linspace(-6.0, np.log10(0.5), 40), 1.0 - 10.0 ** np.linspace(-6.0, np.log10(0.4), 40)])
    z = np.array([pd.student_quantile(v, nu) for v in p])
    T, f = pd.student_terms(z, nu)
    gap = np.abs(T - p)
    bound = 4e-16 * np.maximum(p, 1.0 - p) + EPS * np.abs(z) * f
    print(f"nu {nu:g}: largest |T(z) - p| {gap.max():.2e}, largest share of its bound {(gap / bound).max():.2f}")
    assert np.all(gap <= bound)
    assert np.all(np.diff(z[np.argsort(p)]) > 0.0) and pd.student_quantile(0.5, nu) == 0.0
    ref = scipy.special.stdtrit(nu, p)                                   # scipy's own inverse is good to 1e-11 of p only
    assert np.all(np.abs(scipy.special.stdtr(nu, z) - p) <= 1e-14 + 1e-13 * p) and np.allclose(z, ref, rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------
# 2. the log likelihood
# ---------------------------------------------------------------------------------------------------------

def ll_case(seed=3, S=300, E=40, nc=6):
    rng = np.random.default_rng(seed)
    X = np.concatenate([np.ones((S, 1)), rng.standard_normal((S, nc - 1))], axis=1)
    betas = rng.standard_normal(nc) + 0.05 * rng.standard_normal((E, nc))
    sig = 0.3 * np.exp(0.2 * rng.standard_normal(E))
    y = X @ betas.mean(axis=0) + np.sqrt(0.3) * rng.standard_t(3, S)
    w = rng.choice([0.25, 1.0, 4.0], S)
    return X, y, betas, sig, w


@pytest.mark.parametrize('nu', [1.0, 2.5, 4.0, 30.0, 64.0, 1e3, 1e9])
def test_ll_against_scipy_t_logpdf(nu):
    """The bound is derived: the log term L = log1p(.) carries 4 ulp (the square, the product with g, log1p itself and the
    product with hp) and is scaled by hp = (nu + 1) / 2; c_d + lw adds a few ulp of its own size, and scipy's value has
    as much again."""
    X, y, betas, sig, w = ll_case()
    for weights in (None, w):
        sw = None if weights is None else np.sqrt(weights)
        ours = sc.log_likelihood(X, y, betas, sig, nu, sw)
        scale = np.sqrt(sig)[None, :] / (1.0 if sw is None else sw[:, None])
        mu = X @ betas.T
        ref = scipy.stats.t.logpdf(y[:, None], nu, loc=mu, scale=scale)
        L = np.log1p(((y[:, None] - mu) / scale) ** 2 / nu)
        bound = 2.0 * (0.5 * (nu + 1.0) * 4.0 * EPS * L + 8.0 * EPS * (1.0 + np.abs(ref)))
        if nu >= 1e3:                                                    # scipy's constant is a difference of two gammaln there
            bound = bound + 4.0 * EPS * scipy.special.gammaln(0.5 * nu)
        print(f"nu {nu:g} weights {weights is not None}: largest error {np.abs(ours - ref).max():.2e}, largest share of its bound "
              f"{(np.abs(ours - ref) / bound).max():.2f}")
        assert np.all(np.abs(ours - ref) <= bound)


def test_ll_at_a_huge_nu_is_the_gaussian_ll():
    """log t_nu = log N + O(u^4 / (4 nu)), u = e / sd: at nu = 1e9 within max u^4 / (4 nu) (plus the rounding of log1p's tiny
    argument times hp, 4 ulp of u^2 / 2)."""
    X, y, betas, sig, w = ll_case()
    sw = np.sqrt(w)
    t = sc.log_likelihood(X, y, betas, sig, 1e9, sw)
    g = sc.log_likelihood(X, y, betas, sig, np.inf, sw)
    u = (y[:, None] - X @ betas.T) * sw[:, None] / np.sqrt(sig)
    # u^4 / (4 nu) from the log term, (u^2 + 1) / (2 nu) + 1 / (4 nu) from the constant and the factor (nu + 1) / nu
    bound = (u ** 4).max() / 4e9 + ((u * u).max() + 2.0) / 2e9 + 8.0 * EPS * (1.0 + np.abs(g).max() + (u * u).max())
    print(f"largest |ll_t - ll_gauss| {np.abs(t - g).max():.2e}, bound {bound:.2e}, max |u| {np.abs(u).max():.2f}")
    assert np.abs(t - g).max() <= bound
    ref = scipy.stats.norm.logpdf(y[:, None], loc=X @ betas.T, scale=np.sqrt(sig)[None, :] / sw[:, None])
    assert np.abs(g - ref).max() <= 16.0 * EPS * (1.0 + np.abs(ref).max())


def test_constant_weights_shift_the_weighted_gaussian_ll():
    """w = c with sigsqd -> c sigsqd is the same density: ll(w = c, c sigsqd) = ll(1, sigsqd) up to rounding -- the c_d of
    c sigsqd is lower by 0.5 log c, which lw = 0.5 log c gives back (c = 4: every scaled quantity is the same mantissa)."""
    X, y, betas, sig, _ = ll_case()
    for nu in (np.inf, 4.0):
        base = sc.log_likelihood(X, y, betas, sig, nu, None)
        shifted = sc.log_likelihood(X, y, betas, 4.0 * sig, nu, np.full(X.shape[0], 2.0))
        plain = sc.log_likelihood(X, y, betas, 4.0 * sig, nu, None)
        assert np.abs(shifted - base).max() <= 8.0 * EPS * (1.0 + np.abs(base).max())
        # the weights alone: every ll moves by 0.5 log c and by what sw^2 does to the quadratic term
        u2 = (y[:, None] - X @ betas.T) ** 2 / (4.0 * sig)
        moved = 0.5 * np.log(4.0) - (3.0 * u2 / 2.0 if np.isinf(nu) else 2.5 * (np.log1p(4.0 * u2 / nu) - np.log1p(u2 / nu)))
        assert np.abs((shifted - plain) - moved).max() <= 64.0 * EPS * (1.0 + np.abs(base).max())


# ---------------------------------------------------------------------------------------------------------
# 3. quantiles of mixtures against brentq on a CDF built from stdtr
# ---------------------------------------------------------------------------------------------------------

def mixtures():
    """name -> (mu [S, E], sigsqd [E]): unimodal; two modes 100 apart; sd over four decades; sd 1e-4 of the spread; one draw."""
    rng = np.random.default_rng(11)
    S, E = 6, 60
    shift = np.linspace(-1.0, 1.0, S)[:, None]
    return {
        'unimodal': (shift + 0.3 * rng.standard_normal((S, E)), 0.25 * np.exp(0.2 * rng.standard_normal(E))),
        'two modes': (shift + np.where(rng.random(E) < 0.3, -50.0, 50.0) + 0.01 * rng.standard_normal((S, E)), np.full(E, 0.05 ** 2)),
        'four decades': (shift + 0.3 * rng.standard_normal((S, E)), 10.0 ** rng.uniform(-8.0, 0.0, E)),
        'hard': (shift + rng.uniform(-50.0, 50.0, (S, E)), np.full(E, 0.01 ** 2)),
        'one draw': (shift + np.zeros((S, 1)), np.array([0.49])),
    }


def reference_cdf(mu_row, scale_row, nu):
    return lambda q: float(np.mean(scipy.special.stdtr(nu, (q - mu_row) / scale_row)))


_MIXTURE_PASSES = {}


@pytest.mark.parametrize('nu', [1.0, 2.5, 4.0, 30.0, 64.0])
@pytest.mark.parametrize('name', ['unimodal', 'two modes', 'four decades', 'hard', 'one draw'])
def test_mixture_quantiles_against_brentq(name, nu):
    mu, sig = mixtures()[name]
    S, E = mu.shape
    w = np.resize([0.25, 1.0, 4.0], S)
    sw = np.sqrt(w)
    sd, rinv = pd.scales(sig)
    z = np.array([pd.student_quantile(v, nu) for v in P7])
    block = pd.predictive_rows_from_means(mu, sd, rinv, None, P7, z, nu=nu, sw=sw)
    per = block[:, 6:].reshape(S, 7, 5)
    unresolved = []
    for i in range(S):
        scale = sd / sw[i]
        F = reference_cdf(mu[i], scale, nu)
        for j, p in enumerate(P7):
            q, r, lo, hi, passes = per[i, j]
            a, b = (mu[i] + scale * z[j]).min(), (mu[i] + scale * z[j]).max()
            span = b - a + scale.max()
            root = brentq(lambda v: F(v) - p, a - span, b + span, xtol=1e-300, rtol=4.0 * EPS, maxiter=500)
            # the bracket holds brentq's root -- or, where the CDF is flat and the root ill-conditioned, ends where stdtr's
            # mixture is within 2e-14 of p: it differs from the statement's by 1e-14 at most (test 1)
            near = lo - 4.0 * EPS * abs(lo) <= root <= hi + 4.0 * EPS * abs(hi)      # where it is steep an ulp of q is 3e-14 of F
            assert lo <= q <= hi and (near or abs(F(min(max(root, lo), hi)) - p) <= 2e-14), (name, nu, i, j, lo, root, hi)
            if abs(r) <= pd.FTOL:
                # stdtr and student_cdf differ by 1e-14 at most (test 1), and so do their means
                assert abs(F(q) - p) <= pd.FTOL + 1e-14 and 1 <= passes <= pd.MAX_PASSES, (name, nu, i, j, F(q) - p)
            else:
                unresolved.append((i, j, float(r), int(passes)))
    most = int(per[:, :, 4].max())
    _MIXTURE_PASSES[(name, nu)] = most
    print(f"{name}, nu {nu:g}: most passes {most}, unresolved {len(unresolved)} of {S * 7}: {unresolved}")
    if name != 'hard':
        assert not unresolved                                            # every pair inside 32 passes
    else:
        # a pair may end unresolved here: it is counted and listed above, and its bracket holds the root (asserted above)
        res = pd._assemble(dict(S=S, E=E, p=P7, data=None, sd=sd, ftol=pd.FTOL, nu=nu, sw=sw), block)
        assert res.unresolved == len(unresolved) and sorted(set(i for i, *_ in unresolved)) == res.unresolved_rows.tolist()


# ---------------------------------------------------------------------------------------------------------
# 4. and 5. what the t likelihood is worth
# ---------------------------------------------------------------------------------------------------------

def assembled_predictive(X, y, betas, sig, nu, quantiles):
    p = np.asarray(quantiles, dtype=np.float64)
    sd, rinv = pd.scales(sig)
    z = np.array([pd.student_quantile(v, nu) if np.isfinite(nu) else pd.normal_quantile(v) for v in p])
    block = pd.predictive_rows_host(X, betas, sd, rinv, y, p, z, nu=nu)
    return pd._assemble(dict(S=X.shape[0], E=betas.shape[0], p=p, data=y, sd=sd, ftol=pd.FTOL, nu=nu, sw=None), block)


@pytest.mark.parametrize('seed', [0, 1])
def test_t_noise_is_calibrated_where_the_gaussian_formula_is_not(seed):
    """4 000 rows of y = X beta + 0.05 t_4, the nu = 4 posterior, every 4th draw."""
    rng = np.random.default_rng(7)
    n = 4000
    X = columns(rng.uniform(size=(n, 2)))
    y = X @ BETA_TRUE + 0.05 * rng.standard_t(4, n)
    out = run(X, y, 4.0, seed)
    betas, sig = out['betas'][0][::4], out['sigsqd'][0][::4]
    quantiles = (0.025, 0.25, 0.75, 0.975)
    t = assembled_predictive(X, y, betas, sig, 4.0, quantiles)
    g = assembled_predictive(X, y, betas, sig, np.inf, quantiles)        # the Gaussian formula on the very same draws
    cover = {round(c['nominal'], 2): c['observed'] for c in t.coverage}
    cover_g = {round(c['nominal'], 2): c['observed'] for c in g.coverage}
    print(f"seed {seed}: t pit_ks {t.pit_ks:.4f} (critical {1.36 / np.sqrt(n):.4f}), coverage {cover}; gaussian pit_ks "
          f"{g.pit_ks:.4f}, coverage {cover_g}; unresolved {t.unresolved}")
    assert t.noise == 'student' and t.nu == 4.0 and not t.weighted and g.noise == 'gaussian' and t.unresolved == 0
    assert t.pit_ks <= 1.36 / np.sqrt(n)
    assert abs(cover[0.95] - 0.95) <= 3.0 * np.sqrt(0.95 * 0.05 / n)
    assert abs(cover[0.5] - 0.5) <= 3.0 * np.sqrt(0.5 * 0.5 / n)
    assert cover_g[0.95] < 0.91
    assert np.allclose(t.sd ** 2, (t.sd ** 2 - 2.0 * np.mean(sig)) + 2.0 * np.mean(sig)) and np.all(t.sd > g.sd)


@pytest.mark.parametrize('seed', [0, 1])
def test_compare_favours_t_on_planted_gross_errors(seed):
    rows, student, gauss = planted_runs(seed)
    X, y, _ = planted()

    def scored(out, nu):
        betas, sig = out['betas'][0], out['sigsqd'][0]
        stats = sc.score_rows_host(X, y, betas, sig, want_loo=False, nu=nu)
        return sc._assemble(dict(S=X.shape[0], E=betas.shape[0], methods=('waic',), nu=nu, sw=None), stats)

    t, g = scored(student, 4.0), scored(gauss, np.inf)
    cmp = sc.compare(t, g)
    print(f"seed {seed}: elpd_waic {t.elpd_waic:.0f} (t) against {g.elpd_waic:.0f} (gaussian); difference {cmp.elpd_diff:.0f}, SE "
          f"{cmp.se_diff:.1f}, ratio {cmp.elpd_diff / cmp.se_diff:.1f}")
    assert cmp.measure == 'elpd_waic' and t.noise == 'student' and g.noise == 'gaussian'
    assert cmp.elpd_diff > 10.0 * cmp.se_diff
    worst = np.argsort(t.pointwise['elpd_waic'])[:len(rows)]
    assert len(set(worst.tolist()) & set(rows.tolist())) >= 0.9 * len(rows)      # the rows it predicts badly are the planted ones


# ---------------------------------------------------------------------------------------------------------
# 6. the defaults are the calls as they were; refusals
# ---------------------------------------------------------------------------------------------------------

def host_model(monkeypatch):
    """A FoKL whose score / predictive run the host statement: ``FoKL.score`` hands over to ``score.score`` with a device."""
    mtx, phis, kernel, inputs, data, a, b, atau, btau = small_model()
    model = FoKLRoutines.FoKL(kernel=kernel, phis=phis, UserWarnings=False, ConsoleOutput=False)
    model.mtx, model.inputs, model.data = mtx, inputs, data
    monkeypatch.setattr(model, '_backend', lambda: None)
    drop = lambda f: (lambda *args, device=None, **kw: f(*args, **kw))
    monkeypatch.setattr(FoKLRoutines._score, 'score', drop(sc.score_host))
    monkeypatch.setattr(FoKLRoutines._predictive, 'predictive', drop(pd.predictive_host))
    return model, (mtx, phis, kernel, inputs, data, a, b, atau, btau)


def same(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for key in a:
        if isinstance(a[key], dict):
            same(a[key], b[key])
        elif isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        else:
            assert a[key] == b[key] or (a[key] != a[key] and b[key] != b[key]), key


def test_the_defaults_are_the_calls_as_they_were(monkeypatch):
    model, args = host_model(monkeypatch)
    mtx, phis, kernel, inputs, data = args[:5]
    gauss = RB.resample_robust_host(*args, nu=np.inf, chains=1, draws=40, burnin=5)
    plain = dict(betas=gauss.betas, sigsqd=gauss.sigsqd)
    X = FoKLRoutines._score.basis_matrix(inputs, mtx, phis, kernel)
    # today's formulas, restated here, are what the default path computes bit for bit
    e = data[:, None] - X @ gauss.betas.T
    ll = np.array([-0.5 * np.log(2.0 * np.pi * s) for s in gauss.sigsqd]) - (e * e) * (0.5 / gauss.sigsqd)
    assert np.array_equal(sc.log_likelihood(X, data, gauss.betas, gauss.sigsqd), ll)
    base_s = sc.score_host(gauss.betas, gauss.sigsqd, mtx, phis, kernel, inputs, data)
    base_p = pd.predictive_host(gauss.betas, gauss.sigsqd, mtx, phis, kernel, inputs, data)
    assert base_s.noise == base_p.noise == 'gaussian' and np.isinf(base_s.nu) and not base_s.weighted and not base_p.weighted
    same(sc.score_host(gauss.betas, gauss.sigsqd, mtx, phis, kernel, inputs, data, nu=np.inf, weights=None), base_s)
    same(pd.predictive_host(gauss.betas, gauss.sigsqd, mtx, phis, kernel, inputs, data, nu=np.inf, weights=None), base_p)
    # weights of one through the weighted statement: other code, the same operations on the same numbers, the same bits
    ones = np.ones(inputs.shape[0])
    weighted = pd.predictive_host(gauss.betas, gauss.sigsqd, mtx, phis, kernel, inputs, data, weights=ones)
    assert weighted.weighted
    for key in ('pit', 'quantiles', 'residual', 'brackets', 'passes', 'mean', 'sd'):
        assert np.array_equal(weighted[key], base_p[key]), key
    assert np.array_equal(sc.score_host(gauss.betas, gauss.sigsqd, mtx, phis, kernel, inputs, data, weights=ones).pointwise['lppd'],
                          base_s.pointwise['lppd'])
    # FoKL: a plain result under 'posterior' is the default call; so is a robust nu = inf result with weights of one
    same(model.score(plain, likelihood='posterior'), model.score(plain))
    same(model.predictive(plain, likelihood='posterior'), model.predictive(plain))
    same(model.score(gauss, likelihood='posterior'), model.score(gauss))
    same(model.score(plain), base_s)
    same(model.predictive(plain), base_p)


def test_posterior_likelihood_reads_nu_and_weights_from_the_result(monkeypatch):
    model, args = host_model(monkeypatch)
    mtx, phis, kernel, inputs, data = args[:5]
    w = np.resize([0.25, 1.0, 4.0], inputs.shape[0])
    res = RB.resample_robust_host(*args, nu=4.0, weights=w, chains=1, draws=40, burnin=5)
    for call in (model.score, model.predictive):                         # the default refuses, as ever, and says what to pass
        with pytest.raises(ValueError, match="Gaussian likelihood.*likelihood='posterior'$"):
            call(res)
    s = model.score(res, likelihood='posterior')
    same(s, sc.score_host(res.betas, res.sigsqd, mtx, phis, kernel, inputs, data, nu=4.0, weights=w))
    assert s.noise == 'student' and s.nu == 4.0 and s.weighted
    p = model.predictive(res, likelihood='posterior')
    same(p, pd.predictive_host(res.betas, res.sigsqd, mtx, phis, kernel, inputs, data, nu=4.0, weights=w))
    assert p.noise == 'student' and p.weighted and np.all(np.isfinite(p.sd)) and p.unresolved == 0
    # other inputs: ones by default, weights= for those rows
    new = inputs[:7] * 0.9 + 0.05
    same(model.predictive(res, inputs=new, likelihood='posterior'),
         pd.predictive_host(res.betas, res.sigsqd, mtx, phis, kernel, new, None, nu=4.0))
    same(model.score(res, inputs=new, data=data[:7], likelihood='posterior', weights=w[:7], method='lpd'),
         sc.score_host(res.betas, res.sigsqd, mtx, phis, kernel, new, data[:7], nu=4.0, weights=w[:7], method='lpd'))
    # nu = inf with weights: the weights are no longer ignored
    gw = RB.resample_robust_host(*args, nu=np.inf, weights=w, chains=1, draws=40, burnin=5)
    sg = model.score(gw, likelihood='posterior')
    assert sg.noise == 'gaussian' and sg.weighted and not np.array_equal(sg.pointwise['lppd'], model.score(gw).pointwise['lppd'])
    # the moments of the predictive
    heavy = pd.predictive_host(res.betas, res.sigsqd, mtx, phis, kernel, inputs, data, nu=2.0)
    cauchy = pd.predictive_host(res.betas, res.sigsqd, mtx, phis, kernel, inputs, data, nu=1.0)
    assert np.all(np.isinf(heavy.sd)) and np.all(np.isfinite(heavy.mean)) and np.all(np.isnan(cauchy.mean)) and np.all(np.isinf(cauchy.sd))
    X = FoKLRoutines._score.basis_matrix(inputs, mtx, phis, kernel)
    assert np.allclose(p.sd ** 2, (X @ res.betas.T).var(axis=1) + np.mean(res.sigsqd) * (4.0 / 2.0) / w, rtol=1e-10, atol=0.0)


def test_refusals_name_the_limit(monkeypatch):
    model, args = host_model(monkeypatch)
    mtx, phis, kernel, inputs, data = args[:5]
    res = RB.resample_robust_host(*args, nu=4.0, chains=1, draws=30, burnin=0)
    n = inputs.shape[0]
    for f in (sc.score_host, pd.predictive_host):
        call = lambda **kw: f(res.betas, res.sigsqd, mtx, phis, kernel, inputs, data, **kw)
        for kw, text in ((dict(nu=0.5), 'nu = 0.5 is NaN or < 1'), (dict(nu=np.nan), 'NaN or < 1'), (dict(nu='x'), 'nu must be a number'),
                         (dict(weights=np.ones(n - 1)), f'one value per row \\({n}\\)'),
                         (dict(weights=np.r_[np.ones(n - 1), 0.0]), 'finite and > 0'),
                         (dict(weights=np.r_[np.ones(n - 1), np.inf]), 'finite and > 0')):
            with pytest.raises(ValueError, match=text):
                call(**kw)
    with pytest.raises(ValueError, match=f'beyond FOKL_PREDICTIVE_NU_MAX = {pd.NU_MAX}'):
        pd.predictive_host(res.betas, res.sigsqd, mtx, phis, kernel, inputs, data, nu=pd.NU_MAX + 1.0)
    assert sc.score_host(res.betas, res.sigsqd, mtx, phis, kernel, inputs, data, nu=1e9, method='waic').noise == 'student'
    assert pd.NU_MAX >= 64
    for call in (model.score, model.predictive):
        with pytest.raises(ValueError, match="likelihood must be one of \\('gaussian', 'posterior'\\)"):
            call(res, likelihood='student')
        with pytest.raises(ValueError, match="weights=...\\) needs likelihood='posterior'"):
            call(dict(betas=res.betas, sigsqd=res.sigsqd), weights=np.ones(n))
        with pytest.raises(ValueError, match=f"the posterior's weights hold {n - 1} values and {n} rows"):
            call(dict(betas=res.betas, sigsqd=res.sigsqd, nu=4.0, weights=np.full(n - 1, 2.0)), likelihood='posterior')
        with pytest.raises(ValueError, match='Gaussian likelihood'):
            call(dict(betas=res.betas, sigsqd=res.sigsqd, nu=4.0))


def test_numpys_stream_is_left_alone(monkeypatch):
    model, args = host_model(monkeypatch)
    res = RB.resample_robust_host(*args, nu=4.0, chains=1, draws=30, burnin=0)
    np.random.seed(5)
    state = np.random.get_state()
    model.score(res, likelihood='posterior')
    model.predictive(res, likelihood='posterior')
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]

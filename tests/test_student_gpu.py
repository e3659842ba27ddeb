"""fokl_score_rows_noise / fokl_predictive_rows_noise (the Student-t and weighted instances of score_kernel and
predictive_kernel, csrc/fokl_student.inc) and ``likelihood='posterior'`` on the device against their host statement.

  * exact -- pass 0 on integer columns, coefficients and z with sd = 1 and sw in {0.5, 1, 2} (``max_passes = 0``): mu0, s1, s2,
    min, max and the brackets mu +- z / sw are integer or dyadic arithmetic whatever the order of the sums, ``np.array_equal``
    against whole-array numpy.  This pins the lane map, the row's sw, the padding draws and the rows past the end.
  * rounded -- test_predictive_gpu.check_rounded's scheme restated for the t statement: PIT, moments, every quantile, the
    device's own residual and the score's statistics against predictive_rows_host / score_rows_host with ``nu`` and ``sw``,
    to 100 times the statement's own rounding sensitivity on that very case (every mu perturbed by 1e-15 sum |X beta|,
    computed on the host: nothing here is tuned against the kernel).
``score_report`` / ``predictive_report`` say which noise instance ran.
"""
import warnings

import numpy as np
import pytest

from test_score_gpu import stage, continuous_case
from test_predictive_gpu import split, lds_bytes, Z_INT, mixed_tile
from fokl_gpy_amd import _capi, FoKLRoutines
from fokl_gpy_amd import predictive as pd, score as sc
from fokl_gpy_amd.embedded import basis_matrix

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 1000)
DRAWS = (1, 15, 16, 17, 63, 64, 65, 1003)
WIDTHS = (1, 5, 129, 300)
QS = (0, 1, 3, 8)
NOISES = {'student': 4.0, 'gaussian_weighted': np.inf}


def row_sw(S):
    return np.resize([0.5, 1.0, 2.0, 2.0, 1.0], S)


def check_exact(ctx, S, E, nc, Q, noise, seed=0):
    rng = np.random.default_rng(seed)
    cols = rng.integers(-3, 4, size=(S, nc - 1)).astype(np.float64)
    betas = rng.integers(-3, 4, size=(E, nc)).astype(np.float64)
    y = rng.integers(-20, 21, size=S).astype(np.float64)
    sd, rinv = pd.scales(np.ones(E))
    z = np.array(Z_INT[Q], dtype=np.float64)
    p = (np.arange(Q) + 1.0) / (Q + 1.0)
    nu, sw = NOISES[noise], row_sw(S)
    slots, X = stage(ctx, cols, y)
    head, per = split(ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, max_passes=0, nu=nu, sw=sw), Q)
    mu = X @ betas.T
    d = mu - mu[:, :1]
    where = (S, E, nc, Q, noise)
    assert np.array_equal(head[:, 0], mu[:, 0]) and np.array_equal(head[:, 1], d.sum(axis=1)), where
    assert np.array_equal(head[:, 2], (d * d).sum(axis=1)), where
    assert np.array_equal(head[:, 3], mu.min(axis=1)) and np.array_equal(head[:, 4], mu.max(axis=1)), where
    assert np.array_equal(per[:, :, 2], mu.min(axis=1)[:, None] + z / sw[:, None]), where       # the row's own sw
    assert np.array_equal(per[:, :, 3], mu.max(axis=1)[:, None] + z / sw[:, None]), where
    assert np.all(np.isinf(per[:, :, 1])) and np.all(per[:, :, 4] == 0)
    assert np.all(per[:, :, 2] <= per[:, :, 0]) and np.all(per[:, :, 0] <= per[:, :, 3])
    host = pd.predictive_rows_host(X, betas, sd, rinv, y, p, z, max_passes=0, nu=nu, sw=sw)
    assert np.max(np.abs(head[:, 5] - host[:, 5])) <= 1e-14          # the same CDF on both sides, a few ulp of a value <= 1
    if Q:
        assert np.allclose(per[:, :, 0], split(host, Q)[1][:, :, 0], rtol=1e-14, atol=1e-14)     # the first trial: one sqrt
    rep = ctx.predictive_report()
    assert rep['noise'] == noise and rep['instance'] == ('pit_quantiles' if Q else 'pit')
    assert rep['row_tiles'] == -(-S // 16) and 1 <= rep['grid'] <= rep['row_tiles'] and rep['lds_bytes'] == lds_bytes(nc)
    assert rep['quantiles'] == Q and rep['passes_max'] == 0 and rep['passes_sum'] == 0 and rep['unresolved'] == S * Q


@pytest.mark.parametrize('noise', list(NOISES))
def test_the_lane_map_and_the_rows_own_sw(device_ctx, noise):
    """mu[row][draw] = draw + 1000 row and sw = 2^(row % 3 - 1): every minimum, maximum and bracket names its row and its
    row's sw; were rows and draws, or the rows' sw, placed otherwise, a row would show another row's numbers."""
    S, E = 37, 41
    slots, X = stage(device_ctx, np.arange(S, dtype=np.float64)[:, None], np.zeros(S))
    betas = np.stack([np.arange(E, dtype=np.float64), np.full(E, 1000.0)], axis=1)
    sd, rinv = pd.scales(np.ones(E))
    z = np.array([-2.0, 0.0, 2.0])
    sw = 2.0 ** (np.arange(S) % 3 - 1.0)
    block = device_ctx.predictive_rows_noise(slots, betas, sd, rinv, False, [0.1, 0.5, 0.9], z, max_passes=0, nu=NOISES[noise], sw=sw)
    head, per = split(block, 3)
    base = 1000.0 * np.arange(S)
    assert np.array_equal(head[:, 0], base) and np.array_equal(head[:, 3], base) and np.array_equal(head[:, 4], base + E - 1)
    assert np.array_equal(head[:, 1], np.full(S, E * (E - 1) / 2.0))
    assert np.array_equal(head[:, 2], np.full(S, (np.arange(E) ** 2.0).sum())) and np.array_equal(head[:, 5], np.zeros(S))
    assert np.array_equal(per[:, :, 2], base[:, None] + z / sw[:, None])
    assert np.array_equal(per[:, :, 3], base[:, None] + E - 1 + z / sw[:, None])
    rep = device_ctx.predictive_report()
    assert rep['instance'] == 'quantiles' and rep['noise'] == noise


@pytest.mark.parametrize('S', ROWS)
@pytest.mark.parametrize('E', DRAWS)
def test_exact_over_rows_and_draws(device_ctx, S, E):
    check_exact(device_ctx, S, E, nc=5, Q=3, noise='student', seed=S + E)


@pytest.mark.parametrize('noise', list(NOISES))
@pytest.mark.parametrize('nc', WIDTHS)
def test_exact_over_widths(device_ctx, nc, noise):
    check_exact(device_ctx, 17, 65, nc, Q=3, noise=noise, seed=nc)


@pytest.mark.parametrize('noise', list(NOISES))
@pytest.mark.parametrize('Q', QS)
def test_exact_over_the_number_of_quantiles(device_ctx, Q, noise):
    check_exact(device_ctx, 1000, 1003, 129, Q, noise, seed=Q)


# ---------------------------------------------------------------------------------------------------------
# rounded: the statement's own sensitivity
# ---------------------------------------------------------------------------------------------------------

def perturbed_means(X, betas, seed=0, rel=1e-15):
    rng = np.random.default_rng(seed)
    mu = X @ betas.T
    return mu, mu + rel * (np.abs(X) @ np.abs(betas).T) * rng.choice([-1.0, 1.0], size=mu.shape)


def mixture_cdf(mu, sd, rinv, q, nu, sw):
    """F [S] of the statement's mixtures at q [S]."""
    if np.isfinite(nu):
        return pd.student_cdf((q[:, None] - mu) * ((1.0 / sd)[None, :] * sw[:, None]), nu).sum(axis=1) / mu.shape[1]
    return pd.mixture_cdf(mu, rinv[None, :] * sw[:, None], q)


def predictive_sensitivity(X, betas, sig, y, p, z, nu, sw):
    """How far mu -> mu + 1e-15 sum |X beta| (random signs) moves the statement: (pit, mean, var, F(q) - p at its own q)."""
    sd, rinv = pd.scales(sig)
    mu, mu2 = perturbed_means(X, betas)
    E = mu.shape[1]
    a = pd.predictive_rows_from_means(mu, sd, rinv, y, p, z, nu=nu, sw=sw)
    b = pd.predictive_rows_from_means(mu2, sd, rinv, y, p, z, max_passes=0, nu=nu, sw=sw)
    moments = lambda blk: (blk[:, 0] + blk[:, 1] / E, (blk[:, 2] - blk[:, 1] ** 2 / E) / E)
    q = split(a, len(p))[1][:, :, 0]
    dF = max([np.abs(mixture_cdf(mu, sd, rinv, q[:, j], nu, sw) - mixture_cdf(mu2, sd, rinv, q[:, j], nu, sw)).max()
              for j in range(len(p))] + [0.0])
    return (np.abs(a[:, 5] - b[:, 5]).max(), np.abs(moments(a)[0] - moments(b)[0]).max(),
            np.abs(moments(a)[1] - moments(b)[1]).max(), dF), a


def check_rounded(dev, X, betas, sig, y, p, nu, sw):
    """The device block against the statement -> the device's own unresolved."""
    Q, E = len(p), betas.shape[0]
    sd, rinv = pd.scales(sig)
    z = np.array([pd.student_quantile(v, nu) if np.isfinite(nu) else pd.normal_quantile(v) for v in p])
    moved, host = predictive_sensitivity(X, betas, sig, y, p, z, nu, sw)
    first = split(pd.predictive_rows_host(X, betas, sd, rinv, y, p, z, max_passes=0, nu=nu, sw=sw), Q)[1]
    moments = lambda blk: (blk[:, 0] + blk[:, 1] / E, (blk[:, 2] - blk[:, 1] ** 2 / E) / E)
    err_pit = np.abs(dev[:, 5] - host[:, 5]).max()
    err_mean = np.abs(moments(dev)[0] - moments(host)[0]).max()
    err_var = np.abs(moments(dev)[1] - moments(host)[1]).max()
    per = split(dev, Q)[1]
    mu = X @ betas.T
    F = np.stack([mixture_cdf(mu, sd, rinv, per[:, j, 0], nu, sw) - p[j] for j in range(Q)], axis=1)
    print(f"S {X.shape[0]} E {E} nc {X.shape[1]} Q {Q} nu {nu:g}: pit {err_pit:.2e} mean {err_mean:.2e} var {err_var:.2e} "
          f"|F_host(q_dev) - p| {np.abs(F).max():.2e} |r_dev - that| {np.abs(per[:, :, 1] - F).max():.2e} against the sensitivity "
          f"{moved} x 100; passes {int(per[:, :, 4].max())} (host {int(split(host, Q)[1][:, :, 4].max())})")
    assert err_pit <= 100.0 * moved[0] and err_mean <= 100.0 * moved[1] and err_var <= 100.0 * moved[2]
    assert np.all(first[:, :, 2] <= per[:, :, 0]) and np.all(per[:, :, 0] <= first[:, :, 3])
    assert np.abs(F).max() <= pd.FTOL + 100.0 * moved[3]
    assert np.abs(per[:, :, 1] - F).max() <= pd.FTOL + 100.0 * moved[3]
    assert np.all(per[:, :, 2] <= per[:, :, 0]) and np.all(per[:, :, 0] <= per[:, :, 3]) and np.all(per[:, :, 4] >= 1)
    return int((np.abs(per[:, :, 1]) > pd.FTOL).sum())


@pytest.mark.parametrize('S, E, nc, p, nu', [(200, 1000, 100, (0.025, 0.5, 0.975), 4.0), (1000, 64, 5, (0.025, 0.5, 0.975), 1.0),
                                             (17, 1003, 300, (0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999, 0.9), 2.5),
                                             (100, 65, 129, (0.1,), 64.0), (33, 15, 1, (0.025, 0.5, 0.975), 30.0),
                                             (1000, 64, 5, (0.025, 0.5, 0.975), np.inf)])
def test_predictive_rounded_against_the_host_statement(device_ctx, S, E, nc, p, nu):
    cols, betas, y, sig = continuous_case(S, E, nc, S + E + nc)
    slots, X = stage(device_ctx, cols, y)
    sd, rinv = pd.scales(sig)
    sw = np.sqrt(np.resize([0.25, 1.0, 4.0], S))
    z = np.array([pd.student_quantile(v, nu) if np.isfinite(nu) else pd.normal_quantile(v) for v in p])
    call = lambda *a, **kw: device_ctx.predictive_rows_noise(slots, betas, sd, rinv, *a, nu=nu, sw=sw, **kw)
    dev = call(True, p, z)
    unresolved = check_rounded(dev, X, betas, sig, y, np.array(p), nu, sw)
    rep = device_ctx.predictive_report()
    assert rep['noise'] == ('student' if np.isfinite(nu) else 'gaussian_weighted') and rep['instance'] == 'pit_quantiles'
    assert rep['unresolved'] == unresolved and rep['quantiles'] == len(p)
    assert rep['passes_max'] == int(split(dev, len(p))[1][:, :, 4].max()) and rep['passes_sum'] >= rep['passes_max']
    assert np.array_equal(call(True, p, z), dev)                                                  # no atomics: the same bits
    only = call(True, [], [])                                                                     # the PIT alone
    assert only.shape == (S, 6) and np.array_equal(only, dev[:, :6]) and device_ctx.predictive_report()['instance'] == 'pit'
    bare = call(False, p, z)                                                                      # no data: pit is zero
    assert np.array_equal(bare[:, 5], np.zeros(S)) and np.array_equal(bare[:, 6:], dev[:, 6:])
    if np.isfinite(nu):                                                                           # without weights: sw = 1
        plain = device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=nu)
        assert np.array_equal(plain, device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=nu, sw=np.ones(S)))


def stats_of_ll(ll, want_loo):
    """score_rows_host from a given ll: everything after ll is the statement's own text."""
    keep = sc.log_likelihood
    try:
        sc.log_likelihood = lambda *a, **kw: ll
        return sc.score_rows_host(None, None, None, None, want_loo)
    finally:
        sc.log_likelihood = keep


def ll_of_means(mu, y, sig, nu, sw):
    e = sw[:, None] * (y[:, None] - mu)
    lw = np.log(sw)[:, None]
    if np.isfinite(nu):
        c, g, hp = sc.student_constants(sig, nu)
        return (c + lw) - hp * np.log1p((e * e) * g)
    c, h = sc.likelihood_constants(sig)
    return (c + lw) - (e * e) * h


@pytest.mark.parametrize('S, E, nc, nu', [(200, 1000, 100, 4.0), (1000, 64, 5, 1.0), (17, 1003, 300, 1e9), (100, 65, 129, 64.0),
                                          (33, 25, 1, 2.5), (1000, 64, 5, np.inf)])
def test_score_rounded_against_the_host_statement(device_ctx, S, E, nc, nu):
    cols, betas, y, sig = continuous_case(S, E, nc, S + E + nc)
    slots, X = stage(device_ctx, cols, y)
    sw = np.sqrt(np.resize([0.25, 1.0, 4.0], S))
    stats, tail = device_ctx.score_rows_noise(slots, betas, sig, True, True, nu=nu, sw=sw)
    ref, ref_tail = sc.score_rows_host(X, y, betas, sig, want_tail=True, nu=nu, sw=sw)
    mu, mu2 = perturbed_means(X, betas)
    assert np.array_equal(ll_of_means(mu, y, sig, nu, sw), sc.log_likelihood(X, y, betas, sig, nu, sw))
    moved = np.abs(stats_of_ll(ll_of_means(mu2, y, sig, nu, sw), True) - ref)
    err = np.abs(stats - ref)
    finite = np.isfinite(ref[:, 4]) & np.isfinite(stats[:, 4])
    print(f"S {S} E {E} nc {nc} nu {nu:g}: errors {[f'{err[finite, k].max():.2e}' for k in range(7)]} against the sensitivity "
          f"{[f'{moved[finite, k].max():.2e}' for k in range(7)]} x 100; tail {np.abs(tail - ref_tail).max():.2e}")
    assert np.array_equal(np.isfinite(stats[:, 4]), np.isfinite(ref[:, 4])) and np.array_equal(stats[:, 7], ref[:, 7])
    for k in range(7):
        assert err[finite, k].max() <= 100.0 * moved[finite, k].max(), sc.STATS[k]
    rep = device_ctx.score_report()
    assert rep['noise'] == ('student' if np.isfinite(nu) else 'gaussian_weighted') and rep['instance'] == 'waic_loo'
    assert rep['row_tiles'] == -(-S // 16) and rep['kernel_ms'] > 0.0
    again, again_tail = device_ctx.score_rows_noise(slots, betas, sig, True, True, nu=nu, sw=sw)
    assert np.array_equal(again, stats, equal_nan=True) and np.array_equal(again_tail, tail)        # the same bits
    waic = device_ctx.score_rows_noise(slots, betas, sig, False, nu=nu, sw=sw)
    assert np.array_equal(waic[:, :3], stats[:, :3]) and not waic[:, 3:].any() and device_ctx.score_report()['instance'] == 'waic'


# ---------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------

def test_a_hard_row_does_not_change_its_tile_mates(device_ctx):
    a, betas, sig = mixed_tile()
    sd, rinv = pd.scales(sig)
    p = (0.025, 0.5, 0.975)
    z = np.array([pd.student_quantile(v, 4.0) for v in p])
    slots, _ = stage(device_ctx, a[:, None], np.zeros(16))
    mixed = device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0)
    rep_mixed = device_ctx.predictive_report()
    easy = np.arange(16) != 7
    slots, _ = stage(device_ctx, a[easy][:, None], np.zeros(15))
    alone = device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0)
    rep_alone = device_ctx.predictive_report()
    assert np.array_equal(mixed[easy], alone)                        # bit for bit, in other lanes of another tile
    assert rep_mixed['passes_max'] > rep_alone['passes_max'] and rep_mixed['passes_max'] == split(mixed, 3)[1][7, :, 4].max()
    assert rep_alone['unresolved'] == 0


def test_rows_of_a_long_call_equal_a_short_call(device_ctx):
    cols, betas, y, sig = continuous_case(1000, 65, 9, 5)
    sd, rinv = pd.scales(sig)
    p = (0.05, 0.95)
    z = np.array([pd.student_quantile(v, 4.0) for v in p])
    sw = np.sqrt(np.resize([0.25, 1.0, 4.0], 1000))
    slots, _ = stage(device_ctx, cols, y)
    long = device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0, sw=sw)
    long_s = device_ctx.score_rows_noise(slots, betas, sig, True, nu=4.0, sw=sw)
    slots, _ = stage(device_ctx, cols[:17], y[:17])
    short = device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0, sw=sw[:17])
    assert np.array_equal(long[:17], short)
    assert np.array_equal(device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0, sw=sw[:17]), short)
    assert np.array_equal(long_s[:17], device_ctx.score_rows_noise(slots, betas, sig, True, nu=4.0, sw=sw[:17]), equal_nan=True)


# ---------------------------------------------------------------------------------------------------------
# the Gaussian unweighted call through the new entry points; refusals
# ---------------------------------------------------------------------------------------------------------

def test_gaussian_unweighted_is_routed_to_the_parent(device_ctx):
    """nu = inf with sw = None through the new entry points is ROUTED to the parents' instances: their bits, noise 'gaussian'."""
    cols, betas, y, sig = continuous_case(200, 30, 4, 3)
    sd, rinv = pd.scales(sig)
    p = np.array([0.025, 0.975])
    z = np.array([pd.normal_quantile(v) for v in p])
    slots, _ = stage(device_ctx, cols, y)
    parent = device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
    assert device_ctx.predictive_report()['noise'] == 'gaussian'
    assert np.array_equal(device_ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z), parent)
    assert device_ctx.predictive_report()['noise'] == 'gaussian'
    parent = device_ctx.score_rows(slots, betas, sig, True)
    assert device_ctx.score_report()['noise'] == 'gaussian'
    assert np.array_equal(device_ctx.score_rows_noise(slots, betas, sig, True), parent, equal_nan=True)
    assert device_ctx.score_report()['noise'] == 'gaussian' and device_ctx.score_report()['instance'] == 'waic_loo'


def test_refusals_launch_nothing(device_ctx, monkeypatch):
    ctx = device_ctx
    cols, betas, y, sig = continuous_case(200, 30, 4, 3)
    sd, rinv = pd.scales(sig)
    p = np.array([0.025, 0.975])
    z = np.array([pd.student_quantile(v, 4.0) for v in p])
    slots, X = stage(ctx, cols, y)
    sw = np.ones(200)
    before = ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0, sw=sw)
    before_s = ctx.score_rows_noise(slots, betas, sig, True, nu=4.0, sw=sw)
    ctx.timing_enable(True)
    ctx.timing_reset()

    def refused(match, **kw):
        args = dict(slots=slots, betas=betas, sd=sd, rinv=rinv, with_data=True, p=p, z=z, nu=4.0, sw=sw)
        args.update(kw)
        with pytest.raises(_capi.FoklNativeError, match=match) as exc:
            ctx.predictive_rows_noise(**args)
        assert exc.value.code == -2
        assert ctx.predictive_report()['instance'] == 'none' and ctx.predictive_report()['grid'] == 0

    def refused_score(match, **kw):
        args = dict(slots=slots, betas=betas, sigsqd=sig, want_loo=True, nu=4.0, sw=sw)
        args.update(kw)
        with pytest.raises(_capi.FoklNativeError, match=match) as exc:
            ctx.score_rows_noise(**args)
        assert exc.value.code == -2
        assert ctx.score_report()['instance'] == 'none' and ctx.score_report()['grid'] == 0

    try:
        for check in (refused, refused_score):
            check('nu is NaN or < 1', nu=0.5)
            check('nu is NaN or < 1', nu=float('nan'))
            check('every sw .* must be finite and > 0', sw=np.r_[np.ones(199), 0.0])
            check('every sw .* must be finite and > 0', sw=np.r_[np.ones(199), np.inf])
            check('every sw .* must be finite and > 0', sw=np.r_[np.nan, np.ones(199)])
            for bad in (np.nan, np.inf):                         # draws of a flagged chain, or overflowed ones
                spoiled = betas.copy()
                spoiled[0, 0] = bad
                check('_rows_noise: every coefficient must be finite', betas=spoiled)
                check('_rows_noise: every coefficient must be finite', betas=spoiled, nu=np.inf, sw=None)
        refused(f'beyond FOKL_PREDICTIVE_NU_MAX = {_capi.PREDICTIVE_NU_MAX}', nu=_capi.PREDICTIVE_NU_MAX + 1.0)
        refused('fokl_predictive_rows_noise: .*at most FOKL_PREDICTIVE_MAX_QUANTILES = 8', p=np.linspace(0.1, 0.9, 9), z=np.zeros(9))
        refused('max_passes must be >= 0', max_passes=-1)
        refused('neither data nor quantiles', with_data=False, p=[], z=[])
        refused('positive and finite', sd=-sd)
        monkeypatch.setenv('FOKL_PREDICTIVE_FREE_BYTES', str(64 << 20))
        refused(f'{200 * 8 + 4 * 8 * (_capi.PREDICTIVE_STUDENT_ITERATIONS + 1)} of row precisions and t coefficients.*the device has {64 << 20} free')
        monkeypatch.delenv('FOKL_PREDICTIVE_FREE_BYTES')
        monkeypatch.setenv('FOKL_SCORE_FREE_BYTES', str(64 << 20))
        refused_score(f'{200 * 8} of row precisions.*the device has {64 << 20} free')
        monkeypatch.delenv('FOKL_SCORE_FREE_BYTES')
        refused_score('fokl_score_rows_noise: PSIS needs at least 25 draws', betas=betas[:10], sigsqd=sig[:10])
        with pytest.raises(ValueError, match='sw holds 199 values, 200 rows'):
            ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0, sw=np.ones(199))
        with pytest.raises(ValueError, match='sw holds 199 values, 200 rows'):
            ctx.score_rows_noise(slots, betas, sig, True, nu=4.0, sw=np.ones(199))
        assert ctx.timing_get(_capi.K_PREDICTIVE)['launches'] == 0 and ctx.timing_get(_capi.K_SCORE)['launches'] == 0
    finally:
        ctx.timing_enable(False)
    assert np.array_equal(ctx.read_slot(2), cols[:, 0]) and np.array_equal(ctx.read_slot(_capi.SLOT_Y), y)
    assert np.array_equal(ctx.predictive_rows_noise(slots, betas, sd, rinv, True, p, z, nu=4.0, sw=sw), before)
    assert np.array_equal(ctx.score_rows_noise(slots, betas, sig, True, nu=4.0, sw=sw), before_s, equal_nan=True)
    assert ctx.score_rows_noise(slots, betas, sig, False, nu=1e9).shape == (200, 8)               # any finite nu >= 1 is scored


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------

def test_posterior_likelihood_after_a_fit_and_a_robust_resample():
    rng = np.random.default_rng(2024)
    n = 2000
    x = rng.random((n, 3))
    w = np.resize([0.25, 1.0, 4.0], n)
    y = np.sin(4 * x[:, 0]) + x[:, 1] * x[:, 2] + 0.05 * rng.standard_t(4, n) / np.sqrt(w)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', burnin=60, draws=60, UserWarnings=False, ConsoleOutput=False)
        np.random.seed(7)
        model.fit(x, y, clean=True)
        state = np.random.get_state()[1].copy()
        res = model.resample_robust(nu=4.0, weights=w, chains=4, draws=64, burnin=20, seed=5)
        assert not res.flagged.any() and res.nu == 4.0
        for call in (model.score, model.predictive):
            with pytest.raises(ValueError, match="Gaussian likelihood.*likelihood='posterior'"):
                call(res)
        p = (0.025, 0.25, 0.5, 0.75, 0.975)
        dev = model.predictive(res, quantiles=p, likelihood='posterior')
        scored = model.score(res, likelihood='posterior')
        assert model.setnos is None and np.array_equal(np.random.get_state()[1], state)
        args = (res.betas, res.sigsqd, model.mtx, model.phis, model.kernel, model.inputs, model.data)
        host = pd.predictive_host(*args, quantiles=p, nu=4.0, weights=w)
        host_s = sc.score_host(*args, nu=4.0, weights=w)
        assert sorted(dev.keys()) == sorted(host.keys()) and dev.rows == n and dev.draws == 256
        assert dev.noise == scored.noise == 'student' and dev.weighted and scored.weighted and dev.nu == scored.nu == 4.0
        X = basis_matrix(model.inputs, model.mtx, model.phis, model.kernel)
        data = np.asarray(model.data, dtype=np.float64).reshape(-1)
        sw = np.sqrt(w)
        sd, rinv = pd.scales(res.sigsqd)
        z = np.array([pd.student_quantile(v, 4.0) for v in p])
        moved, _ = predictive_sensitivity(X, res.betas, res.sigsqd, data, np.array(p), z, 4.0, sw)
        F = np.stack([mixture_cdf(X @ res.betas.T, sd, rinv, dev.quantiles[:, j], 4.0, sw) - p[j] for j in range(5)], axis=1)
        print(f"pit {np.abs(dev.pit - host.pit).max():.2e} mean {np.abs(dev.mean - host.mean).max():.2e} var "
              f"{np.abs(dev.sd ** 2 - host.sd ** 2).max():.2e} F {np.abs(F).max():.2e} against {moved} x 100; coverage "
              f"{dev.coverage}, pit_ks {dev.pit_ks:.4f}")
        assert np.abs(dev.pit - host.pit).max() <= 100.0 * moved[0] and np.abs(dev.mean - host.mean).max() <= 100.0 * moved[1]
        assert np.abs(dev.sd ** 2 - host.sd ** 2).max() <= 100.0 * moved[2] + 4.0 * np.finfo(float).eps * host.sd.max() ** 2
        assert np.abs(F).max() <= pd.FTOL + 100.0 * moved[3] and np.abs(dev.residual - F).max() <= pd.FTOL + 100.0 * moved[3]
        assert dev.unresolved == int((np.abs(dev.residual) > pd.FTOL).sum()) == 0
        mu, mu2 = perturbed_means(X, res.betas)
        ref = sc.score_rows_host(X, data, res.betas, res.sigsqd, nu=4.0, sw=sw)
        moved_s = np.abs(stats_of_ll(ll_of_means(mu2, data, res.sigsqd, 4.0, sw), True) - ref)
        for k, name in enumerate(('lppd', 'll_mean', 'p_waic', 'elpd_loo', 'khat', 'sigma')):
            ok = np.isfinite(host_s.pointwise['khat']) if 'khat' in host_s.pointwise else np.ones(n, dtype=bool)
            assert np.abs(scored.pointwise[name] - host_s.pointwise[name])[ok].max() <= 100.0 * moved_s[ok, k].max(), name
        assert model._backend().ctx.score_report()['noise'] == 'student'
        new = model.predictive(res, inputs=0.05 + 0.9 * rng.random((501, 3)), clean=True, likelihood='posterior')
        assert new.rows == 501 and 'pit' not in new and not new.weighted and new.unresolved == 0
        # a plain resample under 'posterior' takes the old entry point: the default call's bits
        post = model.resample(chains=4, draws=64, burnin=20, seed=5)
        a, b = model.predictive(post, quantiles=p), model.predictive(post, quantiles=p, likelihood='posterior')
        assert np.array_equal(a.quantiles, b.quantiles) and np.array_equal(a.pit, b.pit) and b.noise == 'gaussian'
        assert model._backend().ctx.predictive_report()['noise'] == 'gaussian'
        a, b = model.score(post), model.score(post, likelihood='posterior')
        assert np.array_equal(a.pointwise['elpd_loo'], b.pointwise['elpd_loo']) and a.elpd_waic == b.elpd_waic
        cmp = sc.compare(scored, model.score(res, likelihood='posterior', method='waic'))
        assert cmp.measure == 'elpd_waic' and cmp.elpd_diff == 0.0

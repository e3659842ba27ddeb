"""resample.resample_host, the statement of the posterior resampler (fokl_gpy_amd/resample.py): the posterior it samples
against the reference's own chain, the recursion against the project's chain on identical numbers, its gamma sampler, its
bookkeeping (thin / burnin / keep / chains), its diagnostics and its refusals.  No device."""
import os

import numpy as np
import pytest
import scipy.stats

from helpers import GOLDEN
from fokl_gpy_amd import FoKLRoutines, _capi, getKernels, resample as R

KERNEL = 'Bernoulli Polynomials'
SIGMAS = 6.0                    # 6 sigma over fewer than 100 coordinates: a false alarm below 1e-6
FIXTURES = ('bern_m3', 'bern_m6', 'bern_m8_capped')


def load_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=True)
    hypers = dict(a=4.0, atau=4.0)
    hypers.update({str(k): v for k, v in zip(g['hyper_keys'], g['hyper_vals']) if str(k) in ('a', 'atau')})
    phis = getKernels.bernoulli()
    cap = int(g['phis_cap'])
    if cap > 0:
        phis = phis[:cap]
    return dict(mtx=g['ref_mtx'], inputs=g['ref_norm_inputs'], data=g['ref_norm_data'].reshape(-1), betas=g['ref_betas'],
                a=float(hypers['a']), atau=float(hypers['atau']), b=float(g['ref_b']), btau=float(g['ref_btau']), phis=phis)


def run_host(f, **kw):
    return R.resample_host(f['mtx'], f['phis'], KERNEL, f['inputs'], f['data'], f['a'], f['b'], f['atau'], f['btau'], **kw)


def ess_of_rows(rows, chains=1):
    """(ESS of the mean, ESS of the variance) per column of rows [chains * n, D], chain-major."""
    by_chain = rows.reshape(chains, -1, rows.shape[1])
    centred = (by_chain - by_chain.mean(axis=(0, 1))) ** 2
    return (np.sum([R.ess_ips(c) for c in by_chain], axis=0), np.sum([R.ess_ips(c) for c in centred], axis=0))


def assert_same_distribution(ours, ours_chains, theirs, what, variances=True):
    """The 6-sigma rule: means within 6 s sqrt(1 / ESS_a + 1 / ESS_b) with s the pooled standard deviation; the ratio of
    the variances inside the F band of the same two-sided level."""
    ess_a, ess_va = ess_of_rows(ours, ours_chains)
    ess_b, ess_vb = ess_of_rows(theirs)
    ess_a, ess_va = np.minimum(ess_a, ours.shape[0]), np.minimum(ess_va, ours.shape[0])
    ess_b, ess_vb = np.minimum(ess_b, theirs.shape[0]), np.minimum(ess_vb, theirs.shape[0])
    na, nb = ours.shape[0], theirs.shape[0]
    pooled = np.sqrt(((na - 1) * ours.var(axis=0, ddof=1) + (nb - 1) * theirs.var(axis=0, ddof=1)) / (na + nb - 2))
    gap = np.abs(ours.mean(axis=0) - theirs.mean(axis=0))
    bound = SIGMAS * pooled * np.sqrt(1.0 / ess_a + 1.0 / ess_b)
    print(f"{what}: largest mean gap / bound {np.max(gap / bound):.3f}")
    assert np.all(gap <= bound), f"{what}: means differ by up to {np.max(gap / bound):.2f} of the 6-sigma bound"
    if not variances:
        return
    tail = scipy.stats.norm.sf(SIGMAS)
    ratio = ours.var(axis=0, ddof=1) / theirs.var(axis=0, ddof=1)
    low = scipy.stats.f.ppf(tail, ess_va - 1, ess_vb - 1)
    high = scipy.stats.f.isf(tail, ess_va - 1, ess_vb - 1)
    print(f"{what}: variance ratios in [{ratio.min():.3f}, {ratio.max():.3f}], band at least [{low.max():.3f}, {high.min():.3f}]")
    assert np.all((ratio >= low) & (ratio <= high)), f"{what}: a variance ratio leaves its F band"


@pytest.mark.parametrize('name', FIXTURES)
def test_same_posterior_as_the_references_chain(name):
    f = load_fixture(name)
    res = run_host(f, chains=16, draws=2000, burnin=500, seed=1)
    assert res.betas.shape == (16 * 2000, f['mtx'].shape[0] + 1) and not res.flagged.any()
    assert_same_distribution(res.betas, 16, f['betas'], name)


def synthetic_spectrum(p1, seed=5, n=4000):
    rng = np.random.default_rng(seed)
    lamb = n * np.sort(rng.uniform(0.01, 1.0, p1))
    beta = rng.standard_normal(p1)
    qty = lamb * beta
    dtd = float(np.sum(lamb * beta * beta) + n * 0.04)
    return dict(lamb=lamb, qty=qty, dtd=dtd, astar=4 + 1 + n / 2 + p1 / 2, atau_star=4 + (p1 - 1) / 2, b=0.8, btau=3.0,
                shift=beta.copy())


def test_it_is_the_recursion_it_claims_to_be():
    """One chain fed numpy's own normals and standard gammas equals fokl_gibbs_chain on the same stream to 1e-12 of each
    coordinate's scale (the bound tests/test_chain_device.py holds the chain kernels to)."""
    p1, draws = 37, 300
    s = synthetic_spectrum(p1)
    state = np.random.RandomState(2024).get_state()
    w_ref, sig_ref, tau_ref = _capi.gibbs_chain(s['lamb'], s['qty'], s['astar'], s['atau_star'], s['b'], s['btau'], s['dtd'],
                                                0.16, 0.6, draws, _capi.LegacyStream(state), want_sig_tau=True)
    rs = np.random.RandomState()
    rs.set_state(state)
    normals, gs, gt = np.empty((draws, p1)), np.empty(draws), np.empty(draws)
    for k in range(draws):                                     # FR:1527, 1541, 1547: the order the chain consumes the stream in
        normals[k] = rs.normal(size=p1)
        gs[k] = rs.standard_gamma(s['astar'])
        gt[k] = rs.standard_gamma(s['atau_star'])
    got = R.chains_host(s['lamb'], s['qty'], s['shift'], s['astar'], s['atau_star'], s['b'], s['btau'], s['dtd'], [0.16], [0.6],
                        0, draws, 1, 0, normals=normals, gammas=(gs, gt))
    scale = np.max(np.abs(w_ref), axis=0)
    assert np.max(np.abs(got['w'][0] - w_ref) / scale) < 1e-12
    assert np.max(np.abs(got['sigsqd'][0] / sig_ref - 1)) < 1e-12 and np.max(np.abs(got['tausqd'][0] / tau_ref - 1)) < 1e-12


@pytest.mark.parametrize('shape', [1.0, 4.5, 5e5])
def test_gamma_sampler(shape):
    n = 100_000
    per = 250
    got = np.array([R.standard_gamma(17, c, k, shape, which) for c in range(n // (2 * per)) for k in range(per)
                    for which in ('sigsqd', 'tausqd')])
    values, attempts = got[:, 0], got[:, 1]
    assert values.shape[0] == n and np.isfinite(values).all()
    p = scipy.stats.kstest(values, scipy.stats.gamma(shape).cdf).pvalue
    print(f"shape {shape}: KS p = {p:.4f}, attempts per variate {attempts.mean():.4f}, most {int(attempts.max())}")
    assert p > 1e-4
    assert attempts.max() < R.ATTEMPT_CAP and attempts.mean() < 1.06


def test_accept_decisions_are_not_decided_by_the_last_bit():
    """The kernel's log / cos are not glibc's: an accept decided by the last bit would part a device chain from its
    statement.  With the numbers of the device tests (seed 11, 257 chains x 257 iterations, both shapes) moved by one ulp
    either way, fewer than 1 chain in 100 changes any decision."""
    chains, iters, seed = 257, 257, 11
    changed = np.zeros(chains, dtype=bool)
    for shape, (pn, pu) in ((2158.5, (_capi.RES_SIG_NORMAL, _capi.RES_SIG_UNIFORM)),
                            (22.0, (_capi.RES_TAU_NORMAL, _capi.RES_TAU_UNIFORM))):
        b, c = R.gamma_constants(shape)
        x = np.array([[_capi.embedded_rng(seed, ch, k, pn, 2) for k in range(iters)] for ch in range(chains)])
        u = np.array([[_capi.embedded_rng(seed, ch, k, pu, 2) for k in range(iters)] for ch in range(chains)])

        def accept(x, u):
            with np.errstate(all='ignore'):
                v1 = 1.0 + c * x
                v, x2 = v1 * v1 * v1, x * x
                return (v1 > 0) & ((u < 1.0 - 0.0331 * (x2 * x2)) | (np.log(u) < 0.5 * x2 + b * ((1.0 - v) + np.log(v))))

        base = accept(x, u)
        for dx in (-np.inf, np.inf):
            for du in (-np.inf, np.inf):
                moved = accept(np.nextafter(x, dx), np.clip(np.nextafter(u, du), 0.0, 1.0))
                changed |= (moved != base).any(axis=(1, 2))
    assert changed.sum() <= chains // 100


def test_thin_burnin_keep_and_chains_are_consistent():
    f = load_fixture('bern_m3')
    full = run_host(f, chains=5, draws=40, burnin=7, thin=1, seed=3)
    thin = run_host(f, chains=5, draws=40, burnin=7, thin=3, seed=3)
    assert thin.kept == 14 and thin.betas.shape[0] == 5 * 14
    by_chain = full.betas.reshape(5, 40, -1)
    # (the draws themselves are equal bit for bit -- the eigenbasis rows below; betas = W Q' goes through a BLAS product
    # whose rounding may depend on the number of rows)
    assert np.allclose(thin.betas.reshape(5, 14, -1), by_chain[:, ::3], rtol=0, atol=1e-13)
    assert np.array_equal(thin.sigsqd.reshape(5, 14), full.sigsqd.reshape(5, 40)[:, ::3])
    assert np.array_equal(thin.chain, np.repeat(np.arange(5), 14))
    for key in ('w', 'sigsqd', 'tausqd'):                      # the sums see every iteration, whatever is kept
        assert np.array_equal(thin.rhat[key], full.rhat[key])
    # burn-in discards iterations of the same chain: 7 + 40 iterations from the start are the 47 of a run without burn-in
    long = run_host(f, chains=5, draws=47, burnin=0, seed=3)
    assert np.allclose(long.betas.reshape(5, 47, -1)[:, 7:], by_chain, rtol=0, atol=1e-13)
    # keep modes
    eig = run_host(f, chains=5, draws=40, burnin=7, seed=3, keep='w')
    assert eig.betas is None and np.allclose(eig.w @ eig.Q.T, full.betas, rtol=0, atol=1e-13)
    eig_thin = run_host(f, chains=5, draws=40, burnin=7, thin=3, seed=3, keep='w')
    eig_long = run_host(f, chains=5, draws=47, burnin=0, seed=3, keep='w')
    assert np.array_equal(eig_thin.w.reshape(5, 14, -1), eig.w.reshape(5, 40, -1)[:, ::3])
    assert np.array_equal(eig_long.w.reshape(5, 47, -1)[:, 7:], eig.w.reshape(5, 40, -1))
    none = run_host(f, chains=5, draws=40, burnin=7, seed=3, keep=None)
    assert none.betas is None and none.w is None and none.sigsqd is None and none.ess is None
    assert np.array_equal(none.rhat['w'], full.rhat['w']) and 'betas' not in none.rhat
    assert np.allclose(none.chain_mean['w'] @ full.Q.T, by_chain.mean(axis=1), rtol=0, atol=1e-12)
    assert np.allclose(none.chain_mean['sigsqd'], full.sigsqd.reshape(5, 40).mean(axis=1), rtol=1e-12)
    assert np.allclose(none.chain_var['tausqd'], full.tausqd.reshape(5, 40).var(axis=1, ddof=1), rtol=1e-9)
    # chain c of a run is chain c run alone
    s = synthetic_spectrum(20)
    args = (s['lamb'], s['qty'], s['shift'], s['astar'], s['atau_star'], s['b'], s['btau'], s['dtd'])
    many = R.chains_host(*args, np.full(64, 0.16), np.full(64, 0.6), 2, 9, 1, 4)
    for c in (0, 17, 63):
        alone = R.chains_host(*args, [0.16], [0.6], 2, 9, 1, 4, chain_ids=[c])
        for key in ('w', 'sigsqd', 'tausqd', 'attempts', 'sums', 'counts'):
            assert np.array_equal(alone[key][0], many[key][c]), key


def test_sums_give_the_split_rhat_of_the_rows():
    from fokl_gpy_amd.embedded import split_rhat
    s = synthetic_spectrum(9)
    for draws in (40, 41):
        raw = R.chains_host(s['lamb'], s['qty'], s['shift'], s['astar'], s['atau_star'], s['b'], s['btau'], s['dtd'],
                            np.full(6, 0.16), np.full(6, 0.6), 3, draws, 1, 8)
        rows = np.concatenate([raw['w'], raw['sigsqd'][:, :, None], raw['tausqd'][:, :, None]], axis=2)
        assert np.allclose(R.split_rhat_from_sums(raw['sums'], draws), split_rhat(rows), rtol=1e-8)


def test_rhat_can_say_yes_and_no():
    """Yes: a well-determined model (400 rows, 18 columns) after 2 000 iterations from dispersed starts.  No: 20 iterations
    without burn-in.  Where the rows determine the model, sigma^2 forgets its start at once -- its new value looks at the old
    one only through the P + 1 normals' share of the residual, a lag-one autocorrelation of about
    (P + 1) / (2 a + 2 + n + P + 1), 0.04 on that model -- so a short run can only show its start where the columns
    outnumber the rows: the 38-column model of bern_m6 on its first 20 rows (0.56), from the default 64 chains."""
    f = load_fixture('bern_m3')
    good = run_host(f, chains=8, draws=2000, burnin=0, seed=2, init='dispersed', keep=None)
    worst = max(good.rhat['w'].max(), good.rhat['sigsqd'], good.rhat['tausqd'])
    assert worst < 1.01, worst
    assert good.sigsqd0.max() / good.sigsqd0.min() > 3          # the starts really are dispersed
    few = load_fixture('bern_m6')
    few.update(inputs=few['inputs'][:20], data=few['data'][:20])
    short = run_host(few, chains=64, draws=20, burnin=0, seed=2, init='dispersed', keep=None)
    print(f"rhat after 2 000 iterations at most {worst:.4f}; of sigsqd after 20 iterations {short.rhat['sigsqd']:.3f}")
    assert short.rhat['sigsqd'] > 1.1, short.rhat['sigsqd']
    same = run_host(f, chains=3, draws=4, burnin=0, seed=2, init='reference', keep=None)
    assert np.all(same.sigsqd0 == f['b'] / (1 + f['a'])) and np.all(same.tausqd0 == f['btau'] / (1 + f['atau']))


def test_a_negative_bstar_flags_its_chain():
    s = synthetic_spectrum(6)
    raw = R.chains_host(s['lamb'], s['qty'], s['shift'], s['astar'], s['atau_star'], -1e9, s['btau'], s['dtd'], [0.16, 0.2],
                        [0.6, 0.6], 0, 5, 1, 4)
    assert np.array_equal(raw['counts'][:, :2], [[0, R.FLAG_BSTAR_NEGATIVE]] * 2)
    assert np.isnan(raw['sigsqd']).all() and np.isnan(raw['w'][:, 1:]).all() and np.isfinite(raw['w'][:, 0]).all()
    capped = R.chains_host(s['lamb'], s['qty'], s['shift'], 1.0, 1.0, s['b'], s['btau'], s['dtd'], np.full(8, 0.16),
                           np.full(8, 0.6), 0, 60, 1, 4, attempt_cap=1)
    assert (capped['counts'][:, 1] == R.FLAG_ATTEMPT_CAP).any() and capped['counts'][:, 3].max() == 1


def test_refusals():
    f = load_fixture('bern_m3')
    with pytest.raises(ValueError, match='fitted model'):
        R.resample_host(None, f['phis'], KERNEL, f['inputs'], f['data'], 4, f['b'], 4, f['btau'])
    with pytest.raises(ValueError, match='fitted model'):
        R.resample_host(f['mtx'], f['phis'], KERNEL, f['inputs'], f['data'], 4, None, 4, f['btau'])
    with pytest.raises(ValueError, match='shapes >= 1'):
        R.resample_host(f['mtx'][:1], f['phis'], KERNEL, f['inputs'], f['data'], 4, f['b'], 0.25, f['btau'])
    wide = np.zeros((R.MAX_COLUMNS, 3), dtype=int)
    wide[:, 0] = 1
    with pytest.raises(ValueError, match=f'at most {R.MAX_COLUMNS}'):
        R.resample_host(wide, f['phis'], KERNEL, f['inputs'], f['data'], 4, f['b'], 4, f['btau'])
    for bad in (dict(chains=0), dict(draws=0), dict(thin=0), dict(burnin=-1), dict(init='wide'), dict(keep='all'),
                dict(seed=0.5)):
        with pytest.raises(ValueError):
            run_host(f, **bad)
    model = FoKLRoutines.FoKL(kernel=KERNEL, UserWarnings=False, ConsoleOutput=False)
    with pytest.raises(ValueError, match='fitted model'):
        model.resample()
    model.mtx = f['mtx']
    with pytest.raises(ValueError, match='Unexpected keyword'):
        model.resample(chain=3)
    with pytest.raises(ValueError, match='terms \\+ 1'):
        model.resample(betas=np.zeros((4, 3)))
    with pytest.raises(_capi.FoklNativeError):                  # the generator refuses a purpose it does not know
        _capi.embedded_rng(0, 0, 0, 9, 1)


def test_numpys_global_stream_is_left_alone():
    f = load_fixture('bern_m3')
    np.random.seed(99)
    before = np.random.get_state()
    run_host(f, chains=3, draws=10, burnin=2, seed=5)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]

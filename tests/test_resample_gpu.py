"""fokl_resample_chains on the device against its statement resample.chains_host, over the edges of the lane layout; its
independence of the launch shape; flagged chains; and FoKL.resample end to end behind a fit."""
import copy
import warnings

import numpy as np
import pytest

from helpers import load_case
from fokl_gpy_amd import FoKLRoutines, _capi, resample as R
from fokl_gpy_amd.embedded import basis_matrix
from test_resample_host import assert_same_distribution, synthetic_spectrum

pytestmark = pytest.mark.gpu

SEED = 11
ASTAR, ATAU_STAR = 2158.5, 22.0              # (the shapes test_accept_decisions_are_not_decided_by_the_last_bit looks at)
P1S = (1, 2, 18, 63, 64, 65, 128, 129, 300, 768)
CHAINS = (1, 3, 64, 257)
ITERATIONS = (1, 2, 257)
THINS = (1, 7)
# Device against statement, relative to each coordinate's scale.  The chain kernels' bound is 1e-12
# (tests/test_chain_device.py); measured here before anything was asserted, the largest difference over every case below
# is 2.3e-12 (tausqd at P + 1 = 768; 1.0e-12 at 300, below 7e-13 up to 129; DESIGN section 3, resample): the device's
# log / cos differ from glibc's in the last place, and bstar = b + (w'lam w - 2 w'qty + y'y + ...) / 2 cancels three sums that
# grow with P + 1 down to the residual, which lifts that last place by their ratio.  The bound is ten times the
# measurement, far below the project's draw tolerance of 1e-9.
TOL = 2.3e-11


def spectrum_args(p1):
    s = synthetic_spectrum(p1)
    return (s['lamb'], s['qty'], s['shift'], ASTAR, ATAU_STAR, s['b'], s['btau'], s['dtd'])


def starts(chains):
    """Every chain its own start (a chain read at another chain's index would show)."""
    return 0.16 * (1.0 + 0.01 * np.arange(chains)), 0.6 * (1.0 + 0.02 * np.arange(chains))


_STATEMENTS = {}


def statement(p1, iterations):
    """The statement of all 257 chains (chain c is the same whatever the number of chains: test_resample_host)."""
    key = (p1, iterations)
    if key not in _STATEMENTS:
        sig0, tau0 = starts(max(CHAINS))
        _STATEMENTS[key] = R.chains_host(*spectrum_args(p1), sig0, tau0, 0, iterations, 1, SEED)
    return _STATEMENTS[key]


def compare(dev, host, chains, iterations, thin, rows, worst):
    """Attempt counts equal; values within TOL of the coordinate's scale.  A chain whose attempts part from the statement's
    is compared up to that row only -> the number of chains cut short."""
    cut_short = 0
    w_scale = np.max(np.abs(host['w'][:chains]), axis=(0, 1))
    p1 = w_scale.shape[0]
    scale = np.concatenate([w_scale, [np.max(host['sigsqd'][:chains]), np.max(host['tausqd'][:chains])]])
    whole = np.ones(chains, dtype=bool)
    if rows:
        expect_att = host['attempts'][:chains, ::thin]
        assert dev['w'].shape == (chains, expect_att.shape[1], p1)
        for c in range(chains):
            same = dev['attempts'][c] == expect_att[c]
            upto = expect_att.shape[1] if same.all() else int(np.argmin(same))
            if upto < expect_att.shape[1]:
                cut_short += 1
                whole[c] = False
            for name, sc in (('w', w_scale), ('sigsqd', scale[p1]), ('tausqd', scale[p1 + 1])):
                gap = np.abs(dev[name][c, :upto] - host[name][c, ::thin][:upto]) / sc
                if gap.size:
                    worst[0] = max(worst[0], float(gap.max()))
                    assert gap.max() <= TOL, (name, c, float(gap.max()))
    else:
        assert dev['w'] is None and dev['sigsqd'] is None and dev['attempts'] is None
        whole = np.all(dev['counts'][:, 2:] == host['counts'][:chains, 2:], axis=1)
        cut_short = int((~whole).sum())
    assert np.array_equal(dev['counts'][whole], host['counts'][:chains][whole])
    for power in (0, 1):
        gap = np.abs(dev['sums'][whole, :, power] - host['sums'][:chains][whole, :, power]) / (iterations * scale ** (power + 1))
        if gap.size:
            worst[0] = max(worst[0], float(gap.max()))
            assert gap.max() <= TOL, ('sums', power, float(gap.max()))
    return cut_short


@pytest.mark.parametrize('p1', P1S)
def test_kernel_against_the_statement(device_ctx, p1):
    args = spectrum_args(p1)
    worst, cut_short, compared = [0.0], 0, 0
    for iterations in ITERATIONS:
        host = statement(p1, iterations)
        for chains in CHAINS:
            sig0, tau0 = starts(chains)
            for thin in THINS:
                for rows in (True, False):
                    dev = device_ctx.resample_chains(*args, sig0, tau0, 0, iterations, thin, SEED, rows=rows)
                    cut_short += compare(dev, host, chains, iterations, thin, rows, worst)
                    compared += chains
                    rep = device_ctx.resample_report()
                    assert rep['chains'] == chains and rep['iterations'] == iterations and rep['instance'] * 64 >= p1
                    assert rep['kept'] == -(-iterations // thin) and rep['attempts'] == int(dev['counts'][:, 2].sum())
    print(f"P + 1 = {p1}: largest device - statement difference {worst[0]:.3e} of the scale; {cut_short} of {compared} "
          f"chains cut short by an attempt count")
    assert cut_short <= compared // 100


def test_burn_in_and_thinning_on_the_device(device_ctx):
    args = spectrum_args(65)
    sig0, tau0 = starts(5)
    host = R.chains_host(*args, sig0, tau0, 5, 23, 7, SEED)
    dev = device_ctx.resample_chains(*args, sig0, tau0, 5, 23, 7, SEED)
    assert dev['w'].shape == (5, 4, 65) and np.array_equal(dev['attempts'], host['attempts'])
    assert np.array_equal(dev['counts'], host['counts'])
    assert np.max(np.abs(dev['w'] - host['w']) / np.max(np.abs(host['w']), axis=(0, 1))) <= TOL
    assert np.max(np.abs(dev['sums'] - host['sums']) / np.maximum(np.abs(host['sums']), 1.0)) <= 23 * TOL


def test_results_do_not_depend_on_the_launch_shape(device_ctx):
    for p1 in (18, 300):
        args = spectrum_args(p1)
        sig0, tau0 = starts(13)
        base = device_ctx.resample_chains(*args, sig0, tau0, 3, 50, 2, SEED)
        assert device_ctx.resample_report()['chains_per_group'] == 4
        for per_group in (1, 2, 3):
            other = device_ctx.resample_chains(*args, sig0, tau0, 3, 50, 2, SEED, chains_per_group=per_group)
            rep = device_ctx.resample_report()
            assert rep['chains_per_group'] == per_group and rep['grid'] == -(-13 // per_group)
            for key in base:
                assert np.array_equal(base[key], other[key]), (p1, per_group, key)


def test_a_flagged_chain_is_nan_from_there_on_and_alone(device_ctx):
    """bstar < 0 through a negative b.  b belongs to the launch, so who is flagged when is steered by the starts: a chain
    that starts at tausqd = 1e-12 draws w ~ 0, sees the whole of y'y in bstar and passes iteration 0; the others do not."""
    s = synthetic_spectrum(18)
    sse = 4000 * 0.04
    args = (s['lamb'], s['qty'], s['shift'], ASTAR, ATAU_STAR, -1.5 * sse, s['btau'], s['dtd'])
    sig0, tau0 = np.full(6, 0.16), np.full(6, 1e-12)
    tau0[2] = 0.6
    dev = device_ctx.resample_chains(*args, sig0, tau0, 0, 4, 1, SEED)
    host = R.chains_host(*args, sig0, tau0, 0, 4, 1, SEED)
    assert np.array_equal(dev['counts'], host['counts'])
    assert dev['counts'][2, 0] == 0 and np.all(dev['counts'][[0, 1, 3, 4, 5], 0] == 1)
    assert np.all(dev['counts'][:, 1] == R.FLAG_BSTAR_NEGATIVE)
    assert np.isnan(dev['sigsqd'][2]).all() and np.isnan(dev['w'][2, 1:]).all() and np.isfinite(dev['w'][2, 0]).all()
    assert np.isfinite(dev['w'][[0, 1, 3], :1]).all() and np.isfinite(dev['sigsqd'][[0, 1, 3], 0]).all()
    assert np.array_equal(np.isnan(dev['w']), np.isnan(host['w'])) and np.array_equal(np.isnan(dev['sums']), np.isnan(host['sums']))
    # the other chains of the launch are untouched by chain 2's flag: the same launch with chain 2 started like them
    tau0[2] = 1e-12
    twin = device_ctx.resample_chains(*args, sig0, tau0, 0, 4, 1, SEED)
    for key in ('w', 'sigsqd', 'tausqd', 'attempts', 'sums', 'counts'):
        assert np.array_equal(twin[key][[0, 1, 3, 4, 5]], dev[key][[0, 1, 3, 4, 5]], equal_nan=True), key
    assert device_ctx.resample_report()['flagged'] == 6


def test_the_attempt_cap_flags_and_does_not_hang(device_ctx):
    s = synthetic_spectrum(18)
    args = (s['lamb'], s['qty'], s['shift'], 1.0, 1.0, s['b'], s['btau'], s['dtd'])
    sig0, tau0 = starts(64)
    dev = device_ctx.resample_chains(*args, sig0, tau0, 0, 60, 1, SEED, attempt_cap=1)
    host = R.chains_host(*args, sig0, tau0, 0, 60, 1, SEED, attempt_cap=1)
    assert np.array_equal(dev['counts'], host['counts']) and np.array_equal(dev['attempts'], host['attempts'])
    assert (dev['counts'][:, 1] == R.FLAG_ATTEMPT_CAP).any() and dev['counts'][:, 3].max() == 1
    assert np.array_equal(np.isnan(dev['sigsqd']), np.isnan(host['sigsqd']))
    assert device_ctx.resample_report()['attempts_max'] == 1


def test_native_refusals_name_the_limit(device_ctx):
    s = synthetic_spectrum(18)
    args = (s['lamb'], s['qty'], s['shift'], ASTAR, ATAU_STAR, s['b'], s['btau'], s['dtd'])
    with pytest.raises(_capi.FoklNativeError, match='shapes >= 1'):
        device_ctx.resample_chains(s['lamb'], s['qty'], s['shift'], ASTAR, 0.5, s['b'], s['btau'], s['dtd'], [0.1], [0.1], 0, 2, 1, 0)
    wide = synthetic_spectrum(769)
    with pytest.raises(_capi.FoklNativeError, match='at most 768'):
        device_ctx.resample_chains(wide['lamb'], wide['qty'], wide['shift'], ASTAR, ATAU_STAR, 0.8, 3.0, wide['dtd'], [0.1],
                                   [0.1], 0, 2, 1, 0)
    with pytest.raises(_capi.FoklNativeError, match='chains per workgroup'):
        device_ctx.resample_chains(*args, [0.1], [0.1], 0, 2, 1, 0, chains_per_group=5)
    assert device_ctx.resample_report()['instance'] == 0
    # rows beyond the device's free memory: 4 096 chains x 2^30 rows x 18 x 8 bytes; nothing that size is allocated here
    lib, h = device_ctx._lib, device_ctx._h
    sig0 = np.full(4096, 0.1)
    out = np.empty(8)
    rc = lib.fokl_resample_chains(h, 18, _capi._ptr(s['lamb']), _capi._ptr(s['qty']), _capi._ptr(s['shift']), ASTAR, ATAU_STAR,
                                  0.8, 3.0, s['dtd'], 4096, _capi._ptr(sig0), _capi._ptr(sig0), 0, 1 << 30, 1, 0, 0, 0,
                                  _capi._ptr(out), _capi._ptr(out), _capi._ptr(out), _capi._ptr(out), _capi._ptr(out),
                                  _capi._ptr(out))
    assert rc != 0 and b'free' in lib.fokl_last_error(h)


def snapshot(value):
    try:
        return copy.deepcopy(value)
    except Exception:
        return value                                     # (handles: compared by identity)


def unchanged(now, before):
    """Equality through nested lists / dicts of arrays, NaN equal to NaN."""
    if now is before or (not isinstance(before, np.ndarray) and repr(now) == repr(before)):
        return True
    if isinstance(before, dict):
        return isinstance(now, dict) and set(now) == set(before) and all(unchanged(now[k], before[k]) for k in before)
    if isinstance(before, (list, tuple)):
        return type(now) is type(before) and len(now) == len(before) and all(unchanged(a, b) for a, b in zip(now, before))
    if isinstance(before, (np.ndarray, float, np.floating)):
        try:
            return bool(np.array_equal(now, before, equal_nan=True))
        except TypeError:
            return bool(np.array_equal(now, before))
    return bool(now == before)


def test_resample_behind_a_fit(device_ctx):
    g, hy, kname, kid, phis = load_case('bern_m8_capped')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = FoKLRoutines.FoKL(kernel=kname, phis=phis, UserWarnings=False, ConsoleOutput=False, **hy)
        np.random.seed(int(g['seed']))
        betas, mtx, evs = model.fit(g['raw_inputs'], g['raw_data'], clean=True)
        mean_fit = model.evaluate()
        mean_fit = mean_fit[0] if isinstance(mean_fit, tuple) else mean_fit
        pop_fit = model.propagate()

        state = np.random.get_state()
        kept = {k: snapshot(v) for k, v in model.__dict__.items() if k != 'inputs'}
        res = model.resample(chains=64, draws=2000)
        after = np.random.get_state()
        assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        assert set(kept) == set(model.__dict__) - {'inputs'}
        for k, v in kept.items():
            assert unchanged(model.__dict__[k], v), k

        p1 = mtx.shape[0] + 1
        assert res.betas.shape == (64 * 2000, p1) and res.sigsqd.shape == (128000,) and not res.flagged.any()
        assert np.array_equal(res.chain, np.repeat(np.arange(64), 2000))
        rep = FoKLRoutines.device_backend().ctx.resample_report()
        assert rep['instance'] == -(-p1 // 64) and rep['chains'] == 64 and rep['iterations'] == 2500
        assert rep['chains_per_group'] == 4 and rep['grid'] == 16 and rep['kernel_ms'] > 0 and rep['flagged'] == 0
        worst = max(res.rhat['w'].max(), res.rhat['betas'].max(), res.rhat['sigsqd'], res.rhat['tausqd'])
        print(f"64 x 2 500 iterations in {rep['kernel_ms']:.2f} ms of kernel; rhat at most {worst:.4f}; ESS of sigsqd "
              f"{res.ess['sigsqd']:.0f}; {rep['attempts']} attempts, at most {rep['attempts_max']}")
        assert worst < 1.01
        assert_same_distribution(res.betas, 64, np.asarray(betas), 'fit against resample')

        # the consumers take the rows: evaluate and propagate on the device
        twin = copy.copy(model)
        twin.setnos = None
        out = twin.evaluate(betas=res.betas, draws=res.betas.shape[0], ReturnBounds=True)
        mean_res, bounds = out[0], out[1]
        rows = slice(0, 40)
        X = basis_matrix(np.asarray(model.inputs)[rows], mtx, phis, kname)
        assert np.max(np.abs(mean_res[rows] - (res.betas @ X.T).mean(axis=0))) < 1e-9
        assert np.all(bounds[:, 0] <= mean_res) and np.all(mean_res <= bounds[:, 1])
        assert np.max(np.abs(mean_fit[rows] - (np.asarray(betas) @ X.T).mean(axis=0))) < 1e-9
        assert_same_distribution(res.betas @ X.T, 64, np.asarray(betas) @ X.T, 'evaluate', variances=False)
        pop_res = model.propagate(betas=res.betas)
        assert pop_res.mean.shape == (128000,)
        assert_same_distribution(pop_res.mean[:, None], 64, pop_fit.mean[:, None], 'propagate', variances=False)
        for keep in ('w', None):
            again = model.resample(chains=64, draws=2000, keep=keep)
            assert np.array_equal(again.sums, res.sums)
            if keep == 'w':
                assert np.allclose(again.w @ again.Q.T, res.betas, rtol=0, atol=1e-12) and again.betas is None

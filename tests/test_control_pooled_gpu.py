"""dynamics.control_pooled on the MI355X against its statement dynamics.control_pooled_host (pinned without a device by
tests/test_control_pooled_host.py): the first pass -- the draws' own parts and the pooled F, g, H -- bit for bit across the
chunk seams of the pooled sum, whole solves with equal status, iterations and best start, u within 1e-9 of the box width
and the costs within 1e-9 relative (the package's customary 1e-9, as tests/test_control_gpu.py), and the returned
trajectories as simulate_host's under the returned controls, bit for bit."""
import warnings

import numpy as np
import pytest

from control_cases import chain, linear, mixed, product
from fokl_gpy_amd import FoKLRoutines, dynamics, optimize

pytestmark = pytest.mark.gpu

NONLINEAR = dict(segments=4, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3})


def _weights(E, seed=3):
    """Non-uniform, with one zero where there is more than one draw."""
    w = 0.25 + np.random.default_rng(seed).random(E)
    if E > 1:
        w[E // 2] = 0.0
    return w


def _system(args):
    return {key: value for key, value in args.items() if key != 'controls'}


def _same_first_pass(dev, host):
    for key in ('F_draws', 'g_draws', 'H_draws', 'F', 'g', 'H'):
        differ = ~((dev[key] == host[key]) | (np.isnan(dev[key]) & np.isnan(host[key])))
        if differ.any():
            at = tuple(np.argwhere(differ)[0])
            print(f"\nfirst pass {key}: {int(differ.sum())} of {differ.size} values differ, first at {at}: device "
                  f"{dev[key][at]!r} host {host[key][at]!r}")
        assert dev[key].shape == host[key].shape and not differ.any(), key


def _compare(ctx, args, width, **kw):
    """control_pooled against control_pooled_host: whole solves -> (device, host)."""
    host = dynamics.control_pooled_host(**args, **kw, keep=['members', 'all'])
    dev = dynamics.control_pooled(**args, **kw, keep=['members', 'all'], device=ctx)
    width = np.asarray(width, dtype=np.float64)[:, np.newaxis]
    finite = np.isfinite(host.cost_draws)
    print(f"\nstatus {dev.status_all.tolist()} iterations {dev.iterations_all.tolist()} max |u - u_host| / width "
          f"{np.max(np.abs(dev.u_all - host.u_all) / width):.2e} max relative cost difference "
          f"{np.max(np.abs(dev.cost_all - host.cost_all) / np.abs(host.cost_all)):.2e}")
    assert np.array_equal(dev.status_all, host.status_all) and np.array_equal(dev.iterations_all, host.iterations_all)
    assert dev.best_start == host.best_start and np.array_equal(dev.descent_steps_all, host.descent_steps_all)
    assert dev.status == host.status and dev.iterations == host.iterations
    assert np.all(np.abs(dev.u_all - host.u_all) <= 1e-9 * width)
    assert np.all(np.abs(dev.cost_all - host.cost_all) <= 1e-9 * np.abs(host.cost_all))
    assert abs(dev.cost_start - host.cost_start) <= 1e-9 * abs(host.cost_start)
    assert np.array_equal(np.isfinite(dev.cost_draws), finite)
    assert np.all(np.abs(dev.cost_draws[finite] - host.cost_draws[finite]) <= 1e-9 * np.abs(host.cost_draws[finite]))
    assert np.array_equal(dev.u, dev.u_all[dev.best_start]) and dev.cost == dev.cost_all[dev.best_start]
    assert dev.cost == dynamics.pooled_sum(dev.cost_draws, dev.draw_weights)
    # every draw's trajectory under the SHARED controls is simulate_host's, bit for bit
    again = dynamics.simulate_host(**{**_system(args), 'forcing': {**(args.get('forcing') or {}), **dynamics.expand_controls(dev)}},
                                   ReturnBounds=False, keep='members')
    assert np.array_equal(again.members, dev.members, equal_nan=True)
    assert np.array_equal(again.first_saturation, dev.first_saturation)
    return dev, host


# ---------------------------------------------------------------------------------------------------------
# 1. the first pass across the chunk seams, bit for bit
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('case', ['chain', 'mixed'])
def test_first_pass_bit_for_bit_across_the_chunk_seams(device_ctx, case, E):
    if case == 'chain':
        args, kw = chain(1, E, 10), dict(targets={'x0': 0.1}, move_weight={'u': 1e-3})
    else:
        args, kw = mixed(E, 20), dict(targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01})
    kw.update(segments=4, starts=2, draw_weights=_weights(E), max_iter=0)
    dev = dynamics.control_pooled(**args, **kw, device=device_ctx)
    host = dynamics.control_pooled_host(**args, **kw)
    _same_first_pass(dev.first_pass, host.first_pass)
    assert np.isfinite(host.first_pass['F']).all() and np.any(host.first_pass['g'] != 0)
    assert np.isnan(dev.first_pass['F_draws']).sum() == (2 if E > 1 else 0)
    assert dev.cost_start == host.cost_start and dev.status == host.status == optimize.ITERATION_LIMIT
    rep = device_ctx.control_pooled_report()
    assert rep['draws'] == E and rep['starts'] == 2 and rep['D'] == 4 and rep['chunks'] == -(-E // 64)
    assert rep['iterations_queued'] == 1 and rep['iterations_with_work'] == 1 and rep['NS'] == len(args['states'])


# ---------------------------------------------------------------------------------------------------------
# 2. - 5. whole solves
# ---------------------------------------------------------------------------------------------------------

def test_whole_solves_mixed_kernels_over_a_chunk_seam(device_ctx):
    dev, _ = _compare(device_ctx, mixed(65, 20), [10.0], segments=4, targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01},
                      starts=2, draw_weights=_weights(65))
    assert dev.iterations > 0 and dev.status != optimize.NON_FINITE
    assert dev.members.shape == (65, 2, 21) and dev.bounds.shape == (2, 21, 2)


def test_whole_solves_product_terms(device_ctx):
    dev, host = _compare(device_ctx, product(9, 20, spread=0.3), [4.0], **NONLINEAR, starts=2)
    assert dev.status == optimize.CONVERGED and dev.cost <= dev.cost_start
    assert dev.bounds.shape == (2, 21, 2) and dev.violation_share.tolist() == [0.0, 0.0]


def test_eight_states(device_ctx):
    args = chain(8, 3, 10)
    want = dynamics.simulate_host(**_system(args), forcing={'u': np.repeat([3.0, 7.0], 5)}, draws=np.array([0]), ReturnBounds=False,
                                  keep='members').members[0]
    dev, _ = _compare(device_ctx, args, [10.0], segments=2, targets={'x0': want[0], 'x7': want[7] + 0.001}, draw_weights=[1.0, 0.5, 2.0])
    assert device_ctx.control_pooled_report()['NS'] == 8 and dev.status != optimize.NON_FINITE


def test_thirty_two_decision_values_across_a_chunk_seam(device_ctx):
    dev, _ = _compare(device_ctx, linear(65, 16, 2, spread=0.05), [2.0, 2.0], segments=16, targets={'x0': 0.5, 'x1': -0.2},
                      move_weight={'u0': 0.01, 'u1': 0.01}, previous=[0.0, 0.1], draw_weights=_weights(65))
    rep = device_ctx.control_pooled_report()
    assert rep['D'] == 32 and rep['chunks'] == 2 and rep['step_lds_bytes'] == 36 * 64 * 8 and dev.u.shape == (2, 16)


def test_soft_limits_and_starts_that_stop_at_different_iterations(device_ctx):
    args = {**product(5, 16, spread=0.3), 'y0': np.array([[0.4, -0.3], [-0.5, 0.5], [0.7, -0.4], [0.2, 0.1], [0.5, -0.2]])}
    dev, _ = _compare(device_ctx, args, [4.0], **NONLINEAR, limits={'x0': (None, 0.6), 'x1': (-0.5, None)}, limit_weight=1e3,
                      starts=3, draw_weights=[1.0, 2.0, 0.5, 1.5, 1.0])
    assert len(set(dev.iterations_all.tolist())) > 1 and np.all(dev.status_all != optimize.NON_FINITE)
    assert dev.violated.shape == (5, 2) and dev.violated.any()
    rep = device_ctx.control_pooled_report()
    assert rep['iterations_with_work'] == int(dev.iterations_all.max()) + 1 and rep['launches_per_iteration'] == 6


# ---------------------------------------------------------------------------------------------------------
# 6. - 8. invariances, bit for bit
# ---------------------------------------------------------------------------------------------------------

KEYS = ('u_all', 'cost_all', 'status_all', 'iterations_all', 'descent_steps_all', 'members', 'cost_draws', 'cost_start', 'first_saturation')


def test_one_draw_is_the_devices_own_control(device_ctx):
    args = mixed(1, 20)
    kw = dict(segments=4, targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01}, starts=3, keep=['members', 'all'])
    pooled = dynamics.control_pooled(**args, **kw, device=device_ctx)
    own = dynamics.control(**args, **kw, device=device_ctx)
    for key in ('u_all', 'cost_all', 'status_all', 'iterations_all', 'descent_steps_all', 'u', 'z', 'cost', 'cost_start', 'status',
                'iterations', 'best_start'):
        assert np.array_equal(pooled[key], own[key][0]), key
    assert np.array_equal(pooled.members, own.members) and pooled.iterations > 0
    assert pooled.cost_draws[0] == pooled.cost


def test_a_zero_weight_nan_draw_changes_no_bit(device_ctx):
    args = product(6, 20, spread=0.3)
    w = np.array([0.2, 1.0, 0.0, 0.7, 0.4, 1.3])
    kw = dict(**NONLINEAR, starts=2, keep=['members', 'all'])
    res = dynamics.control_pooled(**args, **kw, draw_weights=w, device=device_ctx)
    extra = {**args, 'models': [dict(m, betas=np.concatenate([m['betas'], np.full((1, m['betas'].shape[1]), np.nan)]))
                                for m in args['models']]}
    quiet = dynamics.control_pooled(**extra, **kw, draw_weights=np.append(w, 0.0), device=device_ctx)
    for key in ('u', 'cost', 'iterations', 'u_all', 'cost_all', 'iterations_all', 'status_all', 'mean'):
        assert np.array_equal(quiet[key], res[key]), key
    assert res.iterations > 1 and np.array_equal(quiet.cost_draws[:6], res.cost_draws) and np.isnan(quiet.cost_draws[6])
    assert np.array_equal(quiet.members[:6], res.members) and np.isnan(quiet.members[6, :, 1:]).all()
    loud = dynamics.control_pooled(**extra, **kw, draw_weights=np.append(w, 0.1), device=device_ctx)
    assert loud.status == optimize.NON_FINITE and loud.iterations == 0


def test_the_early_stop_read_and_a_repeated_call_change_nothing(device_ctx, monkeypatch):
    args = product(9, 20, spread=0.3)
    kw = dict(**NONLINEAR, starts=3, keep=['members', 'all'], draw_weights=_weights(9))
    runs, reports = [], []
    for poll in ('0', '1', '1'):
        monkeypatch.setenv('FOKL_CONTROL_POLL', poll)
        runs.append(dynamics.control_pooled(**args, **kw, device=device_ctx))
        reports.append(device_ctx.control_pooled_report())
    for other in runs[1:]:
        for key in KEYS:
            assert np.array_equal(runs[0][key], other[key]), key
    most = int(runs[0].iterations_all.max())
    assert 0 < most < 60 and reports[0]['iterations_queued'] == 61 and reports[1]['iterations_queued'] == most + 1
    assert all(rep['iterations_with_work'] == most + 1 for rep in reports)


# ---------------------------------------------------------------------------------------------------------
# 9. native refusals
# ---------------------------------------------------------------------------------------------------------

def _native(ctx, **change):
    args = mixed(3, 7)
    p = dynamics._prepare_control_pooled(args['models'], args['states'], args['inputs'], args['controls'], args['forcing'],
                                         args['y0'], args['t'], None, None, 3, None, {'T': 0.2}, None, None, None, 1e3,
                                         {'u': 0.01}, None, None, 2, 60, 1e-10, None, None)
    p.update(change)
    return ctx.control_pooled_solve(p)


def test_native_refusals(device_ctx, monkeypatch):
    from fokl_gpy_amd._capi import FoklNativeError
    _native(device_ctx)
    rep = device_ctx.control_pooled_report()
    assert rep['draws'] == 3 and rep['starts'] == 2 and rep['launches_per_iteration'] == 6 and rep['chunks'] == 1
    assert 1 <= rep['iterations_with_work'] <= rep['iterations_queued']
    assert rep['lds_bytes'] == dynamics._prepare_control_pooled(
        *(mixed(3, 7)[k] for k in ('models', 'states', 'inputs', 'controls', 'forcing', 'y0', 't')), None, None, 3, None,
        {'T': 0.2}, None, None, None, 1e3, {'u': 0.01}, None, None, 2, 60, 1e-10, None, None)['lds_bytes']
    cases = {
        "draw weights must be non-negative and finite": dict(pool_w=np.array([0.5, -0.5, 1.0])),
        "draw weights must be non-negative and finite ": dict(pool_w=np.array([0.5, np.nan, 0.5])),
        "draw weights must be non-negative and finite  ": dict(pool_w=np.array([0.5, np.inf, 0.5])),
        "draw weights sum to zero": dict(pool_w=np.zeros(3)),
        "a start lies outside the box": dict(z0=np.array([[0.5, 1.5, 0.5], [0.5, 0.5, 0.5]])),      # inherited from fokl_control_solve
        "negative weights": dict(wt=np.array([-1.0, 0.0])),
    }
    for text, change in cases.items():
        with pytest.raises(FoklNativeError, match=text.strip()):
            _native(device_ctx, **change)
        assert set(device_ctx.control_pooled_report().values()) == {0}, text
    # the workspace: 3 draws x 2 starts x (2 + 3 + 9 + 64) x 8 bytes and as much per (start, chunk) = 4 992 bytes
    monkeypatch.setenv('FOKL_CONTROL_POOLED_FREE_BYTES', '4991')
    with pytest.raises(FoklNativeError, match=r"workspace needs 4992 bytes .*FOKL_CONTROL_POOLED_FREE_BYTES"):
        _native(device_ctx)
    assert set(device_ctx.control_pooled_report().values()) == {0}
    monkeypatch.setenv('FOKL_CONTROL_POOLED_FREE_BYTES', '4992')
    _native(device_ctx)                                                # the context is as good as before
    assert device_ctx.control_pooled_report()['draws'] == 3


# ---------------------------------------------------------------------------------------------------------
# 10. end to end
# ---------------------------------------------------------------------------------------------------------

def test_fit_resample_assimilate_control_pooled_simulate(device_ctx):
    """Two small fits, ``resample``, ``assimilate`` against a few measurements, ``control_pooled`` with the re-weighted
    posterior, then ``simulate`` under the one sequence."""
    rng = np.random.default_rng(8)
    n = 300
    T, c, u = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 2.0, n)
    rates = [-0.8 * T + 0.5 * c + 0.9 * (u - 1.0) + 0.01 * rng.standard_normal(n), 0.4 * T - 0.6 * c + 0.01 * rng.standard_normal(n)]
    models = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for k, (inputs, rate) in enumerate(zip(([T, c, u], [T, c]), rates)):
            fit = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', burnin=60, draws=60, tolerance=2, UserWarnings=False,
                                    ConsoleOutput=False)
            np.random.seed(3 + k)
            fit.fit(np.stack(inputs, axis=1), rate, clean=True)
            post = fit.resample(chains=2, draws=4, burnin=20, seed=5 + k)
            models.append(dict(betas=post.betas, mtx=fit.mtx, phis=fit.phis, minmax=fit.minmax, kernel=fit.kernel))
    system = dict(models=models, states=['T', 'c'], inputs=[['T', 'c', 'u'], ['T', 'c']], y0=[0.5, -0.3])
    past = dict(system, t=(0.0, 7.5 * 0.1, 0.1), forcing={'u': np.full(8, 1.2)})
    truth = dynamics.simulate_host(**past, draws=np.array([2]), ReturnBounds=False, keep='members').members[0]
    est = dynamics.assimilate(**past, observe=['T'], data=truth[:1, [4, 8]].T, obs_points=np.array([4, 8]), obs_sd=[0.01],
                              process_sd=0.0, device=device_ctx)
    assert est.weights.shape == (8,) and abs(est.weights.sum() - 1.0) < 1e-12
    args = dict(system, controls=['u'], y0=est.draw_mean[:, :, -1], t=(0.0, 15.5 * 0.1, 0.1))
    kw = dict(segments=4, targets={'T': 0.0}, terminal={'T': 1.0}, move_weight={'u': 0.01}, previous=[1.2], draw_weights=est.weights)
    dev, host = _compare(device_ctx, args, [models[0]['minmax'][2][1] - models[0]['minmax'][2][0]], **kw)
    assert dev.u.shape == (1, 4) and dev.cost <= dev.cost_start and dev.status != optimize.NON_FINITE
    spread = dynamics.simulate(**{**system, 'y0': est.draw_mean[:, :, -1]}, t=args['t'], forcing=dynamics.expand_controls(dev),
                               keep='members', device=device_ctx)
    assert np.array_equal(spread.members, dev.members)
    assert abs(dev.mean[0, -1]) < 0.5                                  # the one sequence steers the posterior towards the target

"""dynamics.control_cvar on the MI355X against its statement dynamics.control_cvar_host (pinned without a device by
tests/test_control_cvar_host.py): the first pass -- a, phi, the soft tail weights q, the band weights c, g, H with the
covariance term and the draws' own parts -- bit for bit across the chunk seams of the pooled sum, whole solves with equal
status and iterations, u within 1e-9 of the box width and cost and cvar within 1e-9 relative (the gates of
tests/test_control_pooled_gpu.py), alpha = 0 as the device's own control_pooled, the status poll, the native refusals and
the report."""
import numpy as np
import pytest

from control_cases import mixed, product
from fokl_gpy_amd import dynamics, optimize

pytestmark = pytest.mark.gpu

# start 0 away from the box centre: with one control the first further start IS the centre
PRODUCT = dict(segments=4, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3}, init=np.array([[1.0, 2.5, 0.5, 3.0]]))
MIXED = dict(segments=4, targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01}, init=np.array([[2.0, 6.0, 4.0, 8.0]]))


def _weights(E, seed=3):
    """Non-uniform, with one zero where there is more than one draw."""
    w = 0.25 + np.random.default_rng(seed).random(E)
    if E > 1:
        w[E // 2] = 0.0
    return w


def _case(case, E):
    return (product(E, 20, spread=0.3), dict(PRODUCT)) if case == 'product' else (mixed(E, 20, spread=0.3), dict(MIXED))


def _with_nan_draws(args, at):
    """Draws `at` as a collapsed draw reaches the solver: every cost of theirs is NaN.  (A NaN in ``y0`` itself is refused by
    the shared preparation before any solver sees it, so the NaN sits in the draws' coefficients, as in
    tests/test_control_pooled_gpu.py.)"""
    models = []
    for m in args['models']:
        betas = np.array(m['betas'], dtype=np.float64)
        betas[at] = np.nan
        models.append(dict(m, betas=betas))
    return {**args, 'models': models}


def _same_first_pass(dev, host):
    assert set(dev) == set(host)
    for key in ('F_draws', 'g_draws', 'H_draws', 'a', 'phi', 'q', 'c', 'g', 'H'):
        differ = ~((dev[key] == host[key]) | (np.isnan(dev[key]) & np.isnan(host[key])))
        if differ.any():
            at = tuple(np.argwhere(differ)[0])
            print(f"\nfirst pass {key}: {int(differ.sum())} of {differ.size} values differ, first at {at}: device "
                  f"{dev[key][at]!r} host {host[key][at]!r}")
        assert dev[key].shape == host[key].shape and not differ.any(), key


# ---------------------------------------------------------------------------------------------------------
# 1. the first pass across the chunk seams, bit for bit
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('case', ['product', 'mixed'])
def test_first_pass_bit_for_bit_across_the_chunk_seams(device_ctx, case, E):
    args, kw = _case(case, E)
    # epsilon: wide enough next to the spread of the draws' costs at the start that several draws sit inside the band (c != 0)
    kw.update(starts=2, draw_weights=_weights(E), max_iter=0, alpha=0.8, epsilon=2e-3 if case == 'product' else 5e-4)
    dev = dynamics.control_cvar(**args, **kw, device=device_ctx)
    host = dynamics.control_cvar_host(**args, **kw)
    _same_first_pass(dev.first_pass, host.first_pass)
    first = host.first_pass
    assert np.isfinite(first['phi']).all() and np.any(first['g'] != 0) and first['q'].shape == (2, E)
    if E > 1:
        assert np.any(first['c'] != 0) and np.all(first['q'][:, E // 2] == 0) and np.isnan(dev.first_pass['F_draws']).sum() == 2
        assert np.all(np.abs(first['q'].sum(axis=1) - 1.0) < 1e-12)
    assert dev.cost_start == host.cost_start and dev.cost == host.cost and dev.status == host.status == optimize.ITERATION_LIMIT
    assert dev.epsilon == host.epsilon == kw['epsilon']
    for key in ('cvar', 'var', 'expected_cost', 'a'):
        assert dev[key] == host[key], key
    assert np.array_equal(dev.tail_weights, host.tail_weights) and np.array_equal(dev.cost_draws, host.cost_draws, equal_nan=True)
    rep = device_ctx.control_cvar_report()
    assert rep['draws'] == E and rep['starts'] == 2 and rep['D'] == 4 and rep['chunks'] == -(-E // 64)
    assert rep['iterations_queued'] == 1 and rep['iterations_with_work'] == 1 and rep['NS'] == 2


def test_first_pass_with_weight_zero_draws_in_front_of_nan(device_ctx):
    E = 65
    args, kw = _case('product', E)
    w = _weights(E)
    w[[0, 64]] = 0.0
    args = _with_nan_draws(args, [0, 64])
    kw.update(starts=2, draw_weights=w, max_iter=0, alpha=0.8, epsilon=2e-3)
    dev = dynamics.control_cvar(**args, **kw, device=device_ctx)
    host = dynamics.control_cvar_host(**args, **kw)
    _same_first_pass(dev.first_pass, host.first_pass)
    assert np.isfinite(dev.first_pass['phi']).all() and np.isfinite(dev.first_pass['H']).all()
    assert np.all(dev.first_pass['q'][:, [0, 64]] == 0) and np.isnan(dev.cost_draws[[0, 64]]).all()
    assert dev.cvar == host.cvar and np.isfinite(dev.cvar)
    # the same draw with a weight: phi is NaN, the solve ends non-finite, on the device as in the statement
    w[64] = 0.5
    kw.update(draw_weights=w)
    dev, host = dynamics.control_cvar(**args, **kw, device=device_ctx), dynamics.control_cvar_host(**args, **kw)
    _same_first_pass(dev.first_pass, host.first_pass)
    assert np.isnan(dev.first_pass['phi']).all() and dev.status == host.status == optimize.NON_FINITE


def test_relative_smoothing_takes_the_start_cost_in_the_pooled_order(device_ctx):
    args, kw = _case('mixed', 130)
    kw.update(starts=2, draw_weights=_weights(130), max_iter=0, alpha=0.9, smoothing=0.05)
    dev, host = dynamics.control_cvar(**args, **kw, device=device_ctx), dynamics.control_cvar_host(**args, **kw)
    pooled = dynamics.control_pooled_host(**args, **{k: v for k, v in kw.items() if k not in ('alpha', 'smoothing')})
    assert dev.epsilon == host.epsilon == 0.05 * pooled.first_pass['F'][0]
    _same_first_pass(dev.first_pass, host.first_pass)


# ---------------------------------------------------------------------------------------------------------
# 2. whole solves
# ---------------------------------------------------------------------------------------------------------

def _compare(ctx, args, width, **kw):
    host = dynamics.control_cvar_host(**args, **kw, keep=['members', 'all'])
    dev = dynamics.control_cvar(**args, **kw, keep=['members', 'all'], device=ctx)
    width = np.asarray(width, dtype=np.float64)[:, np.newaxis]
    print(f"\nstatus {dev.status_all.tolist()} iterations {dev.iterations_all.tolist()} max |u - u_host| / width "
          f"{np.max(np.abs(dev.u_all - host.u_all) / width):.2e} max relative cost difference "
          f"{np.max(np.abs(dev.cost_all - host.cost_all) / np.abs(host.cost_all)):.2e} cvar {dev.cvar!r} host {host.cvar!r}")
    assert np.array_equal(dev.status_all, host.status_all) and np.array_equal(dev.iterations_all, host.iterations_all)
    assert dev.best_start == host.best_start and np.array_equal(dev.descent_steps_all, host.descent_steps_all)
    assert dev.status == host.status and dev.iterations == host.iterations
    assert np.all(np.abs(dev.u_all - host.u_all) <= 1e-9 * width)
    assert np.all(np.abs(dev.cost_all - host.cost_all) <= 1e-9 * np.abs(host.cost_all))
    assert abs(dev.cost - host.cost) <= 1e-9 * abs(host.cost) and abs(dev.cvar - host.cvar) <= 1e-9 * abs(host.cvar)
    assert abs(dev.expected_cost - host.expected_cost) <= 1e-9 * abs(host.expected_cost)
    assert dev.epsilon == host.epsilon and dev.alpha == host.alpha
    m = 1.0 - dev.alpha
    assert dev.cvar - dev.epsilon / (2 * m) <= dev.cost <= dev.cvar * (1 + 1e-12)
    again = dynamics.simulate_host(**{**{k: v for k, v in args.items() if k != 'controls'},
                                      'forcing': {**(args.get('forcing') or {}), **dynamics.expand_controls(dev)}},
                                   ReturnBounds=False, keep='members')
    assert np.array_equal(again.members, dev.members, equal_nan=True)
    return dev, host


def test_whole_solves_product_over_a_chunk_seam(device_ctx):
    dev, _ = _compare(device_ctx, product(65, 20, spread=0.3), [4.0], **PRODUCT, limits={'x1': (None, 0.0)}, limit_weight=1e2,
                      starts=2, alpha=0.9, draw_weights=_weights(65))
    assert dev.status == optimize.CONVERGED and dev.iterations > 1 and dev.cost < dev.cost_start
    assert dev.tail_weights.shape == (65,) and abs(dev.tail_weights.sum() - 1.0) < 1e-12
    rep = device_ctx.control_cvar_report()
    assert rep['iterations_with_work'] == int(dev.iterations_all.max()) + 1 and rep['launches_per_iteration'] == 7


def test_whole_solves_mixed_kernels_a_high_level(device_ctx):
    dev, _ = _compare(device_ctx, mixed(33, 20, spread=0.3), [10.0], **MIXED, starts=2, alpha=0.98)
    assert dev.status == optimize.CONVERGED and dev.iterations > 1 and dev.var <= dev.cvar


# ---------------------------------------------------------------------------------------------------------
# 3. alpha = 0 is the device's own control_pooled; the poll changes nothing
# ---------------------------------------------------------------------------------------------------------

KEYS = ('u_all', 'cost_all', 'status_all', 'iterations_all', 'descent_steps_all', 'members', 'cost_draws', 'cost_start',
        'first_saturation', 'u', 'z', 'cost', 'status', 'iterations', 'best_start', 'mean', 'bounds', 'violated', 'violation_share')


def test_alpha_zero_is_the_devices_own_control_pooled(device_ctx):
    args, kw = _case('mixed', 65)
    kw.update(starts=2, draw_weights=_weights(65), keep=['members', 'all'])
    risk = dynamics.control_cvar(**args, **kw, alpha=0.0, device=device_ctx)
    pooled = dynamics.control_pooled(**args, **kw, device=device_ctx)
    assert set(pooled) <= set(risk) and pooled.iterations > 0
    for key in pooled:
        if isinstance(pooled[key], (list, bool)):
            assert risk[key] == pooled[key], key
        else:
            assert np.array_equal(risk[key], pooled[key], equal_nan=True), key
    assert risk.expected_cost == risk.cost and np.array_equal(risk.tail_weights, risk.draw_weights) and risk.alpha == 0.0
    first = dynamics.control_cvar(**args, **kw, alpha=0.0, max_iter=0, device=device_ctx).first_pass
    want = dynamics.control_pooled(**args, **kw, max_iter=0, device=device_ctx).first_pass
    assert set(first) == set(want) and all(np.array_equal(first[key], want[key], equal_nan=True) for key in want)


def test_the_status_poll_and_a_repeated_call_change_nothing(device_ctx, monkeypatch):
    args, kw = _case('product', 9)
    kw.update(starts=2, keep=['members', 'all'], draw_weights=_weights(9), alpha=0.8)
    runs, reports = [], []
    for poll in ('0', '8', '8'):
        monkeypatch.setenv('FOKL_CONTROL_POLL', poll)
        runs.append(dynamics.control_cvar(**args, **kw, device=device_ctx))
        reports.append(device_ctx.control_cvar_report())
    for other in runs[1:]:
        for key in KEYS + ('cvar', 'var', 'a', 'epsilon', 'tail_weights', 'expected_cost'):
            assert np.array_equal(runs[0][key], other[key]), key
    most = int(runs[0].iterations_all.max())
    assert 0 < most < 60 and reports[0]['iterations_queued'] == 61 and reports[1]['iterations_queued'] == 8 * (most // 8 + 1)
    assert all(rep['iterations_with_work'] == most + 1 for rep in reports)


# ---------------------------------------------------------------------------------------------------------
# 4. native refusals and the report
# ---------------------------------------------------------------------------------------------------------

def _native(ctx, **change):
    args = mixed(3, 7)
    p = dynamics._prepare_control_pooled(args['models'], args['states'], args['inputs'], args['controls'], args['forcing'],
                                         args['y0'], args['t'], None, None, 3, None, {'T': 0.2}, None, None, None, 1e3,
                                         {'u': 0.01}, None, None, 2, 60, 1e-10, None, None)
    p.update(alpha=0.5, smoothing=0.01, epsilon=None)
    p.update(change)
    return ctx.control_cvar_solve(p)


def test_native_refusals_and_report(device_ctx, monkeypatch):
    from fokl_gpy_amd._capi import FoklNativeError
    solved = _native(device_ctx)[0]
    rep = device_ctx.control_cvar_report()
    assert rep['draws'] == 3 and rep['starts'] == 2 and rep['launches_per_iteration'] == 7 and rep['chunks'] == 1 and rep['D'] == 3
    assert 1 <= rep['iterations_with_work'] <= rep['iterations_queued'] and rep['NS'] == 2
    assert rep['step_lds_bytes'] == 7 * 64 * 8 and rep['risk_threads'] == 64 and rep['risk_lds_bytes'] == (2 * 64 + 2 * 64) * 8
    assert rep['lds_bytes'] > 0 and all(rep[key] >= 0 for key in ('tangent_ns', 'risk_ns', 'chunk_ns', 'step_ns', 'trial_ns', 'accept_ns'))
    assert solved['epsilon'] > 0
    cases = {
        "alpha must lie in \\[0, 1\\)": dict(alpha=1.0),
        "alpha must lie in \\[0, 1\\) ": dict(alpha=-0.1),
        "alpha must lie in \\[0, 1\\)  ": dict(alpha=float('nan')),
        "smoothing must be positive and finite": dict(smoothing=0.0),
        "smoothing must be positive and finite ": dict(smoothing=float('inf')),
        "epsilon must be positive and finite": dict(epsilon=0.0),
        "epsilon must be positive and finite ": dict(epsilon=float('inf')),
        "draw weights must be non-negative and finite": dict(pool_w=np.array([0.5, -0.5, 1.0])),
        "draw weights sum to zero": dict(pool_w=np.zeros(3)),
        "a start lies outside the box": dict(z0=np.array([[0.5, 1.5, 0.5], [0.5, 0.5, 0.5]])),      # inherited from fokl_control_solve
        "negative weights": dict(wt=np.array([-1.0, 0.0])),
        # nothing is tracked and constant controls move nothing: the pooled cost at the start is 0, a relative smoothing has no scale
        "relative to the pooled cost at the start, which is 0": dict(wt=np.zeros(2)),
    }
    for text, change in cases.items():
        with pytest.raises(FoklNativeError, match=text.strip()):
            _native(device_ctx, **change)
        assert set(device_ctx.control_cvar_report().values()) == {0}, text
    # the workspace: 3 draws x 2 starts x (2 + 3 + 9 + 64 + 2) x 8, (3 + 6 + 18) x 8 per (start, chunk), 64 x (4 + 3) x 8 per
    # start = 3840 + 432 + 7168 = 11 440 bytes
    monkeypatch.setenv('FOKL_CONTROL_CVAR_FREE_BYTES', '11439')
    with pytest.raises(FoklNativeError, match=r"workspace needs 11440 bytes .*FOKL_CONTROL_CVAR_FREE_BYTES"):
        _native(device_ctx)
    assert set(device_ctx.control_cvar_report().values()) == {0}
    monkeypatch.setenv('FOKL_CONTROL_CVAR_FREE_BYTES', '11440')
    _native(device_ctx)                                                # the context is as good as before
    assert device_ctx.control_cvar_report()['draws'] == 3
    with pytest.raises(ValueError, match="alpha must lie in \\[0, 1\\)"):     # in Python before any device is asked for
        dynamics.control_cvar(**mixed(3, 7), segments=3, targets={'T': 0.2}, alpha=1.0, device=object())

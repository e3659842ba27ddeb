"""dynamics.control on the MI355X against its statement dynamics.control_host (pinned without a device by
tests/test_control_host.py): the tangent pass of the first iterate (F, g, H) bit for bit -- the statement fixes every
order --, whole solves with equal status, iterations and best start, u within 1e-9 of the box width and the cost within 1e-9
relative (the package's customary 1e-9), and the returned trajectories as simulate_host's under the returned controls."""
import warnings

import numpy as np
import pytest

from control_cases import BERN, chain, linear, mixed, model, product
from fokl_gpy_amd import FoKLRoutines, dynamics, optimize

pytestmark = pytest.mark.gpu


def _width(args, kw):
    p = dynamics._prepare_control(**{**dict(forcing=None, draws=None, bounds=None, control_bounds=None, targets=None, weights=None,
                                            terminal=None, limits=None, limit_weight=1e3, move_weight=None, previous=None,
                                            init=None, starts=1, max_iter=60, tol=1e-10, keep=None, segments=8), **args, **kw})
    return p['ctl_width']


def _compare(ctx, args, **kw):
    """control against control_host: the first tangent pass bit for bit, then the whole solves -> (device, host)."""
    first_dev = dynamics.control(**args, **kw, max_iter=0, device=ctx).first_pass
    first_host = dynamics.control_host(**args, **kw, max_iter=0).first_pass
    for key in ('F', 'g', 'H'):
        differ = first_dev[key] != first_host[key]
        if differ.any():
            at = tuple(np.argwhere(differ)[0])
            print(f"\nfirst pass {key}: {int(differ.sum())} of {differ.size} values differ, first at {at}: device "
                  f"{first_dev[key][at]!r} host {first_host[key][at]!r}")
        assert np.array_equal(first_dev[key], first_host[key]), key
    assert np.isfinite(first_host['F']).all() and np.any(first_host['g'] != 0)
    host = dynamics.control_host(**args, **kw, keep=['members', 'all'])
    dev = dynamics.control(**args, **kw, keep=['members', 'all'], device=ctx)
    width = _width(args, kw)[:, np.newaxis]
    print(f"\nstatus {dev.status_all.ravel().tolist()} iterations {dev.iterations_all.ravel().tolist()} max |u - u_host| / width "
          f"{np.max(np.abs(dev.u_all - host.u_all) / width):.2e} max relative cost difference "
          f"{np.max(np.abs(dev.cost_all - host.cost_all) / np.abs(host.cost_all)):.2e}")
    assert np.array_equal(dev.status_all, host.status_all) and np.array_equal(dev.iterations_all, host.iterations_all)
    assert np.array_equal(dev.best_start, host.best_start) and np.array_equal(dev.descent_steps_all, host.descent_steps_all)
    assert np.all(np.abs(dev.u_all - host.u_all) <= 1e-9 * width)
    assert np.all(np.abs(dev.cost_all - host.cost_all) <= 1e-9 * np.abs(host.cost_all))
    assert np.all(np.abs(dev.cost_start - host.cost_start) <= 1e-9 * np.abs(host.cost_start))
    assert np.array_equal(dev.u, dev.u_all[np.arange(dev.u.shape[0]), dev.best_start])
    # every draw's trajectory under ITS OWN controls is simulate_host's, bit for bit
    system = {key: value for key, value in args.items() if key != 'controls'}
    for e in range(dev.u.shape[0]):
        draws = kw.get('draws')
        one = 'mean' if isinstance(draws, str) else np.array([e if draws is None else np.asarray(draws)[e]])
        if np.ndim(args['y0']) == 2:
            system['y0'] = np.asarray(args['y0'])[e]
        alone = dynamics.simulate_host(**{**system, 'forcing': {**(args.get('forcing') or {}), **dynamics.expand_controls(dev, e)}},
                                       draws=one, bounds=kw.get('bounds'), ReturnBounds=False, keep='members')
        assert np.array_equal(alone.members[0], dev.members[e])
        assert alone.first_saturation[0] == dev.first_saturation[e]
    return dev, host


def test_one_state_one_term_one_step_one_decision(device_ctx):
    rng = np.random.default_rng(1)
    args = dict(models=[model('b', [0.2, 0.9], [[1, 1]], [[-1.0, 1.0], [0.0, 2.0]], 1, rng)], states=['x'], inputs=[['x', 'u']],
                controls=['u'], y0=[0.3], t=(0.0, 0.05, 0.1))
    dev, _ = _compare(device_ctx, args, segments=1, targets={'x': 0.31}, terminal={'x': 1.0})
    rep = device_ctx.control_report()
    assert rep['NS'] == 1 and rep['solves'] == 1 and rep['D'] == 1 and rep['spline_factors'] == 0 and rep['bernoulli_factors'] == 2
    assert rep['lds_bytes'] == dynamics.control_lds_bytes(2, 1, 2, 1) and 1 <= rep['launches_with_work'] <= rep['launches_queued']
    assert dev.members.shape == (1, 1, 2) and dev.u.shape == (1, 1, 1)


def test_mixed_kernels_with_a_short_last_hold_and_several_starts(device_ctx):
    """Two states (spline + Bernoulli), 7 steps in holds of 3, 3 and 1; 3 draws x 2 starts."""
    args = mixed(3, 7)
    kw = dict(segments=3, targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01}, starts=2)
    dev, host = _compare(device_ctx, args, **kw)
    rep = device_ctx.control_report()
    assert rep['NS'] == 2 and rep['solves'] == 6 and rep['D'] == 3 and rep['spline_factors'] > 0 and rep['bernoulli_factors'] > 0
    assert rep['launches_with_work'] == int(dev.iterations_all.max()) + 1
    assert dev.u_bounds.shape == (1, 3, 2) and dev.bounds.shape == (2, 8, 2)
    # draw e alone is draw e of the full run, bit for bit; so is the mean draw run twice
    alone = dynamics.control(**args, **kw, draws=np.array([1]), keep=['members', 'all'], device=device_ctx)
    for key in ('u_all', 'cost_all', 'status_all', 'iterations_all'):
        assert np.array_equal(alone[key][0], dev[key][1]), key
    assert np.array_equal(alone.members[0], dev.members[1]) and alone.best_start[0] == dev.best_start[1]
    _compare(device_ctx, args, **{**kw, 'draws': 'mean'})


def test_eight_states(device_ctx):
    """The targets are draw 0's own trajectory under u = (3, 7), x7's moved by 0.001: small residuals."""
    args = chain(8, 2, 6)
    system = {key: value for key, value in args.items() if key != 'controls'}
    want = dynamics.simulate_host(**system, forcing={'u': np.repeat([3.0, 7.0], 3)}, draws=np.array([0]), ReturnBounds=False,
                                  keep='members').members[0]
    dev, _ = _compare(device_ctx, args, segments=2, targets={'x0': want[0], 'x7': want[7] + 0.001})
    assert device_ctx.control_report()['NS'] == 8 and np.all(dev.status == optimize.CONVERGED)
    assert np.all(np.abs(dev.u[0, 0] - [3.0, 7.0]) < 1.0)


def test_soft_limits_and_solves_that_finish_at_different_iterations(device_ctx):
    """A nonlinear system (product terms) whose free optimum crosses the ceiling on x0: the limit binds.  The solves end
    after different numbers of iterations: some finish while others continue."""
    args = {**product(3, 16), 'y0': np.array([[0.4, -0.3], [-0.5, 0.5], [0.7, -0.4]])}
    dev, _ = _compare(device_ctx, args, segments=4, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3},
                      limits={'x0': (None, 0.6), 'x1': (-0.5, None)}, limit_weight=1e2, starts=2)
    assert np.all(dev.status_all == optimize.CONVERGED) and len(set(dev.iterations_all.ravel().tolist())) > 1
    assert np.any(dev.members[:, 0] > 0.6)


def test_thirty_two_decision_values(device_ctx):
    dev, _ = _compare(device_ctx, linear(2, 16, 2, spread=0.05), segments=16, targets={'x0': 0.5, 'x1': -0.2},
                      move_weight={'u0': 0.01, 'u1': 0.01}, previous=[0.0, 0.1])
    assert device_ctx.control_report()['D'] == 32 and dev.u.shape == (2, 2, 16)


def test_a_saturating_horizon(device_ctx):
    """T starts beyond the range its reader was trained on (clamped throughout) and c on the lower edge of its box with a
    negative slope (the slope rule holds it): both act in the tangent pass of the first iterate."""
    args = {**mixed(2, 7), 'y0': [2.3, -0.2]}
    dev, _ = _compare(device_ctx, args, segments=3, targets={'T': 0.0}, bounds=[[-3.0, 3.0], [-2.0, -0.2]])
    assert dev.first_saturation.tolist() == [0, 0] and np.all(dev.members[:, 1] == -0.2) and np.all(dev.members[:, 0] > 2.0)


def test_segments_on_the_bounds_of_the_box(device_ctx):
    track = {'x0': 0.1 + 0.3 * np.sin(np.arange(49) / 5.0), 'x1': -0.05}
    dev, _ = _compare(device_ctx, linear(1, 48), segments=8, targets=track, weights={'x1': 0.5}, terminal={'x0': 2.0},
                      move_weight={'u0': 0.01}, control_bounds={'u0': (-0.3, 0.45)})
    on_bound = (dev.z[0] <= 0.0) | (dev.z[0] >= 1.0)
    assert dev.status[0] == optimize.CONVERGED and 2 <= int(on_bound.sum()) < 8
    assert np.all(dev.u[0][dev.z[0] <= 0.0] == -0.3)


def test_a_step_in_a_steepest_descent_lane(device_ctx):
    """tests/test_control_host.py's case: H overflows, no Newton trial moves z, lane 32 is taken."""
    c0, c1 = (float(v) for v in BERN[0])
    one = dict(betas=np.array([[-1e5 / c1 * c0, 1e5 / c1]]), mtx=np.array([[1]]), phis=BERN, minmax=[[0.0, 1.0]],
               kernel='Bernoulli Polynomials')
    args = dict(models=[one], states=['x'], inputs=[['u']], controls=['u'], y0=[0.0], t=(0.0, 0.5, 1.0))
    with np.errstate(over='ignore'):
        dev, _ = _compare(device_ctx, args, bounds=[[-1e9, 1e9]], segments=1, targets={'x': 1e5 + 1.0}, weights={'x': 1e300},
                          init=[[0.9999]])
    assert dev.descent_steps.tolist() == [1] and dev.z.tolist() == [[[1.0]]] and dev.status.tolist() == [optimize.CONVERGED]


def test_the_early_stop_read_changes_nothing(device_ctx, monkeypatch):
    args = product(4, 16)
    kw = dict(segments=4, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3}, starts=3, keep=['members', 'all'])
    runs, launches = [], []
    for poll in ('0', '1', '8'):
        monkeypatch.setenv('FOKL_CONTROL_POLL', poll)
        runs.append(dynamics.control(**args, **kw, device=device_ctx))
        launches.append(device_ctx.control_report())
    for other in runs[1:]:
        for key in ('u_all', 'cost_all', 'status_all', 'iterations_all', 'descent_steps_all', 'members', 'best_start', 'cost_start'):
            assert np.array_equal(runs[0][key], other[key]), key
    most = int(runs[0].iterations_all.max())
    assert most < 60 and launches[0]['launches_queued'] == 61 and launches[1]['launches_queued'] == most + 1
    assert all(rep['launches_with_work'] == most + 1 for rep in launches)


def _native(ctx, **change):
    """A small prepared problem with entries changed behind ``_prepare_control``'s back, given to the native entry point."""
    args = mixed(2, 7)
    p = dynamics._prepare_control(args['models'], args['states'], args['inputs'], args['controls'], args['forcing'], args['y0'],
                                  args['t'], None, None, 3, None, {'T': 0.2}, None, None, None, 1e3, {'u': 0.01}, None, None, 1,
                                  60, 1e-10, None)
    p.update(change)
    return ctx.control_solve(p)


def test_native_refusals(device_ctx):
    from fokl_gpy_amd._capi import FoklNativeError
    _native(device_ctx)
    assert device_ctx.control_report()['solves'] == 2
    nan_ref = np.full((2, 8), np.nan)
    cases = {
        "at most 32 decision values": dict(n_controls=11, ctl_lo=np.zeros(11), ctl_width=np.ones(11), move=np.zeros(11),
                                           prev=np.zeros(11), D=33, z0=np.full((1, 33), 0.5)),
        "box is empty or not finite": dict(ctl_width=np.array([0.0])),
        "box is empty or not finite ": dict(ctl_lo=np.array([np.nan])),
        "outside the training range": dict(ctl_lo=np.array([-1.0])),
        "read by no model": dict(norm_control=np.full(2, -1, dtype=np.int32)),
        "negative weights": dict(wt=np.array([-1.0, 0.0])),
        "negative weights ": dict(term=np.array([0.0, -1.0])),
        "move weights must be non-negative": dict(move=np.array([-0.1])),
        "limit weight must be non-negative": dict(hl=-1.0),
        "no residual at all": dict(ref=nan_ref, move=np.zeros(1)),
        "terminal weight needs a target": dict(ref=nan_ref, term=np.array([1.0, 0.0])),
        "a start lies outside the box": dict(z0=np.array([[0.5, 1.5, 0.5]])),
        "first steps must increase": dict(seg_first=np.array([0, 3, 3], dtype=np.int32)),
        "box is empty": dict(box=np.array([[-2.0, 2.0], [1.0, 1.0]])),
        "at most 1048576 solves": dict(starts=1 << 20, z0=np.full((1 << 20, 3), 0.5)),
    }
    for text, change in cases.items():
        with pytest.raises((FoklNativeError, ValueError), match=text.strip()):
            _native(device_ctx, **change)
        assert set(device_ctx.control_report().values()) == {0}, text
    # the horizon: no step, too many steps
    args = mixed(1, 7)
    p = dynamics._prepare_control(args['models'], args['states'], args['inputs'], args['controls'], args['forcing'], args['y0'],
                                  args['t'], None, None, 3, None, {'T': 0.2}, None, None, None, 1e3, None, None, None, 1, 60, 1e-10,
                                  None)
    for steps, text in ((0, "no step at all"), (4097, "at most 4096")):
        q = dict(p, n_steps=steps, forcing=np.zeros((steps, p['forcing'].shape[1])), ref=np.full((2, steps + 1), 0.2))
        with pytest.raises(FoklNativeError, match=text):
            device_ctx.control_solve(q)
        assert set(device_ctx.control_report().values()) == {0}
    # LDS: tests/test_control_host.py's system, past the check in Python
    q = dict(p, fac_norm=np.zeros(300, dtype=np.int32), fac_kind=np.ones(300, dtype=np.int32), fac_row=np.zeros(300, dtype=np.int32),
             fac_degree=np.ones(300, dtype=np.int32), n_forcing_factors=300)
    with pytest.raises(FoklNativeError, match=r"bytes of LDS \(\(2 x \(1 \+ 300 factors"):
        device_ctx.control_solve(q)
    assert set(device_ctx.control_report().values()) == {0}
    _native(device_ctx)                                                # the context is as good as before
    assert device_ctx.control_report()['solves'] == 2


def test_fit_resample_control_simulate(device_ctx):
    """Two small fits, ``resample``, then ``control`` per draw, then ``simulate`` under ``u_mean``."""
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
    assert all(m['betas'].shape[0] == 8 for m in models)
    args = dict(models=models, states=['T', 'c'], inputs=[['T', 'c', 'u'], ['T', 'c']], controls=['u'], y0=[0.5, -0.3],
                t=(0.0, 15.5 * 0.1, 0.1))
    kw = dict(segments=4, targets={'T': 0.0}, terminal={'T': 1.0}, move_weight={'u': 0.01})
    dev, host = _compare(device_ctx, args, **kw)
    assert dev.u.shape == (8, 1, 4) and np.all(dev.cost <= dev.cost_start) and np.all(dev.status != optimize.NON_FINITE)
    system = {key: value for key, value in args.items() if key != 'controls'}
    spread = dynamics.simulate(**system, forcing=dynamics.expand_controls(dev), keep='members', device=device_ctx)
    assert spread.members.shape == dev.members.shape
    assert np.all(np.abs(spread.mean[0, -1]) < np.abs(0.5))           # the common controls steer every draw towards the target

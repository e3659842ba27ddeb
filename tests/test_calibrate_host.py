"""dynamics.calibrate_host, the statement the device kernel is tested against (tests/test_calibrate_gpu.py): its target against
``simulate_host``'s trajectory bit for bit, the sampler against a posterior known in closed form, the jump move on a target
with two modes, the bitwise invariances counter-based numbers give, every refusal, and the layout of the struct the native
entry point takes -- none of which needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from test_simulate_host import BERN, SPLINES, _bern_model, _two_state_system
from fokl_gpy_amd import _capi, dynamics

W = dynamics.WALKERS


def _spline_model(betas, mtx, minmax):
    return dict(betas=np.asarray(betas, dtype=np.float64), mtx=np.asarray(mtx), phis=SPLINES, minmax=minmax, kernel='Cubic Splines')


# ---------------------------------------------------------------------------------------------------------
# the systems both test files use
# ---------------------------------------------------------------------------------------------------------

def two_state_u_parameter():
    """``test_simulate_host._two_state_system`` with u as a parameter: d = 2, both observed states, point 0 and a NaN."""
    args = _two_state_system(['T', 'c', 'u'])
    del args['forcing'], args['keep']
    points = np.array([0, 7, 15, 30])
    data = np.array([[1.0, 0.1], [1.02, np.nan], [np.nan, 0.12], [1.05, 0.2]])
    return dict(args, unknown=['y0:c', 'u'], observe=['T', 'c'], data=data, obs_points=points, obs_sd=[0.05, 0.1],
                prior={'u': (6.0, 4.0)})


def case_a():
    """1 state, d = 1 ('y0:y': the exponent d - 1 = 0), 8 steps, 3 observations with point 0 and one NaN among them, E = 2."""
    model = _bern_model([[0.3, -0.8, 0.2], [0.25, -0.7, 0.3]], [[1], [2]], [[0.0, 4.0]])
    return dict(models=[model], states=['y'], inputs=[['y']], y0=[1.0], t=(0.0, 0.8, 0.1), unknown=['y0:y'], observe=['y'],
                data=np.array([[1.4], [np.nan], [1.9]]), obs_points=np.array([0, 4, 8]), obs_sd=[0.2])


def case_b():
    """The two-state system with a real forcing column w besides the parameter u: d = 2 ('y0:c', u), 30 steps, every = 5,
    E = 6."""
    rng = np.random.default_rng(3)
    first = _bern_model(0.2 * rng.standard_normal((6, 6)), [[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0], [0, 0, 0, 2]],
                        [[0.0, 2.0], [-1.0, 1.0], [0.0, 10.0], [-1.0, 3.0]])
    second = _bern_model(0.2 * rng.standard_normal((6, 6)), [[1, 0, 0], [0, 3, 0], [2, 1, 0], [0, 0, 2], [1, 0, 1]],
                         [[0.5, 2.5], [-2.0, 2.0], [-5.0, 20.0]])
    w = 1.0 + 1.5 * np.sin(np.arange(30) / 5.0)
    data = np.array([[1.0], [1.01], [np.nan], [1.03], [1.02], [1.05]])
    return dict(models=[first, second], states=['T', 'c'], inputs=[['T', 'c', 'u', 'w'], ['T', 'c', 'u']], forcing={'w': w},
                y0=[1.0, 0.1], t=(0.0, 1.5, 0.05), unknown=['y0:c', 'u'], observe=['T'], data=data, every=5, obs_sd=[0.05],
                prior={'u': (5.0, 3.0)})


def case_c():
    """8 states and 8 parameters, d = 16, one spline model among them, 4 steps, E = 2: the NS = 8 instance, the largest 7 d."""
    rng = np.random.default_rng(11)
    names, params = [f's{j}' for j in range(8)], [f'k{j}' for j in range(8)]
    models, inputs = [], []
    for j in range(8):
        mtx = [[1, 0, 0], [0, 1, 0], [0, 0, 2], [1, 0, 1]]
        minmax = [[-1.0, 1.0 + 0.1 * j], [-1.0 - 0.05 * j, 1.0], [0.0, 2.0 + j]]
        betas = 0.3 * rng.standard_normal((2, 5))
        models.append(_spline_model(betas, mtx, minmax) if j == 3 else _bern_model(betas, mtx, minmax))
        inputs.append([names[j], names[(j + 1) % 8], params[j]])
    data = 0.2 * rng.standard_normal((2, 3))
    data[0, 1] = np.nan
    return dict(models=models, states=names, inputs=inputs, y0=np.zeros(8), t=(0.0, 0.4, 0.1),
                unknown=[f'y0:{n}' for n in names] + params, observe=['s0', 's3', 's6'], data=data,
                obs_points=np.array([2, 4]), obs_sd=[0.3, 0.2, 0.4], prior={'k2': (1.0, 0.5), 'y0:s1': (0.0, 0.4)})


def mixed_system():
    """A 'Cubic Splines' model and a Bernoulli one; the parameter k is read by both with different minmax rows."""
    rng = np.random.default_rng(7)
    first = _spline_model(0.3 * rng.standard_normal((3, 4)), [[1, 0], [0, 2], [2, 1]], [[0.0, 2.0], [0.5, 3.0]])
    second = _bern_model(0.3 * rng.standard_normal((3, 5)), [[1, 0, 0], [0, 2, 0], [0, 0, 1], [1, 0, 3]],
                         [[-0.5, 2.5], [-1.0, 1.0], [0.0, 2.5]])
    return dict(models=[first, second], states=['x', 'z'], inputs=[['x', 'k'], ['x', 'z', 'k']], y0=[1.0, 0.0], t=(0.0, 1.0, 0.1),
                unknown=['k', 'y0:x'], observe=['z', 'x'], data=np.array([[0.05, np.nan], [0.1, 1.1], [np.nan, 1.2]]),
                obs_points=np.array([0, 5, 10]), obs_sd=[0.1, 0.2], prior={'k': (1.5, 1.0)})


SYSTEM_KEYS = ('models', 'states', 'inputs', 't', 'draws', 'bounds')


def lp_from_simulate_host(args, p, theta, e):
    """lp and the saturation flag of draw e at theta [d] (true scale), from ``simulate_host``'s trajectory: every parameter as
    a constant forcing array, y0 overwritten, the sums in the stated order."""
    forcing, y0 = dict(args.get('forcing') or {}), np.array(np.broadcast_to(args['y0'], (p['K'],)), dtype=np.float64)
    for i, name in enumerate(p['unknown']):
        if name.startswith('y0:'):
            y0[p['states'].index(name[3:])] = theta[i]
        else:
            forcing[name] = np.full(p['n_steps'], theta[i])
    sim = dynamics.simulate_host(**{k: args[k] for k in SYSTEM_KEYS if k in args}, forcing=forcing, y0=y0, ReturnBounds=False,
                                 keep='members')
    y = sim.members[e]
    ss = 0.0
    for r, point in enumerate(p['obs_points']):
        for o in range(len(p['obs_names'])):
            if not np.isnan(p['data'][r, o]):
                res = p['data'][r, o] - y[p['obs_state'][o], point]
                ss = ss + p['obs_hp'][o] * (res * res)
    pp = 0.0
    for i in range(p['d']):
        dl = theta[i] - p['prior_mean'][i]
        pp = pp + p['prior_prec'][i] * (dl * dl)
    return -ss - 0.5 * pp, bool(sim.first_saturation[e] >= 0), y


# ---------------------------------------------------------------------------------------------------------
# 1. the target is simulate_host's trajectory
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('system', [two_state_u_parameter, mixed_system], ids=['two_state', 'mixed_kernels'])
def test_target_is_simulate_hosts_trajectory(system):
    args = system()
    p = dynamics._prepare_calibrate(**args)
    walkers = [0, 1, 5, 64, 127]
    theta = np.broadcast_to(p['starts'][walkers], (p['E'], len(walkers), p['d']))
    lp, sat, points = dynamics.calibrate_target(p, theta, trajectories=True)
    assert np.isfinite(lp).all()
    for e in range(p['E']):
        for i in range(len(walkers)):
            want, want_sat, y = lp_from_simulate_host(args, p, theta[e, i], e)
            assert lp[e, i] == want and sat[e, i] == want_sat, (e, i, lp[e, i], want)
            assert np.array_equal(points[e, i], y)
    print(f"\n{system.__name__}: {lp.size} targets equal simulate_host's bit for bit; {int(sat.sum())} of them saturated")
    if system is mixed_system:                                          # k is normalised twice: two forcing inputs, one unknown
        assert p['norm_param'].tolist() == [0, 0] and p['lo'][0] == 0.5 and p['hi'][0] == 2.5


# ---------------------------------------------------------------------------------------------------------
# 2. the exact posterior of a linear system
# ---------------------------------------------------------------------------------------------------------

def linear_system():
    """``test_simulate_host``'s linear model with an input: dy/dt = a + b y + c u exactly (one order-1 term per column)."""
    c0, c1 = (float(v) for v in BERN[0])
    b1, b2 = -2.0 / c1, 1.0 / c1                                       # b = b1 c1 / 4 = -0.5, c = b2 c1 / 2 = 0.5
    model = _bern_model([[0.5 - (b1 + b2) * c0, b1, b2]], [[1, 0], [0, 1]], [[0.0, 4.0], [0.0, 2.0]])     # a = 0.5
    return dict(models=[model], states=['y'], inputs=[['y', 'u']], t=(0.0, 1.5, 0.25))


def test_exact_posterior_of_a_linear_system():
    """RK4 makes every point affine in (y0, u); with a Gaussian prior the posterior is Gaussian in closed form.  The margin
    (0.1 sd on the mean, 10 % on the sd) is more than twice the worst of 20 seeds of a numpy restatement of the 128-walker
    sampler on a correlated 2-D Gaussian (0.043 sd, 3.1 %)."""
    system = linear_system()
    run = lambda y0, u: dynamics.simulate_host(**system, y0=[y0], forcing={'u': np.full(6, u)}, ReturnBounds=False,
                                               keep='members').members[0, 0]
    base, by_y0, by_u = run(1.5, 1.0), run(2.5, 1.0), run(1.5, 2.0)
    B, C = by_y0 - base, by_u - base
    A = base - 1.5 * B - 1.0 * C
    assert np.allclose(run(1.1, 0.3), A + 1.1 * B + 0.3 * C, rtol=0, atol=1e-13)      # affine, as claimed
    points, sd_obs = np.array([2, 4, 6]), 0.02
    rng = np.random.default_rng(1)
    data = (A + 1.4 * B + 1.1 * C)[points] + sd_obs * rng.standard_normal(3)
    prior = {'u': (1.0, 0.5), 'y0:y': (1.5, 1.0)}
    G = np.stack([B[points], C[points]], axis=1)
    prec = G.T @ G / sd_obs ** 2 + np.diag([1.0 / 1.0 ** 2, 1.0 / 0.5 ** 2])
    cov = np.linalg.inv(prec)
    mean = cov @ (G.T @ (data - A[points]) / sd_obs ** 2 + np.array([1.5 / 1.0 ** 2, 1.0 / 0.5 ** 2]))
    sd = np.sqrt(np.diag(cov))
    assert np.all(mean - 6 * sd > [0.0, 0.0]) and np.all(mean + 6 * sd < [4.0, 2.0])  # the box is 6 sd away on each side
    res = dynamics.calibrate_host(**system, y0=[0.0], unknown=['y0:y', 'u'], observe=['y'], data=data[:, np.newaxis],
                                  obs_points=points, obs_sd=[sd_obs], prior=prior, burnin=200, draws_kept=500, thin=10, seed=4)
    got_sd = np.sqrt(np.diag(res.cov))
    print(f"\nexact mean {mean}, sd {sd}, correlation {cov[0, 1] / sd[0] / sd[1]:.3f}; sampled mean {res.mean}, sd {got_sd}; "
          f"mean error / sd {np.abs(res.mean - mean) / sd}, sd ratio {got_sd / sd}, rhat_max {res.rhat_max:.3f}, "
          f"saturated {res.saturated.mean():.3f}")
    assert res.x.shape == (50 * W, 2) and not res.invalid.any()
    assert np.all(np.abs(res.mean - mean) <= 0.1 * sd)
    assert np.all(np.abs(got_sd / sd - 1.0) <= 0.1)


# ---------------------------------------------------------------------------------------------------------
# 3. the jump move
# ---------------------------------------------------------------------------------------------------------

def test_jump_move_carries_walkers_between_modes():
    """dy/dt = beta B2(u) does not depend on y, and B2(u) = u^2 - u + 1/6 is symmetric about 1/2: one measurement of y gives
    two modes, at u = 1/4 and u = 3/4, whose masses the prior makes unequal.  The stretch move alone keeps every walker in
    the mode it started in; the jump move makes the left mode's share the exact one."""
    model = _bern_model([[0.5, 4.0]], [[2]], [[0.0, 1.0]])
    system = dict(models=[model], states=['y'], inputs=[['u']], y0=[0.0], t=(0.0, 1.0, 0.5))
    truth = dynamics.simulate_host(**system, forcing={'u': np.full(2, 0.25)}, ReturnBounds=False, keep='members').members[0, 0, 2]
    call = dict(system, unknown=['u'], observe=['y'], data=[[truth]], obs_points=[2], obs_sd=[0.04], prior={'u': (0.9, 0.5)})
    p = dynamics._prepare_calibrate(**call)
    grid = (np.arange(40000) + 0.5) / 40000
    lp = dynamics.calibrate_target(p, grid[np.newaxis, :, np.newaxis])[0][0]
    weight = np.exp(lp - lp.max())
    exact = weight[grid < 0.5].sum() / weight.sum()
    valley = weight[np.abs(grid - 0.5) < 0.1].max() / weight.max()
    rng = np.random.default_rng(0)
    starts = np.where(np.arange(W) % 4 != 3, 0.25, 0.75)[:, np.newaxis] + 0.01 * rng.standard_normal((W, 1))
    share_of_starts = float(np.mean(starts < 0.5))
    jumping = dynamics.calibrate_host(**call, starts=starts, burnin=400, draws_kept=1600, thin=8, jump_every=8, seed=2)
    frozen = dynamics.calibrate_host(**call, starts=starts, burnin=100, draws_kept=200, thin=8, jump_every=0, seed=2)
    share = float(np.mean(jumping.x[:, 0] < 0.5))
    share_frozen = float(np.mean(frozen.x[:, 0] < 0.5))
    print(f"\nleft mode: exact share {exact:.4f} (the valley between the modes holds {valley:.1e} of the peak), jump_every=8 "
          f"{share:.4f}, jump_every=0 {share_frozen:.4f}, the starts {share_of_starts:.4f}; jump acceptance {jumping.accept[0, 1]:.3f}")
    assert share_of_starts == 0.75 and abs(exact - share_of_starts) > 0.3
    assert abs(share - exact) <= 0.03
    assert share_frozen == share_of_starts
    assert np.isnan(frozen.accept[0, 1]) and jumping.accept[0, 1] > 0.05


# ---------------------------------------------------------------------------------------------------------
# 4. invariances, an invalid draw, refusals, the struct
# ---------------------------------------------------------------------------------------------------------

SHORT = dict(burnin=3, draws_kept=9, thin=1, jump_every=3, seed=5)


@pytest.fixture(scope='module')
def full_run():
    return dynamics.calibrate_host(**case_b(), **SHORT, keep=['x', 'trajectories'])


def rows_of(res):
    return res.x.reshape(res.draws, -1, W, res.x.shape[1])


def test_a_draw_alone_is_that_draw_of_the_full_run(full_run):
    alone = dynamics.calibrate_host(**case_b(), **SHORT, draws=np.array([4]), keep=['x', 'trajectories'])
    assert alone.draw_ids.tolist() == [4] and np.all(alone.draw == 4)
    pick = full_run.draw == 4
    assert np.array_equal(alone.x, full_run.x[pick]) and np.array_equal(alone.lp, full_run.lp[pick])
    assert np.array_equal(alone.saturated, full_run.saturated[pick])
    assert np.array_equal(alone.trajectories[0], full_run.trajectories[4])
    assert np.array_equal(alone.evals, full_run.evals[4:5]) and np.array_equal(alone.rhat, full_run.rhat[4:5])


def test_thinned_rows_are_every_third_row(full_run):
    thinned = dynamics.calibrate_host(**case_b(), **dict(SHORT, thin=3))
    assert rows_of(thinned).shape[1] == 3
    assert np.array_equal(rows_of(thinned), rows_of(full_run)[:, ::3])
    assert np.array_equal(thinned.lp.reshape(6, 3, W), full_run.lp.reshape(6, 9, W)[:, ::3])
    assert np.array_equal(thinned.rhat, full_run.rhat) and np.array_equal(thinned.accept, full_run.accept)


def test_a_nan_coefficient_invalidates_its_draw_only(full_run):
    args = case_b()
    args['models'][1] = dict(args['models'][1], betas=args['models'][1]['betas'].copy())
    args['models'][1]['betas'][2, 1] = np.nan
    res = dynamics.calibrate_host(**args, **SHORT, keep=['x', 'trajectories'])
    assert res.invalid.tolist() == [False, False, True, False, False, False]
    rest = full_run.draw != 2
    assert np.array_equal(res.x[rest], full_run.x[rest]) and np.array_equal(res.lp[rest], full_run.lp[rest])
    assert np.isnan(res.lp[~rest]).all()
    starts = dynamics._prepare_calibrate(**args)['starts']
    assert np.array_equal(rows_of(res)[2], np.broadcast_to(starts, (9, W, 2)))        # a NaN walker is never left
    assert res.accept[2].tolist() == [0.0, 0.0] and res.evals[2] > W


def test_result_fields(full_run):
    res = full_run
    assert res.x.shape == (6 * 9 * W, 2) and res.lp.shape == res.draw.shape == res.saturated.shape == (6 * 9 * W,)
    assert res.trajectories.shape == (6, W, 2, 31) and res.fit_mean.shape == (2, 31) and res.fit_bounds.shape == (2, 31, 2)
    assert res.accept.shape == (6, 2) and res.rhat.shape == (6, 2) and res.evals.shape == (6,) and res.unknown == ['y0:c', 'u']
    assert np.all(res.fit_bounds[..., 0] <= res.fit_mean) and np.all(res.fit_mean <= res.fit_bounds[..., 1])
    assert np.all((res.x > res.box[:, 0]) & (res.x < res.box[:, 1]))
    last = rows_of(res)[:, -1]                                          # the replay is the final ensemble's own trajectory
    assert np.array_equal(res.trajectories[:, :, 1, 0], last[:, :, 0])
    bare = dynamics.calibrate_host(**case_b(), **SHORT, keep=None)
    assert bare.x is None and bare.cov is None and 'trajectories' not in bare
    assert np.array_equal(bare.rhat, res.rhat) and np.allclose(bare.mean, rows_of(res).mean(axis=(0, 1, 2)), rtol=1e-12)


def test_a_single_kept_iteration():
    res = dynamics.calibrate_host(**case_a(), burnin=0, draws_kept=1, thin=1, jump_every=0)
    assert res.x.shape == (2 * W, 1) and np.isnan(res.rhat).all() and np.isnan(res.rhat_max)
    assert np.allclose(res.mean_per_draw[:, 0], res.x.reshape(2, W).mean(axis=1), rtol=1e-12)
    assert np.allclose(res.sd_per_draw[:, 0], res.x.reshape(2, W).std(axis=1), rtol=1e-9)


REFUSALS = [
    (dict(unknown=[]), "unknown must list 1 to 16 unknowns"),
    (dict(unknown=['u', 'y0:c', 'u']), "unknown names 'u' twice"),
    (dict(unknown=['y0:q']), "unknown: 'y0:q' names no state"),
    (dict(unknown=['T']), "unknown: 'T' is a state \\(its initial value is 'y0:T'\\)"),
    (dict(unknown=['w', 'u']), "unknown: 'w' is a forcing key"),
    (dict(unknown=['u', 'v']), "unknown: no model reads 'v'"),
    (dict(unknown=['y0:c']), "inputs\\[0\\]: 'u' is neither a state"),
    (dict(unknown_bounds={'q': (0, 1)}), "unknown_bounds: 'q' is not an unknown"),
    (dict(unknown_bounds={'u': (0, np.inf)}), "unknown_bounds\\['u'\\] must be two finite numbers"),
    (dict(unknown_bounds={'u': (3.0, 3.0)}), "unknown_bounds\\['u'\\] is empty"),
    (dict(unknown_bounds={'u': (-6.0, 5.0)}), "unknown_bounds\\['u'\\] reaches outside the training range \\[0.0, 10.0\\]"),
    (dict(unknown_bounds={'y0:c': (-1.5, 0.5)}), "unknown_bounds\\['y0:c'\\] reaches outside the box \\[-1.0, 1.0\\] of the state"),
    (dict(prior={'T': (1.0, 1.0)}), "prior: 'T' is not an unknown"),
    (dict(prior={'u': (1.0, 0.0)}), "prior\\['u'\\] must be \\(mean, sd\\)"),
    (dict(starts=np.zeros((64, 2))), "starts must be finite numbers \\[128, 2\\]"),
    (dict(starts=np.full((128, 2), [1.0, 3.0])), "every start must lie strictly inside the box"),
    (dict(burnin=-1), "burnin must be an integer >= 0"),
    (dict(draws_kept=0), "draws_kept must be an integer >= 1"),
    (dict(thin=0), "thin must be an integer >= 1"),
    (dict(jump_every=-2), "jump_every must be an integer >= 0"),
    (dict(seed=0.5), "seed must be an integer"),
    (dict(keep='members'), "keep must be None, 'x', 'trajectories' or a list of the two"),
    (dict(observe=[]), "observe must name at least one measured state"),
    (dict(observe=['u']), "observe: 'u' is not a state"),
    (dict(every=None), "give either obs_points"),
    (dict(obs_sd=[0.0]), "obs_sd must be positive and finite"),
    (dict(data=np.zeros((5, 1))), "data must be \\[6, 1\\]"),
]


@pytest.mark.parametrize('change, message', REFUSALS, ids=[m[:32] for _, m in REFUSALS])
def test_refusals_name_what_is_wrong(change, message):
    with pytest.raises(ValueError, match=message):
        dynamics.calibrate_host(**{**case_b(), **SHORT, **change})


def test_other_refusals():
    args = case_c()
    with pytest.raises(ValueError, match="unknown must list 1 to 16 unknowns"):
        dynamics.calibrate_host(**dict(args, unknown=args['unknown'] + ['k9']))
    # a state no model reads has no finite box of its own
    model = _bern_model([[0.5, 4.0]], [[2]], [[0.0, 1.0]])
    free = dict(models=[model], states=['y'], inputs=[['u']], y0=[0.0], t=(0.0, 1.0, 0.5), unknown=['u', 'y0:y'], observe=['y'],
                data=[[0.3]], obs_points=[2], obs_sd=[0.1])
    with pytest.raises(ValueError, match="unknown 'y0:y': its box .* is not finite"):
        dynamics.calibrate_host(**free)
    assert dynamics._prepare_calibrate(**dict(free, bounds=[[-1.0, 1.0]]))['hi'].tolist() == [1.0, 1.0]
    # two readers of one parameter whose training ranges have nothing in common
    mixed = mixed_system()
    mixed['models'][1] = dict(mixed['models'][1], minmax=[[-0.5, 2.5], [-1.0, 1.0], [3.5, 4.0]])
    with pytest.raises(ValueError, match="parameter 'k': its box is empty"):
        dynamics.calibrate_host(**mixed)
    # the LDS budget: 16 unknowns next to 64 coefficients and many factors
    big = case_c()
    big['models'] = [dict(m, mtx=np.array([[o, 0, 0] for o in range(1, 13)] + [[0, o, 0] for o in range(1, 13)] + [[0, 0, 1]]),
                          betas=np.zeros((2, 26))) if m['kernel'] != 'Cubic Splines' else m for m in big['models']]
    with pytest.raises(ValueError, match=r"the problem needs (\d+) bytes of LDS \(\(1 \+ (\d+) factors \+ 16 normalised states \+ "
                                         r"7 x 16 unknowns\) x 64 x 8 \+ (\d+) coefficients x 8\), a wavefront has 147456") as hit:
        dynamics._prepare_calibrate(**big)
    need, factors, coef = (int(v) for v in re.search(r"needs (\d+) bytes .* (\d+) factors .* (\d+) coefficients", str(hit.value)).groups())
    assert need == (1 + factors + 16 + 112) * 512 + coef * 8 > 147456
    # without a device the call raises: the host statement is not a fallback
    if _capi.device_count() == 0:
        with pytest.raises(_capi.FoklNativeError):
            dynamics.calibrate(**case_a())


def test_lds_bytes_of_the_three_cases():
    for case, (factors, states, coef, d) in ((case_a, (2, 1, 3, 1)), (case_b, (11, 4, 12, 2)), (case_c, (32, 16, 40, 16))):
        p = dynamics._prepare_calibrate(**case())
        assert (p['fac_norm'].shape[0], p['norm_src'].shape[0] - p['n_norm_forcing'], p['coef'].shape[0], p['d']) == \
            (factors, states, coef, d), case.__name__
        assert p['lds_bytes'] == (1 + factors + states + 7 * d) * 64 * 8 + coef * 8


def test_random_numbers_are_a_stream_of_their_own():
    ids = np.array([0, 3], dtype=np.uint32)
    u = _capi.calibrate_rng(9, ids, 2, _capi.INFER_U1, W)
    assert u.shape == (2, W) and np.all((u >= 0) & (u < 1)) and not np.array_equal(u[0], u[1])
    assert np.array_equal(_capi.calibrate_rng(9, ids[1:], 2, _capi.INFER_U1, W)[0], u[1])
    assert not np.array_equal(u[0, :64], _capi.infer_rng(9, 0, 2, _capi.INFER_U1, 64))          # fourth counter word 1
    assert not np.array_equal(u, _capi.assimilate_rng(9, ids, 2, _capi.ASSIMILATE_RESAMPLE, W))  # ... and 2
    normal = _capi.calibrate_rng(9, ids, 2, _capi.INFER_JITTER, 4096)
    assert abs(normal.mean()) < 0.05 and abs(normal.std() - 1.0) < 0.05
    with pytest.raises(_capi.FoklNativeError):
        _capi.calibrate_rng(9, ids, 2, 4, 1)


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every offsetof of fokl_calibrate_problem as a C compiler lays it out equal the ctypes class's, field by
    field and by name (as tests/test_capi_symbols.py checks the two other structs)."""
    import shutil
    import subprocess
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, "no C compiler: the layout of the struct cannot be checked"
    internal = os.path.join(ROOT, 'include', 'fokl_hip_internal.h')
    cls, c_name = _capi._CalibrateProblemStruct, 'fokl_calibrate_problem'
    lines = [f'    printf("sizeof %zu\\n", sizeof({c_name}));']
    lines += [f'    printf("{field} %zu\\n", offsetof({c_name}, {field}));' for field, _ in cls._fields_]
    source = tmp_path / 'layout.c'
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fokl_hip_internal.h"\nint main(void)\n{\n' +
                      '\n'.join(lines) + '\n    return 0;\n}\n')
    program = tmp_path / 'layout'
    res = subprocess.run([cc, '-std=c99', '-Wall', '-I', os.path.dirname(internal), '-o', str(program), str(source)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    printed = subprocess.run([str(program)], capture_output=True, text=True, check=True).stdout.split('\n')
    in_c = {f: int(v) for f, v in (line.split() for line in printed if line)}
    in_python = {'sizeof': ctypes.sizeof(cls), **{field: getattr(cls, field).offset for field, _ in cls._fields_}}
    assert in_python == in_c
    text = re.sub(r'/\*.*?\*/', '', open(internal).read(), flags=re.S)
    body = re.search(r'typedef struct ' + c_name + r' \{(.*?)\} ' + c_name + ';', text, flags=re.S).group(1)
    fields = [name for decl in body.split(';') for name in re.findall(r'(\w+)\s*(?:,|$)', decl.strip())]
    assert fields == [field for field, _ in cls._fields_]

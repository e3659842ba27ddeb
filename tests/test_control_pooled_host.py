"""dynamics.control_pooled_host, the statement the pooled-control kernels are tested against
(tests/test_control_pooled_gpu.py): the order of the pooled sum, one draw as ``control``, the per-draw parts as
``control``'s, a linear system against scipy's bounded least squares on the stacked problem, the pooled gradient against
central differences, what the feature is for (one sequence that beats ``u_mean``), the weights, what follows downstream and
every refusal -- none of which needs a device."""
import numpy as np
import pytest
from scipy.optimize import lsq_linear

from control_cases import linear, mixed, product
from fokl_gpy_amd import dynamics, optimize

NONLINEAR = dict(segments=4, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3})
LQ_COST_GATE, LQ_Z_GATE = 2.95e-14, 5.22e-14          # tests/test_control_host.py's, for one draw
GRADIENT_GATE = 7.3e-11                                # tests/test_control_host.py's central-difference gate ('idle')


def _system(args):
    return {key: value for key, value in args.items() if key != 'controls'}


# ---------------------------------------------------------------------------------------------------------
# 1. the order of the sum
# ---------------------------------------------------------------------------------------------------------

def test_pooled_sum_is_the_chunked_order_spelled_out():
    rng = np.random.default_rng(5)
    E = 130
    X = rng.standard_normal((E, 7)) * 10.0 ** rng.integers(-8, 8, size=(E, 1))
    w = rng.random(E)
    w[[3, 64, 129]] = 0.0
    X[3] = np.nan                                                      # a zero weight in front of a NaN row
    X[129] = np.inf
    chunks = []
    for begin in (0, 64, 128):
        acc = [0.0] * 7
        for e in range(begin, min(begin + 64, E)):
            if w[e] == 0:
                continue
            acc = [acc[k] + float(w[e]) * float(X[e, k]) for k in range(7)]
        chunks.append(acc)
    want = chunks[0]
    for acc in chunks[1:]:
        want = [want[k] + acc[k] for k in range(7)]
    got = dynamics.pooled_sum(X, w)
    assert got.shape == (7,) and np.isfinite(got).all()
    assert got.tolist() == want
    assert dynamics.POOL_CHUNK == 64
    # not the order of a plain left-to-right sum: the chunk seam shows
    plain = [0.0] * 7
    for e in range(E):
        if w[e] != 0:
            plain = [plain[k] + float(w[e]) * float(X[e, k]) for k in range(7)]
    assert got.tolist() != plain
    assert dynamics.pooled_sum(X[:1].reshape(1, 7) * 0 + 2.5, np.array([1.0])).tolist() == [2.5] * 7
    with pytest.raises(ValueError, match="one row per weight"):
        dynamics.pooled_sum(X, w[:5])


# ---------------------------------------------------------------------------------------------------------
# 2., 3. one draw is control; the per-draw parts are control's
# ---------------------------------------------------------------------------------------------------------

def test_one_draw_is_control_bit_for_bit():
    args = mixed(1, 20)
    kw = dict(segments=4, targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01}, starts=3, keep=['members', 'all'])
    pooled, own = dynamics.control_pooled_host(**args, **kw), dynamics.control_host(**args, **kw)
    for key in ('z', 'cost', 'cost_start', 'status', 'iterations', 'best_start', 'descent_steps', 'u'):
        assert np.array_equal(pooled[key], own[key][0]), key
    assert np.array_equal(pooled.members, own.members) and np.array_equal(pooled.first_saturation, own.first_saturation)
    for key in ('u_all', 'cost_all', 'status_all', 'iterations_all'):
        assert np.array_equal(pooled[key], own[key][0]), key
    assert pooled.iterations > 0 and np.array_equal(pooled.mean, own.members[0]) and 'bounds' not in pooled


def test_first_pass_per_draw_parts_are_controls():
    args = product(9, 20, spread=0.3)
    init = np.array([[1.0, 2.5, 0.5, 3.0]])
    pooled = dynamics.control_pooled_host(**args, **NONLINEAR, init=init, starts=2, max_iter=0).first_pass
    own = dynamics.control_host(**args, **NONLINEAR, init=init, starts=2, max_iter=0).first_pass
    assert pooled['F_draws'].shape == (2, 9) and pooled['g_draws'].shape == (2, 9, 4) and pooled['H_draws'].shape == (2, 9, 4, 4)
    assert np.array_equal(pooled['F_draws'], own['F'].T)
    assert np.array_equal(pooled['g_draws'], own['g'].transpose(1, 0, 2))
    assert np.array_equal(pooled['H_draws'], own['H'].transpose(1, 0, 2, 3))
    w = np.full(9, 1.0) / 9.0
    for s in range(2):
        assert pooled['F'][s] == dynamics.pooled_sum(own['F'][:, s], w)
        assert np.array_equal(pooled['g'][s], dynamics.pooled_sum(own['g'][:, s], w))
        assert np.array_equal(pooled['H'][s], dynamics.pooled_sum(own['H'][:, s], w))


# ---------------------------------------------------------------------------------------------------------
# 4. a linear system against lsq_linear on the stacked problem
# ---------------------------------------------------------------------------------------------------------

def test_linear_system_against_stacked_bounded_least_squares():
    """Order-1 Bernoulli terms only and idle clamps: every draw's trajectory is affine in z, the pooled cost is the linear
    least-squares problem whose rows are draw e's scaled by sqrt(w_e), built from simulate_host as
    tests/test_control_host.py builds one draw's; ``lsq_linear(method='bvls')`` solves it exactly.  Gates: that file's."""
    E, steps, nc, K = 5, 12, 2, 4
    D = nc * K
    args = linear(E, steps, n_controls=2, spread=0.1)
    w = np.array([0.5, 1.0, 2.0, 0.25, 1.25])
    wn = w / w.sum()
    track = {'x0': 0.1 + 0.1 * np.sin(np.arange(steps + 1) / 5.0), 'x1': -0.05}
    weights, terminal, move = {'x0': 1.0, 'x1': 0.5}, {'x0': 2.0}, 0.01
    res = dynamics.control_pooled_host(**args, segments=K, targets=track, weights=weights, terminal=terminal,
                                       move_weight={'u0': move, 'u1': move}, draw_weights=w, keep='members')
    assert np.all(res.first_saturation == -1)
    lo, width = np.array([-1.0, -1.0]), np.array([2.0, 2.0])
    seg_of = np.searchsorted(res.segment_first, np.arange(steps), side='right') - 1
    h, P = args['t'][2], steps + 1

    def residuals(z):
        u = lo[:, np.newaxis] + z.reshape(nc, K) * width[:, np.newaxis]
        forcing = {name: u[c][seg_of] for c, name in enumerate(args['controls'])}
        ys = dynamics.simulate_host(**{**_system(args), 'forcing': forcing}, ReturnBounds=False, keep='members').members
        assert np.all(np.abs(ys) < 4.0)                                # the clamps stay idle: the map is affine
        rows = []
        for e in range(E):
            y = ys[e]
            r = [np.sqrt(h * wt) * (y[j, 1:] - np.broadcast_to(track[name], P)[1:]) for j, (name, wt) in enumerate(weights.items())]
            r.append(np.sqrt(2.0) * (y[0, -1:] - track['x0'][-1:]))
            for c in range(nc):
                r.append(np.sqrt(move) * np.diff(u[c]))
            rows.append(np.sqrt(wn[e]) * np.concatenate(r))
        return np.concatenate(rows)

    centre = np.full(D, 0.5)
    r0 = residuals(centre)
    A = np.stack([(residuals(centre + 0.25 * np.eye(D)[d]) - r0) / 0.25 for d in range(D)], axis=1)
    b = A @ centre - r0
    ref = lsq_linear(A, b, bounds=(0.0, 1.0), method='bvls', tol=1e-15, max_iter=2000)
    cost_ref = float(np.sum((A @ ref.x - b) ** 2))
    z = res.z.ravel()
    relative = abs(res.cost - cost_ref) / cost_ref
    print(f"\nstacked problem: status {res.status}, {res.iterations} iterations, cost {res.cost:.15e} (exact {cost_ref:.15e}, "
          f"relative difference {relative:.2e}), max |z - z_ref| {np.max(np.abs(z - ref.x)):.2e}")
    assert res.status == optimize.CONVERGED and 1 <= res.iterations <= 3
    assert not np.any((ref.x <= 0.0) | (ref.x >= 1.0))
    assert relative <= LQ_COST_GATE
    assert np.max(np.abs(z - ref.x)) <= LQ_Z_GATE
    # the first step alone lands there: the problem is quadratic and the box idle
    one = dynamics.control_pooled_host(**args, segments=K, targets=track, weights=weights, terminal=terminal,
                                       move_weight={'u0': move, 'u1': move}, draw_weights=w, max_iter=1)
    print(f"after one step: max |z - z_ref| {np.max(np.abs(one.z.ravel() - ref.x)):.2e}")
    assert np.max(np.abs(one.z.ravel() - ref.x)) <= LQ_Z_GATE


# ---------------------------------------------------------------------------------------------------------
# 5. the pooled gradient
# ---------------------------------------------------------------------------------------------------------

def test_pooled_gradient_against_central_differences():
    """g of the pooled first pass against central differences (step 1e-5 in z) of the pooled F itself.  The difference errs
    by about delta^2 |F'''| / 6 + eps |F| / delta = 1e-10 |F'''| / 6 + 1e-11 |F|, with F of the order 0.1 here; the gate is
    the one tests/test_control_host.py sets for one draw's central differences with idle clamps, 7.3e-11."""
    args = product(9, 20, spread=0.3)
    w = np.linspace(0.5, 2.0, 9)
    z = np.array([0.3, 0.6, 0.45, 0.2])

    def first(zz):
        return dynamics.control_pooled_host(**args, **NONLINEAR, init=4.0 * zz[np.newaxis, :], draw_weights=w, max_iter=0).first_pass

    base = first(z)
    delta, worst = 1e-5, 0.0
    for d in range(4):
        step = np.zeros(4)
        step[d] = delta
        difference = (first(z + step)['F'][0] - first(z - step)['F'][0]) / (2 * delta)
        worst = max(worst, abs(difference - base['g'][0, d]))
    print(f"\npooled gradient: max |g| {np.max(np.abs(base['g'])):.3e}, max |g - central difference| {worst:.3e}, "
          f"gate {GRADIENT_GATE:.1e}")
    assert np.max(np.abs(base['g'])) > 0.01
    assert worst <= GRADIENT_GATE


# ---------------------------------------------------------------------------------------------------------
# 6. it does what it is for
# ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def spread_case():
    args = product(9, 20, spread=0.3)
    own = dynamics.control_host(**args, **NONLINEAR)
    at_mean = dynamics.control_host(**args, **NONLINEAR, init=own.u_mean, max_iter=0).first_pass['F'][:, 0]
    from_mean = dynamics.control_pooled_host(**args, **NONLINEAR, init=own.u_mean, keep='members')
    return args, own, at_mean, from_mean


def test_the_pooled_optimum_beats_the_mean_of_the_optima(spread_case):
    args, own, at_mean, from_mean = spread_case
    w = np.full(9, 1.0 / 9.0)
    cost_at_mean = float(np.sum(w * at_mean))
    assert abs(from_mean.cost_start - cost_at_mean) <= 1e-12 * cost_at_mean
    assert from_mean.cost <= from_mean.cost_start and from_mean.status == optimize.CONVERGED
    centre = dynamics.control_pooled_host(**args, **NONLINEAR)
    assert centre.status == optimize.CONVERGED
    print(f"\nmean of the draws' own optima {np.mean(own.cost):.7f} <= pooled optimum {from_mean.cost:.7f} (from the box "
          f"centre {centre.cost:.7f}, {centre.iterations} iterations) < u_mean under every draw {cost_at_mean:.7f}; "
          f"max |u - u'| {np.max(np.abs(centre.u - from_mean.u)):.2e}")
    assert np.max(np.abs(centre.u - from_mean.u)) <= 1e-6 * 4.0
    assert np.mean(own.cost) <= from_mean.cost < cost_at_mean
    assert np.mean(own.cost) <= centre.cost < cost_at_mean


# ---------------------------------------------------------------------------------------------------------
# 7. weights
# ---------------------------------------------------------------------------------------------------------

def _with_nan_draw(args):
    models = [dict(m, betas=np.concatenate([m['betas'], np.full((1, m['betas'].shape[1]), np.nan)])) for m in args['models']]
    return {**args, 'models': models}


def test_weights_scale_zero_and_nan():
    args = product(6, 20, spread=0.3)
    w = np.array([0.2, 1.0, 0.0, 0.7, 0.4, 1.3])
    kw = dict(**NONLINEAR, starts=2, keep=['members', 'all'])
    res = dynamics.control_pooled_host(**args, **kw, draw_weights=w)
    assert res.status == optimize.CONVERGED and res.iterations > 1
    assert np.array_equal(res.draw_weights, w / w.sum())
    scaled = dynamics.control_pooled_host(**args, **kw, draw_weights=4 * w)
    for key in ('u_all', 'cost_all', 'status_all', 'iterations_all', 'cost_draws', 'members', 'mean', 'bounds', 'cost', 'best_start'):
        assert np.array_equal(res[key], scaled[key]), key
    assert res.cost == dynamics.pooled_sum(res.cost_draws, res.draw_weights)
    assert np.isfinite(res.cost_draws).all() and res.cost_draws.shape == (6,)
    # a last draw with NaN coefficients: weight 0 changes no bit, a positive weight ends non-finite
    extra = _with_nan_draw(args)
    quiet = dynamics.control_pooled_host(**extra, **kw, draw_weights=np.append(w, 0.0))
    for key in ('u', 'cost', 'iterations', 'u_all', 'cost_all', 'iterations_all', 'status_all'):
        assert np.array_equal(quiet[key], res[key]), key
    assert np.array_equal(quiet.cost_draws[:6], res.cost_draws) and np.isnan(quiet.cost_draws[6])
    assert np.array_equal(quiet.mean, res.mean) and np.array_equal(quiet.bounds, res.bounds)
    loud = dynamics.control_pooled_host(**extra, **kw, draw_weights=np.append(w, 0.1))
    assert loud.status == optimize.NON_FINITE and loud.status_all.tolist() == [optimize.NON_FINITE] * 2 and loud.iterations == 0


# ---------------------------------------------------------------------------------------------------------
# 8. downstream
# ---------------------------------------------------------------------------------------------------------

def test_downstream_simulate_expand_and_violations(spread_case):
    args, own, _, from_mean = spread_case
    again = dynamics.simulate_host(**{**_system(args), 'forcing': dynamics.expand_controls(from_mean)}, keep='members')
    assert np.array_equal(again.members, from_mean.members)
    assert np.array_equal(again.first_saturation, from_mean.first_saturation)
    assert np.array_equal(again.bounds, from_mean.bounds)             # uniform weights: evaluate's order statistics
    assert np.array_equal(from_mean.u_mean, from_mean.u) and from_mean.u.shape == (1, 4)
    with pytest.raises(ValueError, match="one control sequence for all draws"):
        dynamics.expand_controls(from_mean, 0)
    assert dynamics.expand_controls(own, 0)['u'].shape == (20,)        # control's results as before
    assert not from_mean.violated.any() and from_mean.violation_share.tolist() == [0.0, 0.0]
    # a ceiling inside the spread of the draws' x0: some draws break it, some do not
    ceiling = float(np.median(from_mean.members[:, 0].max(axis=1)))
    w = np.linspace(1.0, 2.0, 9)
    res = dynamics.control_pooled_host(**args, **NONLINEAR, limits={'x0': (None, ceiling)}, limit_weight=1e-3, draw_weights=w,
                                       keep='members')
    broke = (res.members[:, :, 1:] > np.array([ceiling, np.inf])[np.newaxis, :, np.newaxis]).any(axis=2)
    assert np.array_equal(res.violated, broke) and 0 < int(broke[:, 0].sum()) < 9 and not broke[:, 1].any()
    assert res.violation_share[0] == dynamics.pooled_sum(broke[:, 0].astype(float), w / w.sum()) and res.violation_share[1] == 0.0
    assert 0.0 < res.violation_share[0] < 1.0
    # weighted bounds: quantiles over the draws, members of the ensemble themselves
    assert res.bounds.shape == (2, 21, 2) and np.all(res.bounds[..., 0] <= res.bounds[..., 1])
    assert np.all(res.bounds[..., 0] >= res.members.min(axis=0)) and np.all(res.bounds[..., 1] <= res.members.max(axis=0))


# ---------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------

def test_refusals_name_their_limit():
    args = product(4, 8)
    for text, w in (("must be \\[4\\] numbers, one per draw", np.ones(3)), ("negative or non-finite", np.array([1.0, -0.5, 1.0, 1.0])),
                    ("negative or non-finite", np.array([1.0, np.nan, 1.0, 1.0])), ("negative or non-finite", np.array([1.0, np.inf, 1.0, 1.0])),
                    ("all zero", np.zeros(4))):
        with pytest.raises(ValueError, match=text):
            dynamics.control_pooled_host(**args, **NONLINEAR, draw_weights=w)
        with pytest.raises(ValueError, match=text):                    # before any device is asked for
            dynamics.control_pooled(**args, **NONLINEAR, draw_weights=w, device=object())
    with pytest.raises(ValueError, match="not a state"):              # control's refusals are inherited
        dynamics.control_pooled_host(**args, segments=4, targets={'q': 0.0})
    one = dynamics.control_pooled_host(**args, **NONLINEAR, draws='mean', max_iter=2)
    assert one.cost_draws.shape == (1,) and one.draw_weights.tolist() == [1.0]


# ---------------------------------------------------------------------------------------------------------
# 10. first_trial: the trial half of iteration 0, spelled out
# ---------------------------------------------------------------------------------------------------------

def _first_passing(Ft, F, noise, slope, moved):
    """The Armijo decision lane by lane, numbered as the device's wavefront lanes: 0-30 Newton, 32-62 steepest descent."""
    for half in range(2):
        for i in range(31):
            bound = (F + dynamics.ARMIJO * (slope[half, i] if slope[half, i] < 0 else 0.0)) + dynamics.NOISE * noise
            if moved[half, i] and Ft[half, i] <= bound:
                return 32 * half + i
    return -1


def test_first_trial_is_the_trial_half_of_iteration_0():
    args = product(65, 20, spread=0.3)
    w = 0.25 + np.random.default_rng(3).random(65)
    w[32] = 0.0
    kw = dict(**args, **NONLINEAR, starts=2, draw_weights=w, forcing=None, draws=None, bounds=None, control_bounds=None, weights=None,
              terminal=None, limits=None, limit_weight=1e3, previous=None, init=None, tol=1e-10, keep=None)
    p = dynamics._prepare_control_pooled(**kw, max_iter=1)
    z0 = p['z0'].copy()
    solved = dynamics._control_pooled_solve_host(p)
    first = dynamics._control_pooled_solve_host(dynamics._prepare_control_pooled(**kw, max_iter=0))
    assert 'first_trial' not in first and np.array_equal(p['z0'], z0)  # nothing reaches a trial pass; the start is left alone
    ft, w = solved['first_trial'], p['pool_w']
    S, E, D = 2, 65, 4
    assert ft['trial'].shape == (S, D, 2, 31) and ft['Ft_draws'].shape == (S, E, 2, 31) and ft['Ft'].shape == (S, 2, 31)
    assert ft['reached'].all() and not ft['idle_moved'].any() and np.array_equal(ft['F'], first['first_pass']['F'])
    assert np.array_equal(ft['g'], first['first_pass']['g'])
    for s in range(S):
        for i in range(31):                                            # the steepest-descent half: P(z - 2^-i g)
            assert np.array_equal(ft['trial'][s, :, 1, i], np.clip(z0[s] + 2.0 ** -i * -ft['g'][s], 0.0, 1.0))
        step = ft['trial'][s] - z0[s][:, np.newaxis, np.newaxis]
        slope = np.zeros((2, 31))
        for d in range(D):
            slope = slope + ft['g'][s, d] * step[d]
        assert np.array_equal(ft['slope'][s], slope) and np.array_equal(ft['moved'][s], (step != 0).any(axis=0))
        assert np.isnan(ft['Ft_draws'][s, 32]).all() and np.isfinite(np.delete(ft['Ft_draws'][s], 32, axis=0)).all()
        assert np.array_equal(ft['Ft'][s], dynamics.pooled_sum(ft['Ft_draws'][s], w))
        for half, i, e in ((0, 0, 0), (0, 7, 64), (1, 3, 31), (1, 30, 33)):     # a draw's own cost at a trial point is control's
            own = dynamics._control_pass(p, np.ascontiguousarray(ft['trial'][s, :, half, i][:, np.newaxis]), np.array([e]))['F'][0]
            assert own == ft['Ft_draws'][s, e, half, i]
        lane = _first_passing(ft['Ft'][s], ft['F'][s], ft['noise'][s], ft['slope'][s], ft['moved'][s])
        assert lane == ft['lane'][s] and lane >= 0 and ft['status'][s] == -1 and ft['descent_steps'][s] == (lane >= 32)
        assert np.array_equal(ft['z'][s], ft['trial'][s, :, lane // 32, lane % 32])
    assert np.array_equal(solved['z'], ft['z'])                        # iteration 1 only looks
    public = dynamics.control_pooled_host(**args, **NONLINEAR, starts=2, draw_weights=w, max_iter=1)
    assert 'first_trial' not in public and np.array_equal(public.z.ravel(), ft['z'][public.best_start])

"""dynamics.control_cvar_host, the statement the CVaR-control kernels are tested against (tests/test_control_cvar_gpu.py):
alpha = 0 as control_pooled_host, the smoothed risk against brute force and the exact CVaR against the Rockafellar-Uryasev
minimum, the gradient and the curvature (with its covariance term) against central differences, what the feature is for (a
converged plan with a lower CVaR than the expected-cost plan's), one decision value against a grid, the weights, a
non-finite draw and every refusal -- none of which needs a device."""
import numpy as np
import pytest

from control_cases import linear, mixed, product
from fokl_gpy_amd import dynamics, optimize

NONLINEAR = dict(segments=4, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3})
ALPHAS = (0.5, 0.8, 0.9, 0.98)


def _s_eps(t, eps):
    return np.where(t <= 0, 0.0, np.where(t < eps, t * t / (2 * eps), t - eps / 2))


# ---------------------------------------------------------------------------------------------------------
# 1. alpha = 0 is control_pooled_host
# ---------------------------------------------------------------------------------------------------------

def test_alpha_zero_is_control_pooled_bit_for_bit():
    args = mixed(5, 20)
    kw = dict(segments=4, targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01}, starts=3, keep=['members', 'all'])
    risk, pooled = dynamics.control_cvar_host(**args, **kw, alpha=0.0), dynamics.control_pooled_host(**args, **kw)
    assert set(pooled) <= set(risk) and pooled.iterations > 0
    for key in pooled:
        if isinstance(pooled[key], (list, bool)):
            assert risk[key] == pooled[key], key
        else:
            assert np.array_equal(risk[key], pooled[key], equal_nan=True), key
    assert risk.alpha == 0.0 and risk.expected_cost == pooled.cost and np.array_equal(risk.tail_weights, pooled.draw_weights)
    assert risk.cvar == pytest.approx(pooled.cost, rel=1e-14) and risk.var == pooled.cost_draws.min()
    assert np.isnan(risk.a) and np.isnan(risk.epsilon)
    first = dynamics.control_cvar_host(**args, **kw, alpha=0.0, max_iter=0).first_pass
    want = dynamics.control_pooled_host(**args, **kw, max_iter=0).first_pass
    assert set(first) == set(want) and all(np.array_equal(first[key], want[key]) for key in want)


# ---------------------------------------------------------------------------------------------------------
# 2. the smoothed risk and the exact CVaR
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('alpha', ALPHAS)
@pytest.mark.parametrize('eps', [0.05, 0.002])
def test_cvar_smooth_against_brute_force(alpha, eps):
    rng = np.random.default_rng(11)
    E = 130
    F = 0.5 + rng.random(E) ** 2
    w = 0.25 + rng.random(E)
    w[[7, 64]] = 0.0
    F[7] = np.nan                                                      # a zero weight in front of a NaN cost
    w = w / w.sum()
    m = 1.0 - alpha
    live = w != 0
    phi, a, q, c = dynamics.cvar_smooth(F, w, alpha, eps)
    # the objective on a grid of a between the bracket's ends, then on a finer one between the neighbours of the coarse
    # grid's best point (the objective is convex, so its minimum lies between them): phi is its minimum.  The curvature is
    # at most 1 / (m eps), so the fine grid's best value lies within spacing^2 / (8 m eps) of the minimum
    def objective(grid):
        return grid + (w[live][:, np.newaxis] * _s_eps(F[live][:, np.newaxis] - grid[np.newaxis, :], eps)).sum(axis=0) / m

    coarse = np.linspace(F[live].min() - eps, F[live].max(), 20001)
    at = int(np.argmin(objective(coarse)))
    grid = np.linspace(coarse[max(at - 1, 0)], coarse[min(at + 1, 20000)], 20001)
    values = objective(grid)
    spacing = grid[1] - grid[0]
    print(f"\nalpha {alpha} eps {eps}: phi {phi!r} grid minimum {values.min()!r} at a {grid[np.argmin(values)]!r} (a {a!r}), "
          f"sum q - 1 {q.sum() - 1.0:.2e}")
    assert -1e-12 <= values.min() - phi <= spacing ** 2 / (8 * m * eps) + 1e-12
    assert abs(float(a) + (w[live] * _s_eps(F[live] - a, eps)).sum() / m - phi) <= 1e-12
    assert abs(q.sum() - 1.0) <= 1e-12 and np.all(q >= 0) and q[7] == 0 and q[64] == 0 and c[7] == 0
    assert np.all(q[live] <= w[live] / m * (1 + 1e-15))
    band = live & (F - a > 0) & (F - a < eps)
    assert np.array_equal(c != 0, band) and np.all(c[band] == w[band] / (m * eps))
    # the exact CVaR: the Rockafellar-Uryasev minimum is attained at a data value
    cvar, var = dynamics.cvar_exact(F, w, alpha)
    ru = min(x + (w[live] * np.maximum(F[live] - x, 0.0)).sum() / m for x in F[live])
    assert abs(cvar - ru) <= 1e-12 and var in F[live]
    assert cvar - eps / (2 * m) <= phi <= cvar * (1 + 1e-12)


def test_cvar_exact_ranks_ties_by_index_and_skips_weight_zero():
    F = np.array([3.0, np.nan, 3.0, 1.0, 2.0])
    w = np.array([0.2, 0.0, 0.5, 0.2, 0.1])
    cvar, var = dynamics.cvar_exact(F, w, 0.6)                         # m = 0.4: draw 0 fully, draw 2 (the tie's later index) the rest
    m = 1.0 - 0.6
    assert var == 3.0 and cvar == (0.0 + 0.2 * 3.0 + (m - 0.2) * 3.0) / m
    cvar, var = dynamics.cvar_exact(F, w, 0.1)                         # m = 0.9: draws 0, 2, 4 fully (mass 0.8), draw 3 the rest
    m, before = 1.0 - 0.1, (0.0 + 0.2) + 0.5 + 0.1
    assert var == 1.0 and cvar == ((0.0 + 0.2 * 3.0) + 0.5 * 3.0 + 0.1 * 2.0 + (m - before) * 1.0) / m
    # the sequence matters: spelled in index order of the tie, not the reverse
    F2, w2 = np.array([1.0, 1.0 + 2.0 ** -52, 1.0]), np.array([0.3, 0.3, 0.4])
    cvar, var = dynamics.cvar_exact(F2, w2, 0.5)
    assert var == 1.0 and cvar == ((0.0 + 0.3 * F2[1]) + (0.5 - 0.3) * 1.0) / 0.5
    assert np.isnan(dynamics.cvar_exact(np.array([1.0, np.inf]), np.array([0.5, 0.5]), 0.5)).all()
    # alpha = 0: the weighted mean, the VaR the smallest cost
    cvar, var = dynamics.cvar_exact(np.array([1.0, 2.0, 4.0]), np.array([0.25, 0.25, 0.5]), 0.0)
    assert cvar == 2.75 and var == 1.0
    phi, a, q, c = dynamics.cvar_smooth(np.array([1.0, np.inf]), np.array([0.5, 0.5]), 0.5, 0.1)
    assert np.isnan(phi) and np.isnan(a) and q.tolist() == [0.0, 0.0] and c.tolist() == [0.0, 0.0]
    # every trailing index is a risk of its own
    rng = np.random.default_rng(2)
    F3, w3 = rng.random((70, 3)), np.full(70, 1.0 / 70)
    F3[5, 1] = np.nan
    phi, a, q, c = dynamics.cvar_smooth(F3, w3, 0.9, 0.01)
    for k in (0, 2):
        one = dynamics.cvar_smooth(F3[:, k], w3, 0.9, 0.01)
        assert phi[k] == one[0] and a[k] == one[1] and np.array_equal(q[:, k], one[2]) and np.array_equal(c[:, k], one[3])
    assert np.isnan(phi[1]) and not q[:, 1].any()


# ---------------------------------------------------------------------------------------------------------
# 3. gradient and curvature
# ---------------------------------------------------------------------------------------------------------

GRADIENT_GATE = 1.7e-11    # measured on this statement: max |g - central difference| 1.622e-12 with max |g| = 0.126, x 10
CURVATURE_GATE = 2.5e-9    # measured on this statement: max |H - central difference of g| 2.484e-10 with max |H| = 3.74, x 10


def test_gradient_against_central_differences():
    """g of the first pass against central differences (step 1e-5 in z) of phi itself, on the product system with a soft
    limit and unequal weights.  phi is C1 with a curvature that jumps where a draw enters or leaves the band, so the
    difference errs by about delta |jump| / 2 + eps |phi| / delta next to such a point and by delta^2 |phi'''| / 6 otherwise."""
    args = product(9, 20, spread=0.3)
    w = np.linspace(0.5, 2.0, 9)
    z = np.array([0.3, 0.6, 0.45, 0.2])
    kw = dict(**NONLINEAR, limits={'x1': (None, 0.0)}, limit_weight=1e2, draw_weights=w, alpha=0.8, epsilon=2e-3, max_iter=0)

    def first(zz):
        return dynamics.control_cvar_host(**args, **kw, init=4.0 * zz[np.newaxis, :]).first_pass

    base = first(z)
    delta, worst = 1e-5, 0.0
    for d in range(4):
        step = np.zeros(4)
        step[d] = delta
        difference = (first(z + step)['phi'][0] - first(z - step)['phi'][0]) / (2 * delta)
        worst = max(worst, abs(difference - base['g'][0, d]))
    print(f"\nCVaR gradient: max |g| {np.max(np.abs(base['g'])):.3e}, band draws {int((base['c'] != 0).sum())}, tail draws "
          f"{int((base['q'] != 0).sum())}, max |g - central difference| {worst:.3e}, gate {GRADIENT_GATE:.1e}")
    assert np.max(np.abs(base['g'])) > 0.01 and (base['c'] != 0).any() and 0 < (base['q'] != 0).sum() < 9
    assert worst <= GRADIENT_GATE


def test_curvature_with_the_covariance_term_against_central_differences():
    """On the linear system H_e = 2 J' J is every draw's exact Hessian, so H = sum q H_e + the band draws' covariance of
    gradients is the exact Hessian of phi wherever no draw sits on a band edge: against central differences (step 1e-6 in z)
    of g, at a point where the sets of band and tail draws are the same at z - step, z and z + step.  Without the covariance
    term the difference is of the order of the term itself, which the test also shows."""
    args = linear(130, 12, n_controls=2, spread=0.2)
    K, D = 2, 4
    kw = dict(segments=K, targets={'x0': 0.1 + 0.1 * np.sin(np.arange(13) / 5.0), 'x1': -0.05}, weights={'x0': 1.0, 'x1': 0.5},
              terminal={'x0': 2.0}, move_weight={'u0': 0.01, 'u1': 0.01}, alpha=0.8, epsilon=2e-3, max_iter=0)
    z = np.array([0.35, 0.6, 0.55, 0.4])

    def first(zz):
        return dynamics.control_cvar_host(**args, **kw, init=(-1.0 + 2.0 * zz).reshape(2, K)).first_pass

    base = first(z)
    H = base['H'][0]
    H = np.tril(H) + np.tril(H, -1).T
    plain = np.einsum('e,eij->ij', base['q'][0], np.nan_to_num(base['H_draws'][0]))
    plain = np.tril(plain) + np.tril(plain, -1).T
    delta, worst, without = 1e-6, 0.0, 0.0
    for d in range(D):
        step = np.zeros(D)
        step[d] = delta
        up, down = first(z + step), first(z - step)
        for other in (up, down):                                       # no draw crosses a band edge inside the step
            assert np.array_equal(other['c'] != 0, base['c'] != 0) and np.array_equal(other['q'] != 0, base['q'] != 0)
            assert np.array_equal(other['q'] * 0.2 == 1.0 / 130, base['q'] * 0.2 == 1.0 / 130)
        difference = (up['g'][0] - down['g'][0]) / (2 * delta)
        worst = max(worst, float(np.max(np.abs(difference - H[:, d]))))
        without = max(without, float(np.max(np.abs(difference - plain[:, d]))))
    print(f"\nCVaR curvature: max |H| {np.max(np.abs(H)):.3e}, band draws {int((base['c'] != 0).sum())}, max |H - central "
          f"difference of g| {worst:.3e} (without the covariance term {without:.3e}), gate {CURVATURE_GATE:.1e}")
    assert (base['c'] != 0).sum() >= 3 and without > 1e3 * worst
    assert worst <= CURVATURE_GATE


# ---------------------------------------------------------------------------------------------------------
# 4. what it is for
# ---------------------------------------------------------------------------------------------------------

SYSTEMS = {
    'product': lambda: dict(**product(65, 20, spread=0.3), **NONLINEAR, limits={'x1': (None, 0.0)}, limit_weight=1e2),
    'mixed': lambda: dict(**mixed(33, 20, spread=0.3), segments=4, targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01}),
    'linear': lambda: dict(**linear(130, 12, n_controls=2, spread=0.2), segments=4,
                           targets={'x0': 0.1 + 0.1 * np.sin(np.arange(13) / 5.0), 'x1': -0.05}, weights={'x0': 1.0, 'x1': 0.5},
                           terminal={'x0': 2.0}, move_weight={'u0': 0.01, 'u1': 0.01}),
}
_pooled_plans = {}


def _pooled_plan(name):
    if name not in _pooled_plans:
        _pooled_plans[name] = dynamics.control_pooled_host(**SYSTEMS[name](), starts=2, max_iter=60)
    return _pooled_plans[name]


@pytest.mark.parametrize('alpha', ALPHAS)
@pytest.mark.parametrize('name', list(SYSTEMS))
def test_the_plan_converges_and_lowers_the_cvar_of_the_expected_cost_plan(name, alpha):
    pooled = _pooled_plan(name)
    res = dynamics.control_cvar_host(**SYSTEMS[name](), starts=2, max_iter=60, alpha=alpha, smoothing=0.01)
    pooled_cvar = dynamics.cvar_exact(pooled.cost_draws, pooled.draw_weights, alpha)[0]
    print(f"\n{name} alpha {alpha}: status {res.status} after {res.iterations} iterations, cvar {res.cvar:.7f} (expected-cost plan "
          f"{pooled_cvar:.7f}), expected cost {res.expected_cost:.7f} (expected-cost plan {pooled.cost:.7f}), phi {res.cost:.7f}, "
          f"epsilon {res.epsilon:.3e}")
    assert pooled.status == optimize.CONVERGED
    assert res.status == optimize.CONVERGED
    assert res.cvar < pooled_cvar
    assert res.expected_cost >= pooled.cost
    m = 1.0 - alpha
    assert res.cvar - res.epsilon / (2 * m) <= res.cost <= res.cvar * (1 + 1e-12)
    assert res.epsilon == 0.01 * pooled.cost_start or pooled.best_start != 0
    assert abs(res.tail_weights.sum() - 1.0) <= 1e-12 and res.var <= res.cvar and res.alpha == alpha


# ---------------------------------------------------------------------------------------------------------
# 5. one control, one segment: the solver against a grid
# ---------------------------------------------------------------------------------------------------------

def test_one_decision_value_against_a_grid():
    args = product(9, 20, spread=0.3)
    kw = dict(segments=1, targets={'x0': 0.6, 'x1': -0.2}, draw_weights=np.linspace(0.5, 2.0, 9), alpha=0.8, epsilon=1e-3)
    res = dynamics.control_cvar_host(**args, **kw)
    assert res.status == optimize.CONVERGED and res.z.shape == (1, 1)
    p = dynamics._prepare_control_pooled(args['models'], args['states'], args['inputs'], args['controls'], None, args['y0'],
                                         args['t'], None, None, 1, None, kw['targets'], None, None, None, 1e3, None, None, None,
                                         1, 60, 1e-10, kw['draw_weights'], None)
    grid = np.linspace(0.0, 1.0, 2001)
    F = dynamics._control_pass(p, np.ascontiguousarray(np.tile(grid[np.newaxis, :], (1, 9))), np.repeat(np.arange(9), 2001))['F']
    phi = dynamics.cvar_smooth(F.reshape(9, 2001), p['pool_w'], 0.8, 1e-3)[0]
    best = int(np.argmin(phi))
    print(f"\none decision value: solver z {res.z[0, 0]!r} phi {res.cost!r}; grid minimum {phi[best]!r} at z {grid[best]!r}")
    assert 0 < best < 2000 and abs(res.z[0, 0] - grid[best]) <= grid[1] - grid[0]
    assert res.cost <= phi[best]


# ---------------------------------------------------------------------------------------------------------
# 6. weights and inputs
# ---------------------------------------------------------------------------------------------------------

def _with_nan_draw(args):
    models = [dict(m, betas=np.concatenate([m['betas'], np.full((1, m['betas'].shape[1]), np.nan)])) for m in args['models']]
    return {**args, 'models': models}


def test_weights_scale_zero_nan_and_duplicates():
    args = product(6, 20, spread=0.3)
    w = np.array([0.2, 1.0, 0.0, 0.7, 0.4, 1.3])
    kw = dict(**NONLINEAR, starts=2, keep=['members', 'all'], alpha=0.7)
    res = dynamics.control_cvar_host(**args, **kw, draw_weights=w)
    assert res.status == optimize.CONVERGED and res.iterations > 1
    assert np.array_equal(res.draw_weights, w / w.sum()) and res.tail_weights[2] == 0
    # weights in assimilate's shape: [E], non-negative, summing to 1 -- and any multiple of them
    keys = ('u_all', 'cost_all', 'status_all', 'iterations_all', 'cost_draws', 'members', 'cost', 'best_start', 'cvar', 'var',
            'tail_weights', 'a', 'epsilon', 'expected_cost')
    for other in (w / w.sum(), 4 * w):
        scaled = dynamics.control_cvar_host(**args, **kw, draw_weights=other)
        for key in keys:
            assert np.array_equal(res[key], scaled[key]), key
    # a collapsed draw (weight 0, NaN throughout) changes no bit; with a weight it ends the solve non-finite
    extra = _with_nan_draw(args)
    quiet = dynamics.control_cvar_host(**extra, **kw, draw_weights=np.append(w, 0.0))
    for key in ('u', 'cost', 'iterations', 'u_all', 'cost_all', 'iterations_all', 'status_all', 'cvar', 'var', 'a', 'epsilon'):
        assert np.array_equal(quiet[key], res[key]), key
    assert np.array_equal(quiet.cost_draws[:6], res.cost_draws) and np.isnan(quiet.cost_draws[6]) and quiet.tail_weights[6] == 0
    with pytest.raises(ValueError, match="relative to the pooled cost at the start, which is nan"):
        dynamics.control_cvar_host(**extra, **kw, draw_weights=np.append(w, 0.1))
    loud = dynamics.control_cvar_host(**extra, **kw, draw_weights=np.append(w, 0.1), epsilon=res.epsilon)
    assert loud.status == optimize.NON_FINITE and loud.status_all.tolist() == [optimize.NON_FINITE] * 2 and loud.iterations == 0
    assert np.isnan(loud.cost) and np.isnan(loud.cvar)
    # every draw twice at half its weight: the same risk, up to the rounding of another order of summation
    twice = {**args, 'models': [dict(m, betas=np.concatenate([m['betas'], m['betas']])) for m in args['models']]}
    double = dynamics.control_cvar_host(**twice, **kw, draw_weights=np.concatenate([w, w]), epsilon=res.epsilon)
    assert double.status == optimize.CONVERGED
    assert abs(double.cvar - res.cvar) <= 1e-9 * res.cvar and np.max(np.abs(double.u - res.u)) <= 1e-6 * 4.0


def test_first_pass_fields():
    args = product(9, 20, spread=0.3)
    first = dynamics.control_cvar_host(**args, **NONLINEAR, starts=2, init=np.array([[1.0, 2.5, 0.5, 3.0]]), alpha=0.8,
                                       max_iter=0).first_pass
    assert set(first) == {'phi', 'a', 'g', 'H', 'q', 'c', 'F_draws', 'g_draws', 'H_draws'}
    assert first['phi'].shape == (2,) and first['a'].shape == (2,) and first['g'].shape == (2, 4) and first['H'].shape == (2, 4, 4)
    assert first['q'].shape == (2, 9) and first['c'].shape == (2, 9) and first['F_draws'].shape == (2, 9)
    w = np.full(9, 1.0) / 9.0
    eps = 0.01 * dynamics.pooled_sum(first['F_draws'][0], w)
    for s in range(2):
        phi, a, q, c = dynamics.cvar_smooth(first['F_draws'][s], w, 0.8, eps)
        assert first['phi'][s] == phi and first['a'][s] == a and np.array_equal(first['q'][s], q) and np.array_equal(first['c'][s], c)
        assert np.array_equal(first['g'][s], dynamics.pooled_sum(first['g_draws'][s], q))


# ---------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------

def test_refusals_name_their_limit():
    args = product(4, 8)
    cases = (("alpha must lie in \\[0, 1\\)", dict(alpha=1.0)), ("alpha must lie in \\[0, 1\\)", dict(alpha=-0.01)),
             ("alpha must lie in \\[0, 1\\)", dict(alpha=np.nan)), ("smoothing must be positive and finite", dict(smoothing=0.0)),
             ("smoothing must be positive and finite", dict(smoothing=np.inf)), ("smoothing must be positive and finite", dict(smoothing=np.nan)),
             ("epsilon must be positive and finite", dict(epsilon=0.0)), ("epsilon must be positive and finite", dict(epsilon=-1.0)),
             ("epsilon must be positive and finite", dict(epsilon=np.inf)),
             ("must be \\[4\\] numbers, one per draw", dict(draw_weights=np.ones(3))),
             ("negative or non-finite", dict(draw_weights=np.array([1.0, -0.5, 1.0, 1.0]))), ("all zero", dict(draw_weights=np.zeros(4))))
    for text, change in cases:
        with pytest.raises(ValueError, match=text):
            dynamics.control_cvar_host(**args, **NONLINEAR, **change)
        with pytest.raises(ValueError, match=text):                    # before any device is asked for
            dynamics.control_cvar(**args, **NONLINEAR, **change, device=object())
    with pytest.raises(ValueError, match="not a state"):              # control's refusals are inherited
        dynamics.control_cvar_host(**args, segments=4, targets={'q': 0.0})
    # a relative smoothing needs a scale: only moves are penalised and the start holds every control constant, so the cost is 0
    with pytest.raises(ValueError, match="relative to the pooled cost at the start, which is 0.0"):
        dynamics.control_cvar_host(**args, segments=4, move_weight={'u': 0.01})
    fixed = dynamics.control_cvar_host(**args, segments=4, move_weight={'u': 0.01}, epsilon=1e-3)
    assert fixed.status == optimize.CONVERGED and fixed.iterations == 0 and fixed.cvar == 0.0 and -1e-3 / (2 * 0.1) <= fixed.cost <= 0.0
    with pytest.raises(ValueError, match="alpha must lie in \\(0, 1\\)"):
        dynamics.cvar_smooth(np.ones(3), np.ones(3) / 3, 0.0, 0.1)
    with pytest.raises(ValueError, match="one row per weight"):
        dynamics.cvar_smooth(np.ones(4), np.ones(3) / 3, 0.5, 0.1)
    with pytest.raises(ValueError, match="epsilon must be positive and finite"):
        dynamics.cvar_smooth(np.ones(3), np.ones(3) / 3, 0.5, 0.0)
    with pytest.raises(ValueError, match="alpha must lie in \\[0, 1\\)"):
        dynamics.cvar_exact(np.ones(3), np.ones(3) / 3, 1.0)


# ---------------------------------------------------------------------------------------------------------
# first_trial: the trial half of iteration 0, spelled out
# ---------------------------------------------------------------------------------------------------------

def test_first_trial_is_the_trial_half_of_iteration_0():
    args = product(65, 20, spread=0.3)
    w = 0.25 + np.random.default_rng(3).random(65)
    w[32] = 0.0
    kw = dict(**args, **NONLINEAR, starts=2, draw_weights=w, forcing=None, draws=None, bounds=None, control_bounds=None, weights=None,
              terminal=None, limits=None, limit_weight=1e3, previous=None, init=None, tol=1e-10, keep=None)
    risk = dict(alpha=0.8, smoothing=0.01, epsilon=2e-3)
    p = {**dynamics._prepare_control_pooled(**kw, max_iter=1), **risk}
    solved = dynamics._control_cvar_solve_host(p)
    first = dynamics._control_cvar_solve_host({**dynamics._prepare_control_pooled(**kw, max_iter=0), **risk})
    assert 'first_trial' not in first
    ft, w = solved['first_trial'], p['pool_w']
    assert ft['phi_t'].shape == ft['a_t'].shape == (2, 2, 31) and 'Ft' not in ft and ft['reached'].all()
    assert np.array_equal(ft['F'], first['first_pass']['phi']) and np.array_equal(ft['g'], first['first_pass']['g'])
    for s in range(2):
        for half in range(2):
            for i in range(31):                                        # every trial point's risk is cvar_smooth of its own costs
                phi, a, _, _ = dynamics.cvar_smooth(ft['Ft_draws'][s, :, half, i], w, 0.8, 2e-3)
                assert phi == ft['phi_t'][s, half, i] and a == ft['a_t'][s, half, i]
        bound = (ft['F'][s] + dynamics.ARMIJO * np.where(ft['slope'][s] < 0, ft['slope'][s], 0.0)) + dynamics.NOISE * ft['noise'][s]
        ok = (ft['moved'][s] & (ft['phi_t'][s] <= bound)).ravel()
        lane = int(np.argmax(ok)) + int(np.argmax(ok) >= 31)
        assert ok.any() and lane == ft['lane'][s] and np.array_equal(ft['z'][s], ft['trial'][s, :, lane // 32, lane % 32])
        assert np.isnan(ft['Ft_draws'][s, 32]).all() and ft['status'][s] == -1
    assert np.array_equal(solved['z'], ft['z'])
    # alpha = 0 is the pooled solve's first_trial
    zero = dynamics._run_control_cvar_host({**p, 'alpha': 0.0})[0]['first_trial']
    pooled = dynamics._control_pooled_solve_host(p)['first_trial']
    assert set(zero) == set(pooled) and all(np.array_equal(zero[key], pooled[key], equal_nan=True) for key in pooled)

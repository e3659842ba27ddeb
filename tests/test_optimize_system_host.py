"""Constrained optimisation over a system of models without a device: the host statement (optimize.optimize_system_host,
what the kernel is tested against) on problems with known answers, against optimize_host where it must reduce to it,
against a grid and against scipy's SLSQP; the assembly of the results; every refusal before a context is asked for."""
import numpy as np
import pytest

from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd import optimize as opt

PHIS = getKernels.bernoulli()
BERN = 'Bernoulli Polynomials'
MINMAX = [[0.0, 2.0], [-1.0, 3.0]]
TOY_MTX = np.array([[1, 0], [0, 1], [2, 0], [0, 2], [1, 1], [3, 0], [0, 3], [2, 1], [1, 2], [4, 0], [0, 4], [3, 2]])
TOY_MEAN = np.array([0.3, 0.8, -0.5, 1.5, -1.2, 0.9, 0.7, -0.6, 0.5, 0.4, -2.0, 1.6, 0.8])
UNIT = [[0.0, 1.0], [0.0, 1.0]]


def poly(order):
    return np.polynomial.Polynomial(PHIS[order - 1])


def phi(order, x, d=0):
    """Bernoulli basis `order` at normalised x (numpy's polynomial arithmetic: independent of the solver's Horner)."""
    return poly(order).deriv(d)(x) if d else poly(order)(x)


def as_model(betas, mtx, minmax):
    return dict(betas=np.asarray(betas, dtype=float), mtx=np.atleast_2d(mtx), phis=PHIS, minmax=minmax, kernel=BERN)


def value(model, x, d=None):
    """The model (or its derivative with respect to input d) of the FIRST row of betas at true-scale points x [..., m]."""
    betas, mtx = np.atleast_2d(model['betas'])[0], model['mtx']
    low = np.array([mm[0] for mm in model['minmax']], dtype=float)
    span = np.array([mm[1] for mm in model['minmax']], dtype=float) - low
    xn = (np.asarray(x, dtype=float) - low) / span
    out = np.full(xn.shape[:-1], 0.0 if d is not None else betas[0])
    for t, row in enumerate(mtx):
        term = np.ones(xn.shape[:-1])
        for j, order in enumerate(row):
            if order:
                term = term * (phi(int(order), xn[..., j], 1) / span[j] if j == d else phi(int(order), xn[..., j]))
            elif j == d:
                term = term * 0.0
        out = out + betas[t + 1] * term
    return out


def toy_betas(draws=1, seed=3):
    rng = np.random.default_rng(seed)
    return TOY_MEAN * (1 + 0.1 * rng.standard_normal((draws, TOY_MEAN.shape[0])))


class _Reached(Exception):
    pass


class _NoDevice(_capi.DeviceContext):
    """Stands where the device context would be: the CPU tests end here, after every check that needs no device."""

    def __init__(self):
        self._h = None

    def system_optimize(self, p):
        raise _Reached(p)


# ---------------------------------------------------------------------------------------------------------
# 1. one model, no constraint: optimize_host, iterate for iterate
# ---------------------------------------------------------------------------------------------------------

def wide_model(seed=5):
    rng = np.random.default_rng(seed)
    rows = [np.eye(4, dtype=int)[j] * order for j in range(4) for order in (1, 2, 3)]
    for width in (2, 3, 4):
        for _ in range(4):
            row = np.zeros(4, dtype=int)
            row[rng.choice(4, width, replace=False)] = rng.integers(1, 4, width)
            rows.append(row)
    rows.append(np.zeros(4, dtype=int))
    mtx = np.array(rows)
    return mtx, rng.standard_normal(mtx.shape[0] + 1)


@pytest.mark.parametrize('sense', ['max', 'min'])
def test_one_model_without_constraints_is_optimize_host(sense):
    cases = [(toy_betas(6), TOY_MTX, MINMAX, None, None),
             (toy_betas(3, seed=8), TOY_MTX, MINMAX, [[0.5, 1.5], [1.0, 1.0]], {'a': (0.5, 1.5), 'b': (1.0, 1.0)})]
    mtx, mean = wide_model()
    minmax4 = [[-1.0, 1.0], [0.0, 4.0], [2.0, 3.0], [0.0, 1.0]]
    cases.append((mean * (1 + 0.1 * np.random.default_rng(2).standard_normal((4, mean.shape[0]))), mtx, minmax4, None, None))
    for betas, mtx, minmax, box, bounds in cases:
        names = list('abcd')[:mtx.shape[1]]
        one = opt.optimize_host(betas, mtx, PHIS, minmax, sense=sense, bounds=box, starts=12, max_iter=60, tol=1e-10,
                                ReturnAll=True)
        both = opt.optimize_system_host([as_model(betas, mtx, minmax)], [names], ['y'], 'y', sense=sense, bounds=bounds,
                                        starts=12, max_iter=60, tol=1e-10, ReturnAll=True)
        assert np.max(np.abs(both.x_array - one.x)) <= 1e-12 and np.max(np.abs(both.f - one.f)) <= 1e-12
        assert np.array_equal(both.status, one.status) and np.array_equal(both.status_all, one.status_all)
        assert np.array_equal(both.iterations_all, one.iterations_all) and np.array_equal(both.x_all, one.x_all)
        assert np.array_equal(both.f_bounds, one.f_bounds) and np.array_equal(both.x_bounds, one.x_bounds)
        assert np.all(both.violation == 0.0) and both.multipliers == {} and np.array_equal(both.y['y'], both.f)


# ---------------------------------------------------------------------------------------------------------
# 2. hand-built systems with closed-form answers
# ---------------------------------------------------------------------------------------------------------

def disk_problem(level, **kw):
    """max a . phi_1(x) over the unit square under phi_2(x_1) + phi_2(x_2) <= level: a linear objective over a disk."""
    a = np.array([3.0, 4.0])
    linear = as_model([0.5, a[0], a[1]], [[1, 0], [0, 1]], UNIT)
    disk = as_model([0.0, 1.0, 1.0], [[2, 0], [0, 2]], UNIT)
    res = opt.optimize_system_host([linear, disk], [['u', 'v'], ['u', 'v']], ['gain', 'load'], 'gain',
                                   constraints={'load': (None, level)}, starts=8, ReturnAll=True, **kw)
    return a, res


def test_linear_objective_under_an_active_quadratic_inequality():
    q0, q1, q2 = PHIS[1]                                              # phi_2 = q2 (x - c)^2 + bottom
    c, bottom = -q1 / (2 * q2), q0 - q1 * q1 / (4 * q2)
    radius = 0.3
    level = 2 * bottom + q2 * radius ** 2
    a, res = disk_problem(level)
    slope = PHIS[0][1]                                                # phi_1' : the objective's gradient is slope * a
    direction = a / np.hypot(*a)
    assert np.all(res.status_all == opt.CONVERGED) and res.status.tolist() == [0]
    assert np.allclose(res.x_array[0], c + radius * direction, atol=1e-7, rtol=0)
    assert abs(res.y['load'][0] - level) <= 1e-8 * res.multipliers_all.shape[0] and res.violation[0] <= 1e-8
    # stationarity: -slope a + mu 2 q2 (x - c) = 0
    assert abs(res.multipliers['load'][0] - slope * np.hypot(*a) / (2 * q2 * radius)) <= 1e-6
    assert abs(res.f[0] - (0.5 + a @ phi(1, c + radius * direction))) <= 1e-7
    assert res.x['u'][0] == res.x_array[0, 0] and res.variables == ['u', 'v'] and res.constraint_names == ['load']


def test_an_inactive_inequality_leaves_the_box_corner_and_no_multiplier():
    a, res = disk_problem(5.0)
    assert res.x_array.tolist() == [[1.0, 1.0]] and res.multipliers['load'].tolist() == [0.0]
    assert np.all(res.status_all == opt.CONVERGED) and np.all(res.multipliers_all == 0.0) and res.violation[0] == 0.0
    # a lower limit that holds everywhere is as silent; a two-sided range reports the side that binds, with its sign
    lo = opt.optimize_system_host([as_model([0.5, 3.0, 4.0], [[1, 0], [0, 1]], UNIT), as_model([0.0, 1.0, 1.0],
                                  [[2, 0], [0, 2]], UNIT)], [['u', 'v']] * 2, ['gain', 'load'], 'gain', sense='min',
                                  constraints={'load': (-5.0, 5.0)}, starts=4)
    assert lo.x_array.tolist() == [[0.0, 0.0]] and lo.multipliers['load'].tolist() == [0.0]
    floor = opt.optimize_system_host([as_model([0.0, 1.0, 1.0], [[2, 0], [0, 2]], UNIT)], [['u', 'v']], ['load'], 'load',
                                     sense='min', constraints={'load': (0.0, 5.0)}, starts=4)
    assert floor.status.tolist() == [0] and abs(floor.f[0]) <= 1e-8 and floor.multipliers['load'][0] < -0.5


def test_a_pinned_output_is_the_root_of_the_model():
    betas = [0.2, 1.0, 0.3]                                           # phi_1 + 0.3 phi_3: increasing on [0, 1]
    grid = np.linspace(0, 1, 201)
    assert np.all(betas[1] * phi(1, grid, 1) + betas[2] * phi(3, grid, 1) > 0)
    curve = as_model(betas, [[1], [3]], [[10.0, 30.0]])
    target = 0.35
    res = opt.optimize_system_host([curve], [['T']], ['y'], 'T', constraints={'y': (target, target)}, starts=5,
                                   ReturnAll=True)
    whole = betas[0] + betas[1] * poly(1) + betas[2] * poly(3) - target
    roots = [r.real for r in whole.roots() if abs(r.imag) < 1e-12 and 0 <= r.real <= 1]
    assert len(roots) == 1 and np.all(res.status_all == opt.CONVERGED)
    assert abs(res.x['T'][0] - (10.0 + 20.0 * roots[0])) <= 1e-6 and abs(res.y['y'][0] - target) <= 1e-7
    assert res.f[0] == res.x['T'][0] and np.ptp(res.x_all) <= 1e-6


def test_a_fixed_variable_stays_fixed():
    a, free = disk_problem(5.0)
    linear = as_model([0.5, 3.0, 4.0], [[1, 0], [0, 1]], [[0.0, 1.0], [2.0, 6.0]])
    disk = as_model([0.0, 1.0, 1.0], [[2, 0], [0, 2]], [[0.0, 1.0], [2.0, 6.0]])
    res = opt.optimize_system_host([linear, disk], [['u', 'v']] * 2, ['gain', 'load'], 'gain', bounds={'v': (3.3, 3.3)},
                                   constraints={'load': (None, 0.0)}, starts=6, ReturnAll=True)
    assert np.all(res.x_all[..., 1] == 3.3) and res.x['v'].tolist() == [3.3] and res.status.tolist() == [0]
    assert abs(res.y['load'][0]) <= 1e-7 and 0.5 < res.x['u'][0] < 1.0 and abs(value(disk, [res.x['u'][0], 3.3]) - res.y['load'][0]) <= 1e-12


# ---------------------------------------------------------------------------------------------------------
# 3. composition: one model's output is another's input
# ---------------------------------------------------------------------------------------------------------

def chain_models():
    inner = as_model([1.0, 0.8, -0.5, 0.3], [[1], [2], [3]], [[100.0, 500.0]])                  # y1 = f(x)
    outer = as_model([0.2, 0.6, -0.9, 0.7, -0.8, 0.5], [[1, 0], [2, 0], [0, 1], [0, 2], [1, 1]],
                     [[50.0, 600.0], [0.0, 2.5]])                                                # g(x, y1)
    return inner, outer


def test_an_intermediate_is_tied_to_its_model():
    inner, outer = chain_models()
    res = opt.optimize_system_host([inner, outer], [['x'], ['x', 'y1']], ['y1', 'g'], 'g', starts=16, ctol=1e-11,
                                   ReturnAll=True)
    assert res.variables == ['x', 'y1'] and res.constraint_names == ['tie:y1'] and res.status.tolist() == [0]
    grid = np.linspace(100.0, 500.0, 400001)
    h = value(outer, np.stack([grid, value(inner, grid[:, None])], axis=-1))
    best = np.argmax(h)
    from scipy.optimize import minimize_scalar
    fine = minimize_scalar(lambda x: -value(outer, np.array([x, value(inner, np.array([x]))])), method='bounded',
                           bounds=(grid[max(best - 1, 0)], grid[min(best + 1, grid.size - 1)]), options=dict(xatol=1e-10))
    top = max(-fine.fun, h[best])                                     # the grid holds the ends of the range exactly
    assert abs(res.f[0] - top) <= 1e-9 and abs(res.x['x'][0] - fine.x) <= 1e-3
    assert abs(res.y['y1'][0] - res.x['y1'][0]) <= 1e-11 * np.sum(np.abs(inner['betas'])) and res.violation[0] <= 1e-11
    assert abs(res.y['y1'][0] - value(inner, [res.x['x'][0]])) <= 1e-12
    # the intermediate's box: the consuming model's training range; the shared input's: the intersection
    with pytest.raises(_Reached) as hit:
        opt.optimize_system([inner, outer], [['x'], ['x', 'y1']], ['y1', 'g'], 'g', device=_NoDevice())
    p = hit.value.args[0]
    assert p['box'].tolist() == [[100.0, 500.0], [0.0, 2.5]] and p['lo'].tolist() == [0.0, 0.0] and p['hi'].tolist() == [1.0, 1.0]
    assert p['shift'][0].tolist() == [0.0] and p['slope'][0].tolist() == [1.0]
    assert np.allclose(p['shift'][1], [50.0 / 550.0, 0.0]) and np.allclose(p['slope'][1], [400.0 / 550.0, 1.0])


# ---------------------------------------------------------------------------------------------------------
# 4. an independent solver
# ---------------------------------------------------------------------------------------------------------

def test_two_models_three_variables_one_inequality_against_slsqp():
    from scipy.optimize import minimize
    rng = np.random.default_rng(12)
    mtx_a = np.array([[1, 0], [0, 1], [2, 0], [0, 2], [1, 1], [3, 1]])
    mtx_b = np.array([[1, 0], [0, 1], [2, 0], [0, 2], [2, 1]])
    gain = as_model(rng.standard_normal(7), mtx_a, [[0.0, 1.0], [-2.0, 2.0]])                   # reads p, q
    waste = as_model(np.concatenate([[0.0], rng.standard_normal(5)]), mtx_b, [[-1.0, 3.0], [5.0, 9.0]])   # reads q, r
    limit = 0.1
    res = opt.optimize_system_host([gain, waste], [['p', 'q'], ['q', 'r']], ['gain', 'waste'], 'gain',
                                   constraints={'waste': (None, limit)}, starts=48)
    assert res.variables == ['p', 'q', 'r'] and res.status.tolist() == [0] and res.violation[0] <= 1e-8
    fun = lambda z: -float(value(gain, z[[0, 1]]))
    jac = lambda z: -np.array([value(gain, z[[0, 1]], 0), value(gain, z[[0, 1]], 1), 0.0])
    con = dict(type='ineq', fun=lambda z: limit - float(value(waste, z[[1, 2]])),
               jac=lambda z: -np.array([0.0, value(waste, z[[1, 2]], 0), value(waste, z[[1, 2]], 1)]))
    box = [(0.0, 1.0), (-1.0, 2.0), (5.0, 9.0)]                        # q: the intersection of [-2, 2] and [-1, 3]
    best = np.inf
    for start in opt.start_points(48, np.array([b[0] for b in box]), np.array([b[1] for b in box])):
        out = minimize(fun, start, jac=jac, bounds=box, constraints=[con], method='SLSQP', options=dict(ftol=1e-14, maxiter=300))
        if out.success and con['fun'](out.x) >= -1e-9:
            best = min(best, out.fun)
    assert abs(res.f[0] + best) <= 1e-7, (res.f[0], -best)
    assert value(waste, [res.x['q'][0], res.x['r'][0]]) <= limit + 1e-8 * np.sum(np.abs(waste['betas']))
    assert -1.0 <= res.x['q'][0] <= 2.0


# ---------------------------------------------------------------------------------------------------------
# 5. infeasible problems and starts
# ---------------------------------------------------------------------------------------------------------

def test_an_unreachable_limit_reports_infeasible_and_the_least_violating_point():
    disk = as_model([0.0, 1.0, 1.0], [[2, 0], [0, 2]], UNIT)
    res = opt.optimize_system_host([disk], [['u', 'v']], ['load'], 'u', constraints={'load': (None, -1.0)}, starts=6,
                                   ReturnAll=True)
    assert res.status.tolist() == [opt.INFEASIBLE] and np.all(res.status_all == opt.INFEASIBLE)
    assert res.violation[0] > 1e-8 and opt.STATUS_TEXT[opt.INFEASIBLE] == 'infeasible'
    c = -PHIS[1][1] / (2 * PHIS[1][2])                                # the disk's centre: the smallest load there is
    assert np.allclose(res.x_array[0], [c, c], atol=1e-6)
    assert abs(res.violation[0] - (value(disk, [c, c]) + 1.0) / 2.0) <= 1e-9       # scaled by sum |betas| = 2


def test_the_only_feasible_start_is_picked():
    toy = as_model(toy_betas(1)[0], TOY_MTX, MINMAX)
    kw = dict(sense='max', constraints={'y': (0.2, 0.2)}, ReturnAll=True)
    scan = opt.optimize_system_host([toy], [['u', 'v']], ['y'], 'u', starts=24, **kw)
    ok = scan.violation_all[0] <= 1e-8
    assert ok.any() and (~ok).any()                                   # the level set is reached from some starts only
    starts = np.concatenate([scan.x_all[0][~ok][:2], scan.x_all[0][ok][:1], scan.x_all[0][~ok][:1]])
    # start from where the infeasible solves began, not from where they ended
    begun = opt.start_points(24, np.zeros(2), np.ones(2)) * [2.0, 4.0] + [0.0, -1.0]
    starts = np.concatenate([begun[~ok][:2], begun[ok][:1], begun[~ok][2:3]])
    res = opt.optimize_system_host([toy], [['u', 'v']], ['y'], 'u', starts=starts, **kw)
    assert (res.violation_all[0] <= 1e-8).tolist() == [False, False, True, False]
    assert res.best_start.tolist() == [2] and res.status.tolist() == [0] and res.violation[0] <= 1e-8
    assert res.status_all[0, [0, 1, 3]].tolist() == [opt.INFEASIBLE] * 3
    # with no feasible start at all: status 4 and the least violating of them
    none = opt.optimize_system_host([toy], [['u', 'v']], ['y'], 'u', starts=starts[[0, 1, 3]], **kw)
    assert none.status.tolist() == [opt.INFEASIBLE] and none.best_start.tolist() == [int(np.argmin(none.violation_all[0]))]


# ---------------------------------------------------------------------------------------------------------
# 6. draws, bands, the random stream
# ---------------------------------------------------------------------------------------------------------

def test_draws_are_paired_broadcast_or_averaged():
    rng = np.random.default_rng(4)
    inner, outer = chain_models()
    many = dict(outer, betas=outer['betas'] * (1 + 0.05 * rng.standard_normal((40, 6))))
    res = opt.optimize_system_host([inner, many], [['x'], ['x', 'y1']], ['y1', 'g'], 'g', starts=6)
    assert res.f.shape == (40,) and res.x_array.shape == (40, 2) and res.y['y1'].shape == (40,)
    for e in (0, 17, 39):                                             # draw e is the system of row e (and the single row)
        alone = opt.optimize_system_host([inner, dict(outer, betas=many['betas'][e])], [['x'], ['x', 'y1']], ['y1', 'g'],
                                         'g', starts=6, scales={'y1': float(np.sum(np.abs(inner['betas'])))})
        assert alone.f[0] == res.f[e] and np.array_equal(alone.x_array[0], res.x_array[e])
    cut = opt.bounds_cut(40)
    assert np.array_equal(res.f_bounds, np.sort(res.f)[[cut, 40 - cut]])
    assert np.array_equal(res.x_bounds, np.sort(res.x_array, axis=0)[[cut, 40 - cut]].T)
    assert res.f_mean == res.f.mean() and np.array_equal(res.x_mean, res.x_array.mean(axis=0))
    plain = opt.optimize_system_host([inner, many], [['x'], ['x', 'y1']], ['y1', 'g'], 'g', starts=6, ReturnBounds=False)
    assert 'f_bounds' not in plain and np.array_equal(plain.f, res.f)
    mean = opt.optimize_system_host([inner, many], [['x'], ['x', 'y1']], ['y1', 'g'], 'g', starts=6, draws='mean')
    one = opt.optimize_system_host([inner, dict(outer, betas=many['betas'].mean(axis=0))], [['x'], ['x', 'y1']],
                                   ['y1', 'g'], 'g', starts=6)
    assert isinstance(mean.f, float) and mean.f == one.f[0] and mean.x['x'] == one.x['x'][0] and mean.status == 0
    assert 'f_bounds' not in mean and mean.x_array.shape == (2,)
    with pytest.raises(ValueError, match='same number of draws'):
        opt.optimize_system_host([dict(inner, betas=np.tile(inner['betas'], (7, 1))), many], [['x'], ['x', 'y1']],
                                 ['y1', 'g'], 'g', starts=6)


def test_numpys_random_stream_does_not_move():
    np.random.seed(11)
    before = np.random.get_state()
    inner, outer = chain_models()
    opt.optimize_system_host([inner, outer], [['x'], ['x', 'y1']], ['y1', 'g'], 'g', starts=8)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


# ---------------------------------------------------------------------------------------------------------
# 7. refusals: all of them before a context is asked for
# ---------------------------------------------------------------------------------------------------------

class _Untouchable:
    """A device argument that fails the test if anything is asked of it."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for {name} before the arguments were checked")


def test_refusals_come_before_the_device():
    inner, outer = chain_models()
    args = ([inner, outer], [['x'], ['x', 'y1']], ['y1', 'g'], 'g')
    kw = dict(device=_Untouchable())
    spline = dict(inner, kernel='Cubic Splines', phis=getKernels.table_to_phis(np.zeros((2, 4, 499))))
    with pytest.raises(ValueError, match='Cubic Splines'):
        opt.optimize_system([spline, outer], *args[1:], **kw)
    wide = as_model(np.ones(2), np.ones((1, 17), dtype=int), [[0, 1]] * 17)
    with pytest.raises(ValueError, match='at most 16 decision variables'):
        opt.optimize_system([wide], [[f'x{j}' for j in range(17)]], ['y'], 'y', **kw)
    with pytest.raises(ValueError, match='1 to 8 models'):
        opt.optimize_system([inner] * 9, [['x']] * 9, [f'y{k}' for k in range(9)], 'y0', **kw)
    with pytest.raises(ValueError, match="variable 'x'.*no point in common"):
        opt.optimize_system(*args, bounds={'x': (520.0, 550.0)}, **kw)
    apart = dict(outer, minmax=[[501.0, 600.0], [0.0, 2.5]])
    with pytest.raises(ValueError, match="variable 'x'"):
        opt.optimize_system([inner, apart], *args[1:], **kw)
    with pytest.raises(ValueError, match="objective 'h'"):
        opt.optimize_system(*args[:3], 'h', **kw)
    with pytest.raises(ValueError, match="constraints: 'x' is not a model output"):
        opt.optimize_system(*args, constraints={'x': (0, 1)}, **kw)
    with pytest.raises(ValueError, match="bounds: 'g' is not a decision variable"):
        opt.optimize_system(*args, bounds={'g': (0, 1)}, **kw)
    with pytest.raises(ValueError, match='above the upper'):
        opt.optimize_system(*args, bounds={'x': (300.0, 200.0)}, **kw)
    with pytest.raises(ValueError, match='above the upper'):
        opt.optimize_system(*args, constraints={'g': (1.0, 0.0)}, **kw)
    with pytest.raises(ValueError, match='scales'):
        opt.optimize_system(*args, scales={'g': 0.0}, **kw)
    with pytest.raises(ValueError, match='one entry per model'):
        opt.optimize_system([inner, outer], [['x']], ['y1', 'g'], 'g', **kw)
    with pytest.raises(ValueError, match='inputs, xvars'):
        opt.optimize_system([inner, outer], [['x'], ['x']], ['y1', 'g'], 'g', **kw)
    with pytest.raises(ValueError, match='twice'):
        opt.optimize_system([inner, outer], [['x'], ['x', 'x']], ['y1', 'g'], 'g', **kw)
    with pytest.raises(ValueError, match='draws must be'):
        opt.optimize_system(*args, draws='all', **kw)
    with pytest.raises(ValueError, match='sense'):
        opt.optimize_system(*args, sense='largest', **kw)
    with pytest.raises(ValueError, match='starts'):
        opt.optimize_system(*args, starts=np.zeros((4, 3)), **kw)
    with pytest.raises(ValueError, match='at most'):
        opt.optimize_system([dict(inner, betas=np.ones((1 << 15, 4))), outer], *args[1:], starts=64, **kw)
    # the LDS budget: 16 variables with three orders each are 3 x 48 + 136 + 48 + 2 = 330 values, 288 fit
    rows = [np.eye(16, dtype=int)[j] * order for j in range(16) for order in (1, 2, 3)]
    big = as_model(np.ones(49), np.array(rows), [[0, 1]] * 16)
    with pytest.raises(ValueError, match='330 values per solve.*hold 288'):
        opt.optimize_system([big], [[f'x{j}' for j in range(16)]], ['y'], 'y', **kw)
    assert opt.system_lds_rows(48, 16, 1, 0) == 330
    # three two-way models over eight variables with three orders per input fit: 3 x 24 + 36 + 24 + 6 + 2 x 5
    assert opt.system_lds_rows(24, 8, 3, 5) == 148 <= opt.LDS_ROWS
    # what reaches the context when nothing is refused
    with pytest.raises(_Reached) as hit:
        opt.optimize_system(*args, constraints={'g': (None, 0.4)}, bounds={'x': (150.0, None)}, device=_NoDevice())
    p = hit.value.args[0]
    assert [c['name'] for c in p['cons']] == ['tie:y1', 'g'] and [c['model'] for c in p['cons']] == [0, 1]
    assert p['cons'][1]['lo'] == -np.inf and p['cons'][1]['hi'] == 0.4 and p['box'][0].tolist() == [150.0, 500.0]
    assert p['cons'][0]['scale'] == np.sum(np.abs(inner['betas'])) and p['coef'].shape == (1, 10)

"""dynamics.control_host, the statement the device kernel is tested against (tests/test_control_gpu.py): its tangent pass
against central differences of simulate_host, a linear-quadratic problem against scipy's bounded least squares, the
definitions of its statuses on a nonlinear system, the trajectory under the returned controls, its invariances, the soft
limits and every refusal -- none of which needs a device."""
import numpy as np
import pytest
from scipy.optimize import lsq_linear

from control_cases import BERN, chain, linear, mixed, product
from fokl_gpy_amd import _capi, dynamics, optimize


def _forcing(args, res, e=None):
    return {**(args.get('forcing') or {}), **dynamics.expand_controls(res, e)}


def _system(args):
    return {key: value for key, value in args.items() if key != 'controls'}


def _trajectory(args, z, lo, width, seg_of, **kw):
    """simulate_host's trajectory [n_states, P] of draw 0 under the controls lo + z width."""
    u = lo[:, np.newaxis] + z.reshape(lo.shape[0], -1) * width[:, np.newaxis]
    forcing = {**(args.get('forcing') or {}), **{name: u[c][seg_of] for c, name in enumerate(args['controls'])}}
    return dynamics.simulate_host(**{**_system(args), 'forcing': forcing}, ReturnBounds=False, keep='members', **kw).members[0]


# ---------------------------------------------------------------------------------------------------------
# 1. tangents
# ---------------------------------------------------------------------------------------------------------

TANGENT_CASES = {
    # every clamp idle
    'idle': (dict(), 7.3e-11),
    # T starts beyond the range its reader was trained on (its normalised value is clamped throughout), and c starts on the
    # lower edge of its box with a negative slope (the slope rule holds it there)
    'clamp and slope rule': (dict(y0=[2.3, -0.2], bounds=[[-3.0, 3.0], [-2.0, -0.2]]), 4.0e-10),
}


@pytest.mark.parametrize('case', list(TANGENT_CASES))
def test_tangent_pass_against_central_differences(case):
    """The Jacobian d y_j(p) / d z_d of the tangent pass against central differences (step 1e-5 in z) of simulate_host
    trajectories, on a spline + Bernoulli system with two-way terms and a forcing column.  The tangent of y_j(p) is read
    from the public surface: with only (j, p) tracked, weight 1 and target y_j(p) - 1, the first pass's g is 2 h r t
    with r = 1 up to its rounding.

    The central difference itself errs by about delta^2 |y'''| / 6 + eps |y| / delta = 1e-10 |y'''| / 6 + 1e-11 |y|.
    Measured on this host, max |J - difference| over all states, points and directions: 7.3e-12 ('idle') and 4.0e-11
    ('clamp and slope rule'), with max |J| = 0.076 and 0.082; the gates are 10 x that: 7.3e-11 and 4.0e-10."""
    extra, gate = TANGENT_CASES[case]
    extra = dict(extra)
    box = extra.pop('bounds', None)
    args = {**mixed(1, 12), **extra}
    z = np.array([0.3, 0.6, 0.45])
    h, delta, P = args['t'][2], 1e-5, 13
    lo, width = np.array([0.0]), np.array([10.0])
    seg_of = np.repeat(np.arange(3), 4)
    y = _trajectory(args, z, lo, width, seg_of, bounds=box)
    probe = dynamics.control_host(**args, bounds=box, segments=3, targets={'T': 0.0}, init=lo[:, None] + z[None, :] * width[:, None],
                                  max_iter=0, keep='members')
    assert np.array_equal(probe.members[0], y)
    assert (probe.first_saturation[0] == -1) == (case == 'idle')
    if case != 'idle':
        assert probe.first_saturation[0] == 0 and np.all(y[0] > 2.0) and np.all(y[1] == -0.2)
    J = np.zeros((2, P, 3))
    for j, name in enumerate(args['states']):
        for point in range(1, P):
            target = np.full(P, np.nan)
            target[point] = y[j, point] - 1.0
            first = dynamics.control_host(**args, bounds=box, segments=3, targets={name: target},
                                          init=lo[:, None] + z[None, :] * width[:, None], max_iter=0).first_pass
            r = y[j, point] - target[point]                           # 1 up to its rounding
            assert first['F'][0, 0] == (h * r) * r
            J[j, point] = first['g'][0, 0] / (2.0 * h * r)
    worst = 0.0
    for d in range(3):
        step = np.zeros(3)
        step[d] = delta
        up, down = _trajectory(args, z + step, lo, width, seg_of, bounds=box), _trajectory(args, z - step, lo, width, seg_of, bounds=box)
        if case != 'idle':                                            # the same clamps act at the perturbed points
            assert np.all(up[0] > 2.0) and np.all(down[0] > 2.0) and np.all(up[1] == -0.2) and np.all(down[1] == -0.2)
        worst = max(worst, float(np.max(np.abs((up - down) / (2 * delta) - J[:, :, d]))))
    print(f"\ntangents ({case}): max |J| {np.max(np.abs(J)):.3e}, max |J - central difference| {worst:.3e}, gate {gate:.1e}")
    assert np.max(np.abs(J)) > 0.05
    assert worst <= gate


# ---------------------------------------------------------------------------------------------------------
# 2. linear-quadratic problems against scipy.optimize.lsq_linear
# ---------------------------------------------------------------------------------------------------------

def _lq(D, steps, amplitude, move, box=None, previous=None, n_controls=1):
    """-> (control_host's result, the exact minimiser and its cost from the affine residual map built from simulate_host)"""
    args = linear(1, steps, n_controls)
    nc, K = n_controls, D // n_controls
    names = args['controls']
    track = {'x0': 0.1 + amplitude * np.sin(np.arange(steps + 1) / 5.0), 'x1': -0.05}
    weights, terminal = {'x0': 1.0, 'x1': 0.5}, {'x0': 2.0}
    kw = dict(segments=K, targets=track, weights=weights, terminal=terminal, control_bounds=box,
              move_weight={name: move for name in names} if move else None, previous=previous)
    res = dynamics.control_host(**args, **kw, max_iter=60, tol=1e-10)
    lo = np.array([(box or {}).get(name, (-1.0, 1.0))[0] for name in names])
    width = np.array([(box or {}).get(name, (-1.0, 1.0))[1] for name in names]) - lo
    seg_of = np.searchsorted(res.segment_first, np.arange(steps), side='right') - 1
    h, P = args['t'][2], steps + 1

    def residuals(z):
        y = _trajectory(args, z, lo, width, seg_of)
        assert np.all(np.abs(y) < 4.0)                                 # the clamps stay idle: the map is affine
        u = lo[:, np.newaxis] + z.reshape(nc, K) * width[:, np.newaxis]
        r = [np.sqrt(h * w) * (y[j, 1:] - np.broadcast_to(track[name], P)[1:]) for j, (name, w) in enumerate(weights.items())]
        r.append(np.sqrt(2.0) * (y[0, -1:] - track['x0'][-1:]))
        if move:
            for c in range(nc):
                if previous is not None:
                    r.append(np.sqrt(move) * (u[c, :1] - previous[c]))
                r.append(np.sqrt(move) * np.diff(u[c]))
        return np.concatenate(r)

    centre = np.full(D, 0.5)
    r0 = residuals(centre)
    A = np.stack([(residuals(centre + 0.25 * np.eye(D)[d]) - r0) / 0.25 for d in range(D)], axis=1)
    b = A @ centre - r0
    ref = lsq_linear(A, b, bounds=(0.0, 1.0), method='bvls', tol=1e-15, max_iter=2000)
    return res, ref.x, float(np.sum((A @ ref.x - b) ** 2))


LQ_CASES = {
    'D16 idle box, move 0.01': dict(D=16, amplitude=0.1, move=0.01, on_bound=0),
    'D16 idle box, move 0': dict(D=16, amplitude=0.1, move=0.0, on_bound=0, cost_only=True),
    'D8 box binds': dict(D=8, amplitude=0.3, move=0.01, box={'u0': (-0.3, 0.45)}, on_bound=2),
    'D5 box binds': dict(D=5, amplitude=0.3, move=0.01, box={'u0': (-0.3, 0.45)}, on_bound=2),
    'previous': dict(D=8, amplitude=0.1, move=0.01, previous=[0.3], on_bound=0),
    'two controls': dict(D=16, amplitude=0.1, move=0.01, n_controls=2, on_bound=0),
}
LQ_COST_GATE, LQ_Z_GATE = 2.95e-14, 5.22e-14


@pytest.mark.parametrize('case', list(LQ_CASES))
def test_linear_quadratic_against_bounded_least_squares(case):
    """Order-1 Bernoulli terms only: with idle clamps the trajectory is affine in z, the cost a linear least-squares problem
    in a box, and ``lsq_linear(method='bvls')`` on the affine map (built from simulate_host) solves it exactly.

    Measured on this host over the six cases: relative cost difference <= 2.95e-15, max |z - z_ref| <= 5.22e-15 (1.8e-14
    with move weight 0, where the minimiser is ill-determined and only the cost is compared), 1 to 3 iterations.  The gates
    are 10 x that: 2.95e-14 and 5.22e-14."""
    spec = dict(LQ_CASES[case])
    on_bound, cost_only = spec.pop('on_bound'), spec.pop('cost_only', False)
    res, z_ref, cost_ref = _lq(steps=48, **spec)
    z = res.z[0].ravel()
    n_bound = int(np.sum((z_ref <= 0.0) | (z_ref >= 1.0)))
    relative = abs(res.cost[0] - cost_ref) / cost_ref
    print(f"\n{case}: status {res.status[0]}, {res.iterations[0]} iterations, cost {res.cost[0]:.15e} (exact {cost_ref:.15e}, "
          f"relative difference {relative:.2e}), max |z - z_ref| {np.max(np.abs(z - z_ref)):.2e}, {n_bound} segments on a bound")
    assert res.status[0] == optimize.CONVERGED and res.iterations[0] <= 60
    assert n_bound >= on_bound and (on_bound > 0 or n_bound == 0) and n_bound < z.shape[0]
    assert res.first_saturation[0] == -1
    assert relative <= LQ_COST_GATE
    if not cost_only:
        assert np.max(np.abs(z - z_ref)) <= LQ_Z_GATE
        assert np.array_equal((z <= 0.0) | (z >= 1.0), (z_ref <= 0.0) | (z_ref >= 1.0))


# ---------------------------------------------------------------------------------------------------------
# 3. a nonlinear system: the statuses mean what they say
# ---------------------------------------------------------------------------------------------------------

NONLINEAR = dict(segments=4, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3})


@pytest.fixture(scope='module')
def nonlinear():
    args = product(4, 16)
    return args, dynamics.control_host(**args, **NONLINEAR, starts=3, keep=['members', 'all'])


def test_nonlinear_statuses_hold_their_definitions(nonlinear):
    args, res = nonlinear
    E, S = res.cost_all.shape
    assert (E, S) == (4, 3) and np.all(res.status_all != optimize.NON_FINITE)
    for e in range(E):
        for s in range(S):
            # the first pass at the returned point: its cost is the reported one, its projected gradient meets the status
            again = dynamics.control_host(**args, **NONLINEAR, draws=np.array([e]), init=res.u_all[e, s], max_iter=0)
            z = (res.u_all[e, s] - 0.0) / 4.0
            assert np.array_equal(again.z[0], z)
            assert again.first_pass['F'][0, 0] == res.cost_all[e, s]
            g = again.first_pass['g'][0, 0]
            pg = np.max(np.abs(np.clip(z.ravel() - g, 0.0, 1.0) - z.ravel()))
            if res.status_all[e, s] == optimize.CONVERGED:
                assert pg <= 1e-10
            else:
                assert pg > 1e-10
                assert res.status_all[e, s] in (optimize.ITERATION_LIMIT, optimize.STALLED)
                assert (res.iterations_all[e, s] == 60) == (res.status_all[e, s] == optimize.ITERATION_LIMIT)
    assert np.any(res.status_all == optimize.CONVERGED)
    assert np.all(res.cost <= res.cost_start)
    assert np.array_equal(res.best_start, np.argmin(res.cost_all, axis=1))
    assert np.array_equal(res.cost, res.cost_all[np.arange(E), res.best_start])
    assert np.array_equal(res.u, res.u_all[np.arange(E), res.best_start])
    assert res.u_mean.shape == (1, 4) and res.u_bounds.shape == (1, 4, 2) and res.bounds.shape == (2, 17, 2)
    assert np.all(res.u >= 0.0) and np.all(res.u <= 4.0)


def test_more_starts_are_never_worse(nonlinear):
    args, res = nonlinear
    single = dynamics.control_host(**args, **NONLINEAR, starts=1, keep='all')
    assert np.array_equal(single.cost_all[:, 0], res.cost_all[:, 0]) and np.array_equal(single.u_all[:, 0], res.u_all[:, 0])
    assert np.all(res.cost <= single.cost)


def test_members_are_simulate_hosts_trajectories(nonlinear):
    args, res = nonlinear
    for e in range(4):
        alone = dynamics.simulate_host(**{**_system(args), 'forcing': _forcing(args, res, e)}, draws=np.array([e]),
                                       ReturnBounds=False, keep='members')
        assert np.array_equal(alone.members[0], res.members[e])
        assert alone.first_saturation[0] == res.first_saturation[e]
    assert np.array_equal(res.mean, res.members.mean(axis=0))
    spread = dynamics.simulate_host(**{**_system(args), 'forcing': _forcing(args, res)}, keep='members')
    assert spread.members.shape == res.members.shape


# ---------------------------------------------------------------------------------------------------------
# 4. invariances, bit for bit
# ---------------------------------------------------------------------------------------------------------

def _same(a, b, rows=None):
    for key in ('u', 'z', 'cost', 'status', 'iterations', 'cost_start', 'best_start', 'descent_steps', 'first_saturation',
                'members'):
        left = a[key] if rows is None else a[key][rows]
        assert np.array_equal(left, b[key]), key


def test_a_draw_alone_is_its_row_of_the_full_run(nonlinear):
    args, res = nonlinear
    alone = dynamics.control_host(**args, **NONLINEAR, starts=3, draws=np.array([2]), keep=['members', 'all'])
    _same(res, alone, rows=[2])
    assert np.array_equal(alone.cost_all[0], res.cost_all[2]) and np.array_equal(alone.u_all[0], res.u_all[2])


def test_segments_as_a_count_and_as_first_steps():
    args = mixed(2, 7)
    kw = dict(targets={'T': 0.2, 'c': -0.1}, move_weight={'u': 0.01}, keep='members')
    count = dynamics.control_host(**args, segments=3, **kw)
    assert count.segment_first.tolist() == [0, 3, 6] and count.u.shape == (2, 1, 3)           # holds of 3, 3 and 1 steps
    _same(count, dynamics.control_host(**args, segments=np.array([0, 3, 6]), **kw))
    assert dynamics.expand_controls(count, 1)['u'].tolist() == count.u[1, 0][[0, 0, 0, 1, 1, 1, 2]].tolist()


def test_a_state_without_weight_or_limit_changes_nothing():
    args = mixed(2, 7)
    kw = dict(segments=3, move_weight={'u': 0.01}, keep='members')
    plain = dynamics.control_host(**args, targets={'T': 0.2}, **kw)
    _same(plain, dynamics.control_host(**args, targets={'T': 0.2, 'c': 0.7}, weights={'c': 0.0}, **kw))
    _same(plain, dynamics.control_host(**args, targets={'T': 0.2}, limits={'c': (None, None)}, **kw))


def test_the_mean_draw_and_the_random_streams():
    args = mixed(3, 7)
    state = np.random.get_state()[1].copy()
    res = dynamics.control_host(**args, segments=3, targets={'T': 0.2}, draws='mean')
    assert np.array_equal(np.random.get_state()[1], state)
    assert res.u.shape == (1, 1, 3) and 'u_bounds' not in res and 'bounds' not in res
    averaged = [dict(m, betas=np.mean(m['betas'], axis=0, keepdims=True)) for m in args['models']]
    same = dynamics.control_host(**{**args, 'models': averaged}, segments=3, targets={'T': 0.2})
    assert np.array_equal(res.u, same.u) and np.array_equal(res.cost, same.cost)


def test_a_step_in_a_steepest_descent_lane():
    """H overflows (2 w t^2 with w = 1e300, t = 1e5) while F and g stay finite: the Newton direction is -g / inf = -0, no
    Newton trial moves z, and the first steepest-descent lane (P(z - g) = the upper bound, where the optimum lies) is taken."""
    c0, c1 = (float(v) for v in BERN[0])
    model = dict(betas=np.array([[-1e5 / c1 * c0, 1e5 / c1]]), mtx=np.array([[1]]), phis=BERN, minmax=[[0.0, 1.0]],
                 kernel='Bernoulli Polynomials')
    res = dynamics.control_host([model], ['x'], [['u']], controls=['u'], y0=[0.0], t=(0.0, 0.5, 1.0), bounds=[[-1e9, 1e9]],
                                segments=1, targets={'x': 1e5 + 1.0}, weights={'x': 1e300}, init=[[0.9999]])
    assert res.status.tolist() == [optimize.CONVERGED] and res.iterations.tolist() == [1] and res.descent_steps.tolist() == [1]
    assert res.z.tolist() == [[[1.0]]] and res.cost[0] < res.cost_start[0]


# ---------------------------------------------------------------------------------------------------------
# 5. soft limits
# ---------------------------------------------------------------------------------------------------------

def test_a_binding_limit_is_pressed_harder_by_its_weight():
    args = product(1, 16)
    kw = dict(segments=4, targets={'x0': 0.6}, move_weight={'u': 1e-3}, keep='members')
    free = dynamics.control_host(**args, **kw)
    ceiling = float(np.max(free.members[0, 0])) - 0.05                 # binds: the free optimum goes above it
    violation = []
    for weight in (1.0, 1e2, 1e4):
        res = dynamics.control_host(**args, **kw, limits={'x0': (None, ceiling)}, limit_weight=weight)
        assert res.status[0] == optimize.CONVERGED
        violation.append(float(np.sum(np.maximum(0.0, res.members[0, 0, 1:] - ceiling) ** 2)))
    print(f"\nlimit {ceiling:.4f}: squared violation {violation} for weights 1, 1e2, 1e4")
    assert violation[0] > violation[1] > violation[2] > 0.0


# ---------------------------------------------------------------------------------------------------------
# 6. refusals, by message
# ---------------------------------------------------------------------------------------------------------

class _NoDevice(_capi.DeviceContext):
    def __init__(self):
        self._h = None

    def control_solve(self, p):
        pytest.fail("a refused call reached the launch")


def _refused(match, args=None, **kw):
    args = dict(mixed(2, 7) if args is None else args)
    call = dict(segments=3, targets={'T': 0.2})
    call.update(kw)
    for key in ('controls', 'forcing', 'y0', 't', 'models', 'states', 'inputs'):
        if key in call:
            args[key] = call.pop(key)
    for run in (dynamics.control_host, lambda **a: dynamics.control(**a, device=_NoDevice())):
        with pytest.raises(ValueError, match=match):
            run(**args, **call)


def test_refusals():
    base = mixed(2, 7)
    # what simulate refuses of a system
    _refused("at most 8 states", args={**chain(8, 1, 4), 'models': chain(8, 1, 4)['models'] * 2, 'states': [f's{k}' for k in range(16)],
                                       'inputs': chain(8, 1, 4)['inputs'] * 2}, targets={'s0': 0.0})
    _refused("neither a state", inputs=[['T', 'c', 'u'], ['T', 'c', 'q']])
    _refused("h > 0", t=(0.0, 1.0, -0.1))
    # decision values and steps
    _refused("33 decision values, the solver handles at most 32", args=mixed(1, 33), segments=33)
    _refused("at most 4096 steps", t=(0.0, 4096.5 * 0.05, 0.05))
    _refused("no step at all", t=(0.0, 0.0, 0.05))
    _refused("segments", segments=0)
    _refused("segments as an array", segments=np.array([1, 3]))
    _refused("segments=5 holds", segments=5)                          # ceil(7 / 5) = 2 steps per hold cover 7 steps in 4
    # the controls
    _refused("at least one input column", controls=[])
    _refused("no model reads 'w'", controls=['u', 'w'])
    _refused("'T' is a state", controls=['T'])
    _refused("'d' is a forcing key", controls=['d'])
    _refused("no model reads 'u'", args={**base, 'models': [dict(base['models'][0], mtx=np.array([[1, 0, 0], [0, 2, 0], [1, 0, 0], [1, 1, 0]])),
                                                             base['models'][1]]})
    # the control box
    _refused("is empty", control_bounds={'u': (3.0, 3.0)})
    _refused("two finite numbers", control_bounds={'u': (0.0, np.inf)})
    _refused("outside the training range", control_bounds={'u': (-0.5, 5.0)})
    _refused("not a control", control_bounds={'T': (0.0, 1.0)})
    # the cost
    _refused("targets: 'x' is not a state", targets={'x': 0.0})
    _refused("limits: 'x' is not a state", limits={'x': (0.0, 1.0)})
    _refused("weights: 'x' is not a state", weights={'x': 1.0})
    _refused("terminal: 'x' is not a state", terminal={'x': 1.0})
    _refused("negative weights", weights={'T': -1.0})
    _refused("negative weights", terminal={'T': -1.0})
    _refused("negative weights", move_weight={'u': -1.0})
    _refused("negative weights", limit_weight=-1.0)
    _refused(r"one value per point of t \(8\)", targets={'T': np.zeros(7)})
    _refused("no residual at all", targets=None)
    _refused("no residual at all", targets={'T': np.full(8, np.nan)})
    _refused("no residual at all", targets={'T': 0.1}, weights={'T': 0.0})
    _refused("no residual at all", targets=None, move_weight={'u': 0.1}, segments=1)
    _refused("needs a target at the last point", targets=None, terminal={'T': 1.0}, limits={'c': (0.0, 1.0)})
    # starts
    _refused(r"init must be \[1, 3\]", init=np.zeros((1, 4)))
    _refused(r"previous must be \[1\]", previous=[0.0, 1.0], move_weight={'u': 0.1})
    _refused("starts must be a count >= 1", starts=0)
    _refused("one call runs at most 1048576 solves", starts=1 << 20)
    _refused("max_iter", max_iter=-1)
    _refused("keep must be", keep='particles')


def test_the_lds_refusal_prints_its_formula():
    """Eight models that read all eight states and the control, each through ranges of its own and in orders 1 .. 4: 288
    distinct factors and 64 normalised states, whose values and tangents alone are 2 x 353 rows of 512 bytes."""
    rng = np.random.default_rng(3)
    names = [f'x{k}' for k in range(8)]
    models = []
    for k in range(8):
        mtx = np.zeros((36, 9), dtype=int)
        for j in range(9):
            mtx[4 * j + np.arange(4), j] = 1 + np.arange(4)
        minmax = [[-1.0 - 0.01 * k, 1.0 + 0.125 * j] for j in range(8)] + [[0.0, 1.0 + 0.01 * k]]
        models.append(dict(betas=0.01 * rng.standard_normal((1, 37)), mtx=mtx, phis=BERN, minmax=minmax,
                           kernel='Bernoulli Polynomials'))
    args = dict(models=models, states=names, inputs=[names + ['u']] * 8, controls=['u'], y0=np.zeros(8), t=(0.0, 31.5 * 0.05, 0.05))
    need = (r"needs 382272 bytes of LDS \(\(2 x \(1 \+ 288 factors \+ 64 normalised states\) \+ 4 \+ 32 decision values\) x 64 x 8 "
            r"\+ 296 coefficients x 8\), a wavefront has 147456")
    _refused(need, args=args, segments=32, targets={'x0': 0.0})

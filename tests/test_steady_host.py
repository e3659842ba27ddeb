"""dynamics.steady_states_host, the statement the device kernel is tested against (tests/test_steady_gpu.py): a linear
system against its closed form, a cubic with three rest points and its fold over an input grid, a root held on the wall of the
box, the residual recomputed for spline and mixed systems, the status codes, the summaries and every refusal -- none of which
needs a device."""
import numpy as np
import pytest

from fokl_gpy_amd import _capi, dynamics
from test_simulate_adaptive_host import BERN, SPLINES, _bern_model, spline_system, two_state_system

FIELDS = ('y', 'residual', 'iterations', 'status', 'halvings', 'on_wall', 'jacobian')
DTYPES = dict(y=np.float64, residual=np.float64, iterations=np.int32, status=np.int8, halvings=np.int32, on_wall=np.bool_,
              jacobian=np.float64)
ROOTS = (0.8, 2.1, 3.3)
C0, C1 = (float(v) for v in BERN[0])


class _Reached(Exception):
    pass


class _NoDevice(_capi.DeviceContext):
    """Stands where the device context would be: a refused call must not reach the launch, a well-formed one ends here."""

    def __init__(self, expect_launch=False):
        self._h = None
        self.expect_launch = expect_launch

    def steady_states(self, p):
        if not self.expect_launch:
            pytest.fail("a refused call reached the launch")
        raise _Reached(p)


# ---------------------------------------------------------------------------------------------------------
# the systems (tests/test_steady_gpu.py imports them)
# ---------------------------------------------------------------------------------------------------------

def linear_system(E=3):
    """dy/dt = scale_e (A (y - 2) + B (u - 1)) with A = [[-1, -2], [2, -1]] (eigenvalues -1 +- 2 i), B = [1, 0.5], as order-1
    Bernoulli models over [0, 4]^2 x [0, 2] -> (arguments, A [E, 2, 2] and B [E, 2] from the very doubles the models hold,
    the constants [E, 2])."""
    scale = np.linspace(1.0, 2.0, E)
    A, B = np.array([[-1.0, -2.0], [2.0, -1.0]]), np.array([1.0, 0.5])
    models, As, Bs, cs = [], [], [], []
    for k in range(2):
        beta = scale[:, None] * np.array([A[k, 0] * 4.0 / C1, A[k, 1] * 4.0 / C1, B[k] * 2.0 / C1])
        const = -beta @ np.array([C0 + 0.5 * C1, C0 + 0.5 * C1, C0 + 0.5 * C1])       # zero at y = (2, 2), u = 1
        models.append(_bern_model(np.column_stack([const, beta]), [[1, 0, 0], [0, 1, 0], [0, 0, 1]],
                                  [[0.0, 4.0], [0.0, 4.0], [0.0, 2.0]]))
        As.append(np.stack([beta[:, 0] * C1 / 4.0, beta[:, 1] * C1 / 4.0], axis=1))
        Bs.append(beta[:, 2] * C1 / 2.0)
        cs.append(const + beta @ np.array([C0, C0, C0]))
    args = dict(models=models, states=['x', 'z'], inputs=[['x', 'z', 'u'], ['x', 'z', 'u']])
    return args, np.stack(As, axis=1), np.stack(Bs, axis=1), np.stack(cs, axis=1)


def cubic_betas(kappa, roots=ROOTS, lo=0.0, hi=4.0):
    """beta_0 .. beta_3 with beta_0 + sum_k beta_k B_k((y - lo) / (hi - lo)) = -kappa (y - a) (y - b) (y - c)."""
    a, b, c = roots
    in_y = -kappa * np.poly1d([1.0, -a]) * np.poly1d([1.0, -b]) * np.poly1d([1.0, -c])
    mono = in_y(np.poly1d([hi - lo, lo])).coeffs[::-1]                # in v, lowest power first
    basis = np.zeros((4, 4))
    basis[0, 0] = 1.0
    for k in (1, 2, 3):
        basis[:k + 1, k] = [float(v) for v in BERN[k - 1][:k + 1]]
    return np.linalg.solve(basis, mono)


def cubic_slope(kappa, y, roots=ROOTS):
    a, b, c = roots
    return -kappa * ((y - a) * (y - b) + (y - a) * (y - c) + (y - b) * (y - c))


def cubic_system(kappas=(1.0, 1.25, 1.5, 1.75), with_u=False):
    """dy/dt = -kappa_e (y - 0.8) (y - 2.1) (y - 3.3) [+ (u - 1)] on the box [0, 4]: rest points stable, unstable, stable."""
    betas = np.array([cubic_betas(kappa) for kappa in kappas])
    if with_u:
        model = _bern_model(np.column_stack([betas, np.full(len(kappas), 2.0 / C1)]), [[1, 0], [2, 0], [3, 0], [0, 1]],
                            [[0.0, 4.0], [0.0, 2.0]])
        return dict(models=[model], states=['y'], inputs=[['y', 'u']])
    return dict(models=[_bern_model(betas, [[1], [2], [3]], [[0.0, 4.0]])], states=['y'], inputs=[['y']])


def wall_root_system(E=2):
    """dx/dt = scale_e (5 - x), whose rest point 5 lies behind the wall x = 4; dz/dt = scale_e (0.5 x - z): z rests at 2 once x
    is held on the wall."""
    scale = np.linspace(1.0, 1.5, E)
    bx = -1.0 * 4.0 / C1
    first = _bern_model(scale[:, None] * np.array([5.0 - bx * C0, bx]), [[1]], [[0.0, 4.0]])
    bzx, bzz = 0.5 * 4.0 / C1, -1.0 * 4.0 / C1
    second = _bern_model(scale[:, None] * np.array([-(bzx + bzz) * C0, bzx, bzz]), [[1, 0], [0, 1]], [[0.0, 4.0], [0.0, 4.0]])
    return dict(models=[first, second], states=['x', 'z'], inputs=[['x'], ['x', 'z']])


def mixed_system(E=5):
    """A spline model and a Bernoulli model, each reading both states and the input u."""
    rng = np.random.default_rng(11)
    first = dict(betas=np.array([0.05, -0.9, 0.3, 0.2]) * (1 + 0.1 * rng.standard_normal((E, 4))),
                 mtx=np.array([[1, 0, 0], [0, 2, 0], [1, 0, 1]]), phis=SPLINES, minmax=[[0.0, 2.0], [-1.0, 1.0], [0.0, 1.0]],
                 kernel='Cubic Splines')
    second = _bern_model(np.array([0.02, 0.4, -1.1, 0.3]) * (1 + 0.1 * rng.standard_normal((E, 4))),
                         [[1, 0, 0], [0, 1, 0], [0, 2, 1]], [[0.0, 2.0], [-1.0, 1.0], [0.0, 1.0]])
    return dict(models=[first, second], states=['T', 'c'], inputs=[['T', 'c', 'u'], ['T', 'c', 'u']])


def nan_cubic():
    args = cubic_system()
    args['models'][0]['betas'][1, 2] = np.nan
    return args


def recomputed_residual(args, res, **options):
    """max_j |F_j| / ftol_j with F from dynamics._stage (the value operations of ``simulate``) at every reported state."""
    p = dynamics._prepare_steady(**{**dict(at=None, draws=None, bounds=None, starts=9, ftol=None, time_scale=1.0, max_iter=50,
                                           max_halvings=8, merge_tol=1e-6, keep=None), **args, **options})
    Q, E, S, K = res.y.shape
    out = np.empty((Q, E, S))
    n_norms = p['norm_src'].shape[0]
    for q in range(Q):
        for e in range(E):
            fac, xn = np.ones((1 + p['fac_norm'].shape[0], S)), np.zeros((n_norms, S))
            for n in range(p['n_norm_forcing']):
                x = np.full(S, p['forcing'][q, -(p['norm_src'][n] + 1)])
                xn[n], _ = dynamics._clamped((x - p['norm_lo'][n]) / p['norm_span'][n])
            dynamics._factor_values(p, fac, xn, 0, p['n_forcing_factors'])
            with np.errstate(all='ignore'):
                F, _ = dynamics._stage(dict(p, coef=np.repeat(p['coef'][:, e:e + 1], S, axis=1), h=1.0), fac, xn,
                                       np.ascontiguousarray(res.y[q, e].T))
            out[q, e] = dynamics._steady_ratio(F, p['ftol'])
    return out


# ---------------------------------------------------------------------------------------------------------
# 1. a linear system
# ---------------------------------------------------------------------------------------------------------

def test_linear_system_converges_to_its_closed_form_from_every_start():
    """|y - y*| <= n ||J^-1||_inf max_j ftol_j follows from |F_j| <= ftol_j at a converged member of a linear system.  The
    eigenvalues scale_e (-1 +- 2 i) of a 2 x 2 block through np.linalg.eigvals: measured 2.0e-16 relative to |lambda| here; ten
    times that is allowed."""
    args, A, B, c = linear_system()
    u = np.array([0.6, 1.0, 1.7])
    res = dynamics.steady_states_host(**args, at={'u': u}, keep='jacobian')
    assert res.y.shape == (3, 3, 9, 2) and (res.status == 0).all() and (res.iterations <= 2).all() and res.stable.all()
    worst = 0.0
    for q in range(3):
        for e in range(3):
            want = -np.linalg.solve(A[e], B[e] * u[q] + c[e])
            bound = 2 * np.max(np.sum(np.abs(np.linalg.inv(A[e])), axis=1)) * np.max(res.ftol)
            assert np.max(np.abs(res.y[q, e] - want)) <= bound
            lam = np.linspace(1.0, 2.0, 3)[e] * np.array([-1.0 + 2.0j, -1.0 - 2.0j])  # the closed form
            for s in range(9):
                got = res.eig[q, e, s]
                worst = max(worst, max(np.min(np.abs(got - v)) for v in lam) / np.abs(lam[0]))
                assert np.array_equal(res.jacobian[q, e, s], A[e])    # a linear model's tangent is its coefficient
    print(f"\neigenvalues: distance to the closed form, relative: {worst:.3e}")
    assert worst <= 10 * 2.0e-16
    assert (res.n_roots == 1).all() and (res.n_stable == 1).all() and np.array_equal(res.unique_fraction, np.ones(3))
    assert np.array_equal(res.multiplicity, np.tile([0.0, 1.0], (3, 1)))
    for q in range(3):                                                 # three draws: cut = 1, sorted[1] and sorted[3 - 1]
        single = np.sort(np.array([res.roots[q][e][0] for e in range(3)]), axis=0)
        assert np.array_equal(res.unique_bounds[q], np.stack([single[1], single[2]], axis=-1))
        assert np.allclose(res.unique_mean[q], single.mean(axis=0), rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------------------
# 2. three rest points, and their fold
# ---------------------------------------------------------------------------------------------------------

def test_cubic_has_three_rest_points_stable_unstable_stable():
    """A converged root is within n ftol / |f'(root)| of the exact one (|F| <= ftol and the mean value theorem, f' changing by
    less than a tenth over that distance), plus 1e-12 for the rounding of the model's coefficients (four basis functions of
    size <= 10 at 1.1e-16 each, over |f'| >= 1.5).  f' at the roots: measured 2.1e-9 relative here (it is f' at the reported
    root, which is off by up to the bound above, times f'' / f' <= 4); ten times that is allowed."""
    kappas = (1.0, 1.25, 1.5, 1.75)
    res = dynamics.steady_states_host(**cubic_system(kappas), starts=9, keep='jacobian')
    assert res.y.shape == (1, 4, 9, 1) and (res.status == 0).all()
    assert np.array_equal(res.n_roots, np.full((1, 4), 3)) and np.array_equal(res.n_stable, np.full((1, 4), 2))
    assert np.array_equal(res.multiplicity, [[0.0, 0.0, 0.0, 1.0]]) and res.unique_fraction.tolist() == [0.0]
    assert np.isnan(res.unique_mean).all() and np.isnan(res.unique_bounds).all()
    worst = 0.0
    for e, kappa in enumerate(kappas):
        roots = res.roots[0][e]
        assert roots.shape == (3, 1) and res.root_stable[0][e].tolist() == [True, False, True]
        slopes = np.array([cubic_slope(kappa, r) for r in ROOTS])
        assert np.all(np.abs(roots[:, 0] - ROOTS) <= 1.1 * res.ftol[0] / np.abs(slopes) + 1e-12)
        for s in range(9):
            nearest = int(np.argmin(np.abs(res.y[0, e, s, 0] - np.array(ROOTS))))
            worst = max(worst, abs(res.eig[0, e, s, 0] - slopes[nearest]) / abs(slopes[nearest]))
            assert res.stable[0, e, s] == (slopes[nearest] < 0)
    print(f"\nf' at the roots: distance to the closed form, relative: {worst:.3e}")
    assert worst <= 10 * 2.1e-9
    assert (res.iterations.max() > 2) and res.iterations.dtype == np.int32


def test_outer_roots_merge_and_vanish_over_an_input_grid():
    """f(y) + (u - 1) has three roots while -kappa f_max < u - 1 < -kappa f_min, f_min and f_max the values of
    -(y - a) (y - b) (y - c) at the roots of its derivative: with kappa = 1 for 0.2997 < u < 1.8044."""
    a, b, c = ROOTS
    turning = np.roots(np.polyder(np.poly1d([1.0, -a]) * np.poly1d([1.0, -b]) * np.poly1d([1.0, -c])))
    values = sorted(-(y - a) * (y - b) * (y - c) for y in turning)
    kappas = (1.0, 1.25, 1.5)
    u = np.array([0.2, 0.5, 1.0, 1.3, 1.6, 1.9])
    res = dynamics.steady_states_host(**cubic_system(kappas, with_u=True), at={'u': u}, starts=9)
    want = np.array([[3 if -kappa * values[1] < ui - 1.0 < -kappa * values[0] else 1 for kappa in kappas] for ui in u])
    assert want[:, 0].tolist() == [1, 3, 3, 3, 3, 1] and want[:, 1:].min() == 3
    assert np.array_equal(res.n_roots, want)
    assert np.array_equal(res.n_stable, np.where(want == 3, 2, 1))
    assert np.allclose(res.multiplicity[:, 1], [1 / 3, 0, 0, 0, 0, 1 / 3]) and np.allclose(res.multiplicity[:, 3], 1 - res.multiplicity[:, 1])
    assert np.array_equal(res.unique_fraction, res.multiplicity[:, 1]) and np.isnan(res.unique_mean).all()
    assert set(np.unique(res.status)) <= {0, 1, 2} and (res.status[2] == 0).all()
    assert res.roots[0][0][0, 0] < 0.8 and res.roots[5][0][0, 0] > 3.3   # the lower branch is left at u = 0.2, the upper at 1.9


# ---------------------------------------------------------------------------------------------------------
# 3. a root on the wall
# ---------------------------------------------------------------------------------------------------------

def test_a_root_pushed_against_the_wall_is_held_and_is_a_rest_point_of_simulate():
    args = wall_root_system()
    res = dynamics.steady_states_host(**args, starts=5, keep='jacobian')
    assert (res.status == 0).all() and (res.y[..., 0] == 4.0).all()
    assert res.on_wall[..., 0].all() and not res.on_wall[..., 1].any()
    assert np.max(np.abs(res.y[..., 1] - 2.0)) <= 2 * 1.0 * np.max(res.ftol)          # |dF_z / dz| >= 1
    assert np.isnan(res.eig[..., 0]).all() and np.all(res.eig[..., 1].real < 0) and res.stable.all()
    assert (res.jacobian[..., 0, :] == 0).all() and (res.n_roots == 1).all()
    for e in range(2):
        for s in range(5):
            run = dynamics.simulate_host(**args, y0=res.y[0, e, s], t=(0.0, 10 / 64, 1 / 64), draws=np.array([e]),
                                         ReturnBounds=False, keep='members')
            assert np.array_equal(run.members[0], np.repeat(res.y[0, e, s][:, None], 11, axis=1))


# ---------------------------------------------------------------------------------------------------------
# 4. the residual is simulate's F
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['spline', 'mixed', 'two_state'])
def test_residual_is_the_stage_at_the_reported_state(name):
    if name == 'spline':
        args, options = {k: v for k, v in spline_system().items() if k in ('models', 'states', 'inputs')}, {}
    elif name == 'mixed':
        args, options = mixed_system(), dict(at={'u': np.array([0.2, 0.5, 0.9])})
    else:
        args = {k: v for k, v in two_state_system().items() if k in ('models', 'states', 'inputs')}
        options = dict(at={'u': np.array([3.0, 9.0])})
    res = dynamics.steady_states_host(**args, **options, starts=7)
    again = recomputed_residual(args, res, **options, starts=7)
    assert np.array_equal(res.residual, again, equal_nan=True)
    assert (res.status == 0).any() and np.all((res.residual <= 1) == (res.status == 0))
    print(f"\n{name}: status counts {np.bincount(res.status.ravel(), minlength=4).tolist()}, iterations up to "
          f"{res.iterations.max()}, halvings up to {res.halvings.max()}")


# ---------------------------------------------------------------------------------------------------------
# 5. status codes, locality, bookkeeping
# ---------------------------------------------------------------------------------------------------------

def test_status_codes():
    one = dynamics.steady_states_host(**cubic_system(), max_iter=1)
    assert (one.status == 1).any() and set(np.unique(one.status)) <= {0, 1} and (one.iterations[one.status == 1] == 1).all()
    assert (one.residual[one.status == 1] > 1).all()
    # no root and no wall: a right-hand side >= 1 in an unbounded box.  Outside the model's range the clamp makes it flat
    # (from 7.0 the step is F / -0.0 = -inf, where F is 2.6 and not below the 2.4 at 7.0: every trial point fails)
    flat = _bern_model([[1.5, -0.2, 6.0]], [[1], [2]], [[0.0, 4.0]])                  # 1.5 - 0.2 B1 + 6 B2 >= 1.5 - 0.1 - 0.5
    none = dynamics.steady_states_host(models=[flat], states=['y'], inputs=[['y']], bounds=[[-np.inf, np.inf]],
                                       starts=np.array([[0.5], [2.0], [3.9], [7.0]]), ftol=1e-9)
    assert set(np.unique(none.status)) <= {1, 2} and (none.n_roots == 0).all() and none.multiplicity.tolist() == [[1.0]]
    assert none.status[0, 0, 3] == 2 and none.halvings[0, 0, 3] == 9 and none.iterations[0, 0, 3] == 0   # J == 0: stalled
    assert not none.stable.any() and np.isnan(none.unique_mean).all()


def test_a_nan_draw_ends_as_not_finite_and_stays_local():
    res = dynamics.steady_states_host(**nan_cubic(), keep='jacobian')
    assert (res.status[0, 1] == 3).all() and (res.iterations[0, 1] == 0).all() and np.isnan(res.residual[0, 1]).all()
    assert (res.status[0, [0, 2, 3]] == 0).all() and res.n_roots.tolist() == [[3, 0, 3, 3]]
    others = dynamics.steady_states_host(**cubic_system(), draws=np.array([0, 2, 3]), keep='jacobian')
    for key in FIELDS + ('eig', 'stable'):
        assert np.array_equal(res[key][:, [0, 2, 3]], others[key], equal_nan=True), key
    assert np.allclose(res.multiplicity, [[0.25, 0, 0, 0.75]])


def test_bookkeeping():
    args = cubic_system(with_u=True)
    state = np.random.get_state()[1].copy()
    full = dynamics.steady_states_host(**args, at={'u': [0.9, 1.1]}, starts=6, keep='jacobian')
    assert np.array_equal(np.random.get_state()[1], state)           # nothing is drawn
    shapes = dict(y=(2, 4, 6, 1), residual=(2, 4, 6), iterations=(2, 4, 6), status=(2, 4, 6), halvings=(2, 4, 6),
                  on_wall=(2, 4, 6, 1), jacobian=(2, 4, 6, 1, 1), eig=(2, 4, 6, 1), stable=(2, 4, 6), n_roots=(2, 4),
                  n_stable=(2, 4), multiplicity=(2, 4), unique_fraction=(2,), unique_mean=(2, 1), unique_bounds=(2, 1, 2))
    for key, shape in shapes.items():
        assert full[key].shape == shape, key
    for key in FIELDS:
        assert full[key].dtype == DTYPES[key], key
    assert full.eig.dtype == np.complex128 and full.stable.dtype == np.bool_ and full.states == ['y']
    bare = dynamics.steady_states_host(**args, at={'u': [0.9, 1.1]}, starts=6)
    assert 'jacobian' not in bare and 'eig' not in bare
    for key in bare:
        if key not in ('roots', 'root_stable', 'states', 'at'):
            assert np.array_equal(bare[key], full[key], equal_nan=True), key
    # the starts: the centre, then Halton points in the open box; an array is taken as it is; a number in at is shared
    assert full.starts[:, 0].tolist() == [2.0, 2.0, 1.0, 3.0, 0.5, 2.5]
    two = dynamics.steady_starts(4, np.array([[0.0, 1.0], [0.0, 3.0]]))
    assert two.tolist() == [[0.5, 1.5], [0.5, 1.0], [0.25, 2.0], [0.75, 3.0 * (1 / 3 / 3)]]
    given = dynamics.steady_states_host(**args, at={'u': 0.9}, starts=full.starts)
    assert given.y.shape == (1, 4, 6, 1) and np.array_equal(given.y[0], full.y[0])
    mean = dynamics.steady_states_host(**args, at={'u': 0.9}, starts=6, draws='mean')
    assert mean.y.shape == (1, 1, 6, 1) and (mean.n_roots == 3).all()
    last = dynamics.steady_states_host(**args, at={'u': 0.9}, starts=6, draws=2)
    assert np.array_equal(last.y, full.y[:1, 2:])
    # one point alone is that point of the grid
    alone = dynamics.steady_states_host(**args, at={'u': [1.1]}, starts=6, keep='jacobian')
    for key in FIELDS:
        assert np.array_equal(alone[key][0], full[key][1]), key
    # merge_tol = 0: every distinct final state is a root of its own
    apart = dynamics.steady_states_host(**args, at={'u': 0.9}, starts=6, merge_tol=0.0)
    assert (apart.n_roots >= 3).all()


# ---------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------

def test_refusals_name_the_limit_and_launch_nothing():
    good = dict(**cubic_system(with_u=True), at={'u': [0.9, 1.1]})

    def refused(match, **changes):
        with pytest.raises(ValueError, match=match):
            dynamics.steady_states(**{**good, **changes}, device=_NoDevice())

    with pytest.raises(_Reached) as hit:
        dynamics.steady_states(**good, device=_NoDevice(expect_launch=True))
    p = hit.value.args[0]
    assert (p['Q'], p['E'], p['S'], p['K'], p['n_steps']) == (2, 4, 9, 1, 2) and p['forcing'].tolist() == [[0.9], [1.1]]
    assert p['ftol'].tolist() == [1e-9 * 4.0] and (p['max_iter'], p['max_halvings']) == (50, 8) and not p['want_jacobian']
    assert p['lds_rows'] == 2 * (1 + 4 + 1) + 5 and p['starts'].shape == (9, 1) and p['coef'].shape == (5, 4)
    with pytest.raises(_Reached) as hit:
        dynamics.steady_states(**good, time_scale=100.0, device=_NoDevice(expect_launch=True))
    assert hit.value.args[0]['ftol'].tolist() == [1e-9 * 4.0 / 100.0]
    refused(r"at: the input columns \['u'\] are no states and at gives no value", at=None)
    refused(r"at: the input columns \['u'\] are no states", at={'w': 1.0})
    refused(r"at: \['y'\] are states", at={'u': 1.0, 'y': 2.0})
    refused(r"at: the arrays have unequal lengths \{'u': 2, 'w': 3\}", at={'u': [0.9, 1.1], 'w': [1.0, 2.0, 3.0]})
    refused(r"at\['u'\] must be a number or \[Q\] values", at={'u': np.ones((2, 2))})
    refused(r"at\['u'\] must be a number or \[Q\] values", at={'u': []})
    refused(r"at\['u'\] must hold finite numbers", at={'u': [0.9, np.nan]})
    refused("the box is unbounded.*pass starts as an array", bounds=[[0.0, np.inf]])
    refused("the box is unbounded.*pass ftol", bounds=[[0.0, np.inf]], starts=[[1.0]])
    with pytest.raises(_Reached):
        dynamics.steady_states(**good, bounds=[[0.0, np.inf]], starts=[[1.0]], ftol=1e-9, device=_NoDevice(expect_launch=True))
    refused(r"starts\[1\]: state 'y' = 4.5 lies outside its box \[0.0, 4.0\]", starts=[[1.0], [4.5]])
    with pytest.raises(_Reached):                                     # the closed box: the wall itself is inside
        dynamics.steady_states(**good, starts=[[0.0], [4.0]], device=_NoDevice(expect_launch=True))
    refused(r"starts as an array must be \[S, 1\]", starts=[1.0, 2.0])
    refused("starts holds NaN", starts=[[np.nan]])
    for bad in (0, -3, 2.5, True):
        refused(r"starts must be an integer S >= 1 or an array \[S, 1\]", starts=bad)
    for bad in (0, 201, 2.5, '3', True):
        refused(r"max_iter must be an integer in 1\.\.200", max_iter=bad)
    for bad in (-1, 31, 0.5):
        refused(r"max_halvings must be an integer in 0\.\.30", max_halvings=bad)
    for bad in (0.0, -1e-9, np.nan, np.inf):
        refused("ftol must be positive and finite for every state", ftol=bad)
    refused(r"ftol needs one value per state \(1\)", ftol=[1e-9, 1e-9])
    for bad in (0.0, -1.0, np.inf, 'fast'):
        refused("time_scale must be positive and finite", time_scale=bad)
    refused("merge_tol must be finite and not negative", merge_tol=-1e-6)
    for bad in ('members', ('jacobian',), 3):
        refused("keep must be None or 'jacobian'", keep=bad)
    # what simulate refuses, with simulate's message
    refused('at least one fitted model', models=[])
    refused(r'models\[0\] has 2 input columns .* names 1', inputs=[['y']])
    refused("state 'y': its box is empty", bounds=[[1.0, 1.0]])
    refused('draws', draws=2.5)
    # the tangent rows: a system simulate still takes (288 values) needs 291 here
    fits = _bern_model(np.full((2, 285), 0.01), np.tile([[1]], (284, 1)), [[0.0, 1.0]])
    refused(r'needs 291 values per member in LDS \(2 x \(1 \+ 1 factors \+ 1 normalised states\) \+ 285 coefficients.*tangent '
            r'rows\), a wavefront.s 144 KB hold 288', models=[fits], inputs=[['y']], at=None)
    # the host statement refuses the same
    with pytest.raises(ValueError, match=r'max_iter must be an integer in 1\.\.200'):
        dynamics.steady_states_host(**good, max_iter=0)
    with pytest.raises(ValueError, match='needs 291 values per member in LDS'):
        dynamics.steady_states_host(models=[fits], states=['y'], inputs=[['y']])

"""The multistart optimiser without a device: argument handling up to a stand-in context, the start sequence, and the
host statement (optimize.optimize_host, what the kernel is tested against) on analytic models, an exhaustive grid and
scipy's L-BFGS-B."""
import numpy as np
import pytest

from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd import optimize as opt
from fokl_gpy_amd.FoKLRoutines import FoKL

PHIS = getKernels.bernoulli()
MINMAX = [[0.0, 2.0], [-1.0, 3.0]]
TOY_MTX = np.array([[1, 0], [0, 1], [2, 0], [0, 2], [1, 1], [3, 0], [0, 3], [2, 1], [1, 2], [4, 0], [0, 4], [3, 2]])


def phi(order, x, d=0):
    """Bernoulli basis `order` at normalised x (numpy's polynomial arithmetic: independent of the solver's Horner)."""
    p = np.polynomial.Polynomial(PHIS[order - 1])
    return p.deriv(d)(x) if d else p(x)


def model(betas, mtx, xn):
    """The model at normalised points xn [..., m]."""
    out = np.full(np.shape(xn)[:-1], betas[0], dtype=np.float64)
    for t, row in enumerate(np.atleast_2d(mtx)):
        term = np.ones_like(out)
        for j, order in enumerate(row):
            if order:
                term = term * phi(int(order), xn[..., j])
        out = out + betas[t + 1] * term
    return out


def toy_betas(draws=1, seed=3):
    rng = np.random.default_rng(seed)
    mean = np.array([0.3, 0.8, -0.5, 1.5, -1.2, 0.9, 0.7, -0.6, 0.5, 0.4, -2.0, 1.6, 0.8])
    return mean * (1 + 0.1 * rng.standard_normal((draws, mean.shape[0])))


class _Reached(Exception):
    pass


class _NoDevice(_capi.DeviceContext):
    """Stands where the device context would be: the CPU tests end here, after every check that needs no device."""

    def __init__(self):
        self._h = None

    def model_optimize(self, *args):
        raise _Reached(*args)


def _seen(*args, **kwargs):
    with pytest.raises(_Reached) as hit:
        opt.optimize(*args, device=_NoDevice(), **kwargs)
    return hit.value.args


# ---------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------

def test_shapes_reach_the_context_normalised():
    betas = toy_betas(5)
    mtx, b, table, lo, hi, starts, sign, max_iter, tol = _seen(betas, TOY_MTX, PHIS, MINMAX)
    assert mtx.dtype == np.int32 and mtx.shape == (12, 2) and b.shape == (5, 13) and table.shape == (20, 21)
    assert lo.tolist() == [0, 0] and hi.tolist() == [1, 1] and starts.shape == (32, 2)
    assert (sign, max_iter, tol) == (-1.0, 60, 1e-10)
    # 1-D betas are one draw; 'mean' averages the rows; 'min' flips the sign
    assert _seen(betas[0], TOY_MTX, PHIS, MINMAX)[1].shape == (1, 13)
    seen = _seen(betas, TOY_MTX, PHIS, MINMAX, objective='mean', sense='min')
    assert seen[1].shape == (1, 13) and np.array_equal(seen[1][0], betas.mean(axis=0)) and seen[6] == 1.0
    # a box in true scale, one input fixed; user starts in true scale, clipped to the box
    seen = _seen(betas, TOY_MTX, PHIS, MINMAX, bounds=[[0.5, 1.5], [1.0, 1.0]], starts=[[1.0, 1.0], [0.0, 3.0], [2.0, -1.0]])
    assert np.allclose(seen[3], [0.25, 0.5]) and np.allclose(seen[4], [0.75, 0.5]) and seen[3][1] == seen[4][1]
    assert np.allclose(seen[5], [[0.5, 0.5], [0.25, 0.5], [0.75, 0.5]])
    # an integer count of starts inside a narrower box
    seen = _seen(betas, TOY_MTX, PHIS, MINMAX, bounds=[[0.5, 1.5], [-1.0, 0.0]], starts=7)
    assert seen[5].shape == (7, 2) and np.all(seen[5] >= seen[3]) and np.all(seen[5] <= seen[4])


def test_refusals_come_before_the_device():
    betas = toy_betas(3)
    kw = dict(device=_NoDevice())
    with pytest.raises(ValueError, match='Cubic Splines'):
        opt.optimize(betas, TOY_MTX, getKernels.table_to_phis(np.zeros((2, 4, 499))), MINMAX, kernel='Cubic Splines', **kw)
    with pytest.raises(ValueError, match='outside the training range'):
        opt.optimize(betas, TOY_MTX, PHIS, MINMAX, bounds=[[0.0, 2.5], [-1.0, 3.0]], **kw)
    with pytest.raises(ValueError, match='above its upper'):
        opt.optimize(betas, TOY_MTX, PHIS, MINMAX, bounds=[[1.5, 0.5], [-1.0, 3.0]], **kw)
    with pytest.raises(ValueError, match='coefficients per draw'):
        opt.optimize(betas[:, :-1], TOY_MTX, PHIS, MINMAX, **kw)
    with pytest.raises(ValueError, match='at most 16 inputs'):
        opt.optimize(np.ones(2), np.ones((1, 17), dtype=int), PHIS, [[0, 1]] * 17, **kw)
    with pytest.raises(ValueError, match='outside the coefficient table'):
        opt.optimize(np.ones(2), np.array([[21, 0]]), PHIS, MINMAX, **kw)
    with pytest.raises(ValueError, match='sense'):
        opt.optimize(betas, TOY_MTX, PHIS, MINMAX, sense='largest', **kw)
    with pytest.raises(ValueError, match='objective'):
        opt.optimize(betas, TOY_MTX, PHIS, MINMAX, objective='median', **kw)
    with pytest.raises(ValueError, match='starts'):
        opt.optimize(betas, TOY_MTX, PHIS, MINMAX, starts=np.zeros((4, 3)), **kw)
    with pytest.raises(ValueError, match='at most'):
        opt.optimize(np.ones((1 << 15, 13)), TOY_MTX, PHIS, MINMAX, starts=64, **kw)


def test_numpys_random_stream_does_not_move():
    np.random.seed(11)
    before = np.random.get_state()
    _seen(toy_betas(4), TOY_MTX, PHIS, MINMAX, starts=16)
    opt.optimize_host(toy_betas(4), TOY_MTX, PHIS, MINMAX, starts=16)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_start_sequence_is_deterministic_and_inside_the_box():
    lo, hi = np.array([0.2, 0.0, 0.5]), np.array([0.4, 1.0, 0.5])
    a, b = opt.start_points(100, lo, hi), opt.start_points(100, lo, hi)
    assert np.array_equal(a, b) and a.shape == (100, 3)
    assert np.all(a >= lo) and np.all(a <= hi) and np.all(a[:, 2] == 0.5)
    assert np.array_equal(opt.start_points(10, lo, hi), a[:10])          # a longer sequence extends a shorter one
    assert len(np.unique(a[:, :2], axis=0)) == 100
    unit = opt.start_points(64, np.zeros(2), np.ones(2))
    assert unit[0].tolist() == [0.5, 1 / 3]
    counts = np.histogram2d(unit[:, 0], unit[:, 1], bins=4, range=[[0, 1], [0, 1]])[0]
    assert counts.min() >= 2                                              # spread over the box, not clustered


# ---------------------------------------------------------------------------------------------------------
# the host statement on models with a known optimum
# ---------------------------------------------------------------------------------------------------------

def test_first_order_term_ends_in_a_corner():
    res = opt.optimize_host(np.array([1.0, 2.0, -3.0]), np.array([[1, 0], [0, 1]]), PHIS, MINMAX, starts=8, ReturnAll=True)
    assert res.x.tolist() == [[2.0, -1.0]] and np.all(res.status_all == opt.CONVERGED)
    assert abs(res.f[0] - (1.0 + 2.0 * phi(1, 1.0) - 3.0 * phi(1, 0.0))) < 1e-12
    low = opt.optimize_host(np.array([1.0, 2.0, -3.0]), np.array([[1, 0], [0, 1]]), PHIS, MINMAX, starts=8, sense='min')
    assert low.x.tolist() == [[0.0, 3.0]]


def test_second_order_term_has_its_vertex_inside():
    c = PHIS[1]                                                           # c0 + c1 x + c2 x^2, convex
    vertex = -c[1] / (2 * c[2])
    res = opt.optimize_host(np.array([0.5, -2.0, 1.0]), np.array([[2, 0], [0, 1]]), PHIS, MINMAX, starts=5, ReturnAll=True)
    assert np.all(res.status_all == opt.CONVERGED)
    assert np.max(np.abs(res.x_all[..., 0] - 2.0 * vertex)) < 1e-9 and np.all(res.x_all[..., 1] == 3.0)
    assert abs(res.f[0] - (0.5 - 2.0 * phi(2, vertex) + phi(1, 1.0))) < 1e-12


def test_product_term_saddle_inside_maximum_on_the_boundary():
    """phi1(x) phi1(y) has its saddle in the middle of the box and equal maxima in two opposite corners."""
    betas, mtx = np.array([0.0, 1.0]), np.array([[1, 1]])
    starts = [[1.2, 1.1], [0.9, 0.8], [1.9, -0.9], [1.0, 2.0], [1.3, 0.6]]
    res = opt.optimize_host(betas, mtx, PHIS, MINMAX, starts=starts, ReturnAll=True)
    corner = phi(1, 1.0) ** 2
    assert np.all(res.status_all == opt.CONVERGED) and abs(res.f[0] - corner) < 1e-12
    ends = res.x_all[0]
    # every start ends in one of the two maximising corners: the indefinite Hessian sends none to the saddle
    assert all(e.tolist() in ([2.0, 3.0], [0.0, -1.0]) for e in ends), ends
    assert ends[0].tolist() == [2.0, 3.0] and ends[1].tolist() == [0.0, -1.0]
    # exactly on the saddle the gradient is zero: a stationary point is where a local solve stays
    saddle = opt.optimize_host(betas, mtx, PHIS, MINMAX, starts=[[1.0, 1.0]], ReturnAll=True)
    assert saddle.x.tolist() == [[1.0, 1.0]] and saddle.iterations_all[0, 0] == 0


def test_a_fixed_input_stays_fixed():
    betas, mtx = np.array([0.0, -1.0, 2.0, 1.0]), np.array([[2, 0], [0, 1], [1, 1]])
    res = opt.optimize_host(betas, mtx, PHIS, MINMAX, bounds=[[0.0, 2.0], [0.5, 0.5]], starts=6, ReturnAll=True)
    assert np.all(res.x_all[..., 1] == 0.5) and np.all(res.status_all == opt.CONVERGED)
    # with y fixed: maximise -phi2(x) + phi1(x) phi1(yn) over x: a concave parabola
    yn = (0.5 + 1.0) / 4.0
    c, c1 = PHIS[1], PHIS[0]
    xn = (c1[1] * phi(1, yn) - c[1]) / (2 * c[2])
    assert 0 < xn < 1 and abs(res.x[0, 0] - 2.0 * xn) < 1e-9
    assert abs(res.f[0] - model(betas, mtx, np.array([xn, yn]))) < 1e-12


def _projected_gradient(betas, mtx, xn, sign, lo, hi):
    g = np.zeros(xn.shape)
    for j in range(xn.shape[-1]):
        for t, row in enumerate(mtx):
            if row[j]:
                term = betas[t + 1] * phi(int(row[j]), xn[..., j], 1)
                for i, order in enumerate(row):
                    if order and i != j:
                        term = term * phi(int(order), xn[..., i])
                g[..., j] += sign * term
    return np.max(np.abs(np.clip(xn - g, lo, hi) - xn), axis=-1)


def test_multimodal_model_against_a_grid_and_scipy():
    scipy_optimize = pytest.importorskip('scipy.optimize')
    betas = toy_betas()[0]
    res = opt.optimize_host(betas, TOY_MTX, PHIS, MINMAX, starts=64, ReturnAll=True)
    assert np.all(res.status_all == opt.CONVERGED)
    low, span = np.array([0.0, -1.0]), np.array([2.0, 4.0])
    ends = (res.x_all[0] - low) / span
    assert np.all(ends >= 0) and np.all(ends <= 1)
    assert len(np.unique(np.round(ends, 6), axis=0)) >= 3                 # several local maxima are found
    assert np.max(_projected_gradient(betas, TOY_MTX, ends, -1.0, 0.0, 1.0)) < 1e-8
    assert np.max(np.abs(model(betas, TOY_MTX, ends) - res.f_all[0])) < 1e-12
    # exhaustive: the maximum of a 2 001 x 2 001 grid, refined from the best grid point
    axis = np.linspace(0.0, 1.0, 2001)
    grid = np.stack(np.meshgrid(axis, axis, indexing='ij'), axis=-1)
    values = model(betas, TOY_MTX, grid)
    at = np.unravel_index(np.argmax(values), values.shape)
    fine = scipy_optimize.minimize(lambda x: -model(betas, TOY_MTX, x), grid[at], method='L-BFGS-B',
                                   bounds=[(0, 1), (0, 1)], options=dict(ftol=1e-15, gtol=1e-12))
    assert values[at] <= res.f[0] + 1e-12 and abs(-fine.fun - res.f[0]) < 1e-8
    # start by start against L-BFGS-B from the same point.  Two local methods may settle in different basins of a
    # multimodal model; where they settle in the same one this solver's value is not below scipy's by more than 1e-8,
    # and wherever it settles it is a local maximum of the box (no feasible point nearby is higher)
    starts = opt.start_points(64, np.zeros(2), np.ones(2))
    same_basin = 0
    for s in range(64):
        ref = scipy_optimize.minimize(lambda x: -model(betas, TOY_MTX, x), starts[s], method='L-BFGS-B',
                                      bounds=[(0, 1), (0, 1)], options=dict(ftol=1e-15, gtol=1e-12))
        if np.max(np.abs(ref.x - ends[s])) < 1e-3:
            same_basin += 1
            assert res.f_all[0, s] >= -ref.fun - 1e-8, (s, res.f_all[0, s], -ref.fun)
    assert same_basin >= 24
    rng = np.random.default_rng(0)
    near = np.clip(ends[:, None, :] + 1e-4 * rng.uniform(-1, 1, (64, 200, 2)), 0.0, 1.0)
    assert np.all(model(betas, TOY_MTX, near) <= res.f_all[0][:, None] + 1e-13)


def test_draws_give_a_posterior_of_the_optimum():
    betas = toy_betas(60)
    res = opt.optimize_host(betas, TOY_MTX, PHIS, MINMAX, starts=16, ReturnAll=True)
    assert res.x.shape == (60, 2) and res.f.shape == (60,) and res.status.shape == (60,)
    assert np.array_equal(res.f, res.f_all.max(axis=1)) and np.array_equal(res.best_start, res.f_all.argmax(axis=1))
    assert np.array_equal(res.x, res.x_all[np.arange(60), res.best_start])
    cut = opt.bounds_cut(60)
    assert cut == 2 and np.array_equal(res.f_bounds, np.sort(res.f)[[cut, 60 - cut]])
    assert np.array_equal(res.x_bounds, np.sort(res.x, axis=0)[[cut, 60 - cut]].T)
    assert res.f_mean == res.f.mean() and np.array_equal(res.x_mean, res.x.mean(axis=0))
    # 'mean' is 'draws' of the averaged row, with scalars out
    mean = opt.optimize_host(betas, TOY_MTX, PHIS, MINMAX, starts=16, objective='mean')
    one = opt.optimize_host(betas.mean(axis=0), TOY_MTX, PHIS, MINMAX, starts=16)
    assert mean.x.shape == (2,) and np.isscalar(mean.f) and mean.status == opt.CONVERGED
    assert np.array_equal(mean.x, one.x[0]) and mean.f == one.f[0] and 'f_bounds' not in mean and 'f_bounds' not in one
    # the iteration limit is a status, not an error
    short = opt.optimize_host(betas[:4], TOY_MTX, PHIS, MINMAX, starts=16, max_iter=1, ReturnAll=True)
    assert set(np.unique(short.status_all)) <= {opt.CONVERGED, opt.ITERATION_LIMIT} and opt.ITERATION_LIMIT in short.status_all
    assert np.all(short.iterations_all <= 1)


def test_terms_of_any_width():
    """A term with four factors and a row of zeros (a second constant) go through the same sums."""
    rng = np.random.default_rng(5)
    mtx = np.array([[1, 1, 1, 1], [2, 0, 1, 0], [0, 0, 0, 0], [0, 3, 0, 2], [1, 2, 2, 1]])
    betas = rng.standard_normal(6)
    mm = [[0.0, 1.0]] * 4
    res = opt.optimize_host(betas, mtx, PHIS, mm, starts=24, ReturnAll=True)
    ends = res.x_all[0]
    assert np.all(np.isin(res.status_all, (opt.CONVERGED, opt.STALLED)))
    ok = res.status_all[0] == opt.CONVERGED
    assert ok.sum() >= 20 and np.max(_projected_gradient(betas, mtx, ends[ok], -1.0, 0.0, 1.0)) < 1e-8
    assert np.max(np.abs(model(betas, mtx, ends) - res.f_all[0])) < 1e-12
    brute = model(betas, mtx, rng.random((200000, 4))).max()
    assert res.f[0] >= brute


# ---------------------------------------------------------------------------------------------------------
# the method of the class
# ---------------------------------------------------------------------------------------------------------

class _Backend:
    def __init__(self):
        self.ctx = _NoDevice()


def test_the_method_hands_the_model_over():
    m = FoKL(kernel='Bernoulli Polynomials', UserWarnings=False)
    m.betas, m.mtx, m.minmax = toy_betas(9), TOY_MTX, MINMAX
    m._backend_override = _Backend()
    with pytest.raises(_Reached) as hit:
        m.optimize(bounds=[[1.0, 2.0], [-1.0, 1.0]], starts=5, sense='min')
    mtx, b, table, lo, hi, starts, sign = hit.value.args[:7]
    assert np.array_equal(b, m.betas) and np.array_equal(mtx, TOY_MTX) and sign == 1.0
    assert lo.tolist() == [0.5, 0.0] and hi.tolist() == [1.0, 0.5] and starts.shape == (5, 2)
    with pytest.raises(ValueError, match='Cubic Splines'):
        spline = FoKL(UserWarnings=False)
        spline.betas, spline.mtx, spline.minmax = toy_betas(2), TOY_MTX, MINMAX
        spline._backend_override = _Backend()
        spline.optimize()
    with pytest.raises(NotImplementedError):
        m.to_pyomo()


def test_true_scale_round_trip(monkeypatch):
    """The context sees normalised coordinates, the caller true-scale ones: the host statement stands in for the device."""
    m = FoKL(kernel='Bernoulli Polynomials', UserWarnings=False)
    m.betas, m.mtx, m.minmax = toy_betas(6), TOY_MTX, MINMAX

    class Host(_capi.DeviceContext):
        def __init__(self):
            self._h = None

        def model_optimize(self, *args):
            self.args = args
            return opt.solve_host(*args)

    backend = _Backend()
    backend.ctx = Host()
    m._backend_override = backend
    box = [[0.25, 1.75], [0.0, 3.0]]
    res = m.optimize(bounds=box, starts=12, ReturnAll=True)
    lo, hi = backend.ctx.args[3], backend.ctx.args[4]
    assert np.allclose(lo, [0.125, 0.25]) and np.allclose(hi, [0.875, 1.0])
    assert np.all(res.x_all >= np.array(box)[:, 0]) and np.all(res.x_all <= np.array(box)[:, 1])
    xn = (res.x - np.array([0.0, -1.0])) / np.array([2.0, 4.0])
    for e in range(6):
        assert abs(model(m.betas[e], TOY_MTX, xn[e]) - res.f[e]) < 1e-12
    same = opt.optimize_host(m.betas, TOY_MTX, PHIS, MINMAX, bounds=box, starts=12, ReturnAll=True)
    assert np.array_equal(same.x_all, res.x_all) and np.array_equal(same.f_all, res.f_all)
    # a point on a face of the box is reported ON it, not an ulp beside it
    on_lower = res.x_all[..., 0][np.isclose(res.x_all[..., 0], 0.25)]
    assert np.all(on_lower == 0.25)

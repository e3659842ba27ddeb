"""Propagating a population through every posterior draw, without a device: every argument check, the host statement
(population.propagate_host, what the kernel is tested against) against a direct numpy computation on Bernoulli and
spline models, the quantile brackets, the variance shares on a full-factorial grid, and the bounds over the draws."""
import numpy as np
import pytest

from fokl_gpy_amd import getKernels
from fokl_gpy_amd import population as pop
from fokl_gpy_amd.FoKLRoutines import FoKL
from fokl_gpy_amd.GP_Integrate import bounds_cut
from fokl_gpy_amd.embedded import basis_matrix

BERNOULLI, SPLINES = getKernels.bernoulli(), getKernels.sp500()
KERNELS = {'Bernoulli Polynomials': BERNOULLI, 'Cubic Splines': SPLINES}
MTX = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [1, 1, 0], [0, 2, 1], [3, 0, 0]])


def case(kernel='Bernoulli Polynomials', S=500, E=37, seed=0, mtx=MTX):
    rng = np.random.default_rng(seed)
    x = rng.random((S, mtx.shape[1]))
    mean = rng.standard_normal(mtx.shape[0] + 1)
    betas = mean * (1 + 0.2 * rng.standard_normal((E, mean.shape[0])))
    X = basis_matrix(x, mtx, KERNELS[kernel], kernel)
    data = X @ mean + 0.1 * rng.standard_normal(S)
    return dict(betas=betas, mtx=mtx, phis=KERNELS[kernel], kernel=kernel, inputs=x), data, X @ betas.T


# ---------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('change, text', [
    (dict(inputs=np.zeros((10, 2))), 'columns'),
    (dict(inputs=np.zeros((0, 3))), 'at least one row'),
    (dict(inputs=None), 'population'),
    (dict(data=np.zeros(11)), 'one finite value per row'),
    (dict(betas=np.zeros((5, 3))), 'terms \\+ 1'),
    (dict(quantiles=(0.0, 0.5)), 'strictly inside'),
    (dict(quantiles=(0.5, 1.0)), 'strictly inside'),
    (dict(quantiles=np.linspace(0.01, 0.99, 33)), 'strictly inside'),
    (dict(thresholds=np.arange(33.0)), 'at most 32 thresholds'),
    (dict(thresholds=[0.0, np.inf]), 'finite'),
    (dict(thresholds=[np.nan]), 'finite'),
    (dict(passes=0), 'passes'),
    (dict(passes=1.5), 'passes'),
    (dict(draws=0), 'draws'),
    (dict(draws=38), 'draws'),
    (dict(kernel='Fourier'), 'not currently supported'),
    (dict(mtx=np.array([[99, 0, 0]]), betas=np.zeros((4, 2))), 'orders outside'),
])
def test_argument_errors_are_value_errors(change, text):
    kw, _, _ = case(S=10)
    kw.update(change)
    with pytest.raises(ValueError, match=text):
        pop.propagate_host(**kw)


class _Untouchable:
    """Stands where the backend would be: a refused call must not reach it."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was reached ({name}) before the arguments were checked")


def test_errors_come_before_anything_is_uploaded():
    kw, _, _ = case(S=10)
    for change in (dict(passes=0), dict(quantiles=(1.5,)), dict(thresholds=np.arange(40.0)), dict(data=np.zeros(3)),
                   dict(inputs=np.zeros((10, 5)))):
        with pytest.raises(ValueError):
            pop._prepare(**{**dict(data=None, thresholds=None, quantiles=(0.5,), passes=3, draws=None), **kw, **change})
    model = FoKL(kernel='Bernoulli Polynomials', UserWarnings=False, ConsoleOutput=False)
    model.betas, model.mtx, model.inputs = kw['betas'], kw['mtx'], kw['inputs']
    model._backend_override = _Untouchable()
    with pytest.raises(ValueError, match='passes'):
        model.propagate(passes=0)
    with pytest.raises(ValueError, match='at most 32'):
        model.propagate(thresholds=np.arange(33.0))


def test_spline_inputs_outside_the_unit_box_are_refused():
    kw, _, _ = case('Cubic Splines', S=10)
    kw['inputs'] = kw['inputs'] + 0.5
    with pytest.raises(ValueError, match='normalized'):
        pop.propagate_host(**kw)


def test_draws_none_uses_all_rows_and_touches_no_random_state():
    kw, _, Y = case()
    np.random.seed(11)
    before = np.random.get_state()
    res = pop.propagate_host(**kw)
    last = pop.propagate_host(draws=5, **kw)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert res.mean.shape == (37,) and np.allclose(res.mean, Y.mean(axis=0), atol=1e-13)
    assert np.array_equal(last.mean, pop.propagate_host(**{**kw, 'betas': kw['betas'][-5:]}).mean)
    assert np.allclose(last.mean, Y.mean(axis=0)[-5:], atol=1e-13)


class _HostBackend:
    """A backend whose launches are the host statement: the method's own plumbing, without a device."""

    def __init__(self):
        self.uploads = 0

    def upload(self, inputs, data, kid, packed, nb, width):
        self.x, self.y, self.kid, self.uploads = inputs, data, kid, self.uploads + 1

    def reserve_slots(self, count):
        pass

    def build_terms(self, terms, slots):
        kernel = 'Cubic Splines' if self.kid == getKernels.KERNEL_SPLINES else 'Bernoulli Polynomials'
        self.X = basis_matrix(self.x, terms, KERNELS[kernel], kernel)

    def population_stats(self, slots, betas, shift, cuts, with_data):
        assert list(slots) == [0] + list(range(2, 2 + self.X.shape[1] - 1))
        return pop.population_stats_host(self.X, betas, shift, cuts, self.y if with_data else None)[:2]

    def gram(self, rows, cols):
        return self.X.T @ self.X


def test_the_method_fills_in_the_model_and_leaves_setnos_alone():
    kw, data, Y = case()
    model = FoKL(kernel='Bernoulli Polynomials', UserWarnings=False, ConsoleOutput=False)
    model.betas, model.mtx, model.inputs, model.data = kw['betas'], kw['mtx'], kw['inputs'], data
    model.minmax = [[0.0, 2.0]] * 3
    model._backend_override = _HostBackend()
    assert model.setnos is None
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    res = model.propagate(data=model.data, thresholds=[0.0])
    assert model.setnos is None and np.array_equal(np.random.get_state()[1], state)
    assert np.allclose(res.mean, Y.mean(axis=0), atol=1e-13)
    assert np.allclose(res.rmse, np.sqrt(((data[:, None] - Y) ** 2).mean(axis=0)), rtol=1e-12)
    # clean=True normalises with the model's minmax, as evaluate does
    raw = 2.0 * kw['inputs']
    cleaned = model.propagate(inputs=raw, clean=True, quantiles=None)
    assert np.allclose(cleaned.mean, res.mean, atol=1e-12)
    assert np.allclose(model.inputs, kw['inputs'])


# ---------------------------------------------------------------------------------------------------------
# the host statement against a direct computation
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kernel', list(KERNELS))
def test_moments_exceedance_and_rmse_against_numpy(kernel):
    kw, data, Y = case(kernel, S=777, E=41, seed=4)
    thr = np.quantile(Y, [0.1, 0.5, 0.9])
    res = pop.propagate_host(data=data, thresholds=thr, **kw)
    scale = np.abs(Y).max()
    assert np.max(np.abs(res.mean - Y.mean(axis=0))) < 1e-12 * scale
    assert np.max(np.abs(res.var - Y.var(axis=0))) < 1e-12 * scale ** 2
    assert np.max(np.abs(res['min'] - Y.min(axis=0))) < 1e-13 * scale
    assert np.max(np.abs(res['max'] - Y.max(axis=0))) < 1e-13 * scale
    assert np.array_equal(res.exceed, (Y[:, :, None] > thr).mean(axis=0))
    resid = data[:, None] - Y
    assert np.allclose(res.sse, (resid ** 2).sum(axis=0), rtol=1e-12)
    assert np.allclose(res.rmse, np.sqrt((resid ** 2).mean(axis=0)), rtol=1e-12)
    assert np.allclose(res.r2, 1 - (resid ** 2).sum(axis=0) / ((data - data.mean()) ** 2).sum(), rtol=1e-12, atol=1e-12)
    assert res.launches == 1 + 1 + 3


def test_var_survives_a_mean_far_from_the_intercept():
    """The second moment is accumulated about the draw's mean, not about zero or the intercept."""
    kw, _, _ = case(S=400, E=8)
    kw['inputs'] = 0.9 + 0.1 * kw['inputs'] * 1e-3                           # a narrow population far from the basis' zero mean
    Y = basis_matrix(kw['inputs'], kw['mtx'], BERNOULLI, kw['kernel']) @ kw['betas'].T
    res = pop.propagate_host(quantiles=None, **kw)
    assert res.launches == 2
    assert np.allclose(res.var, Y.var(axis=0), rtol=1e-6, atol=0)            # relative to the tiny variance itself


def test_intercept_only_and_one_draw():
    rng = np.random.default_rng(0)
    res = pop.propagate_host(np.array([[1.5]]), np.zeros((0, 2)), BERNOULLI, 'Bernoulli Polynomials', rng.random((9, 2)),
                             thresholds=[1.0, 2.0], sensitivity=True)
    assert res.mean.tolist() == [1.5] and res.var.tolist() == [0.0] and res.exceed.tolist() == [[1.0, 0.0]]
    assert res.components == [] and res.shares.shape == (1, 0) and 'mean_bounds' not in res
    assert np.allclose(res.quantiles, 1.5)


@pytest.mark.parametrize('kernel', list(KERNELS))
def test_order_statistics_lie_in_their_brackets_which_shrink(kernel):
    kw, _, Y = case(kernel, S=1234, E=23, seed=9)
    q = (0.001, 0.025, 0.5, 0.9, 0.999)
    srt = np.sort(Y, axis=0)
    k = np.ceil(np.array(q) * Y.shape[0]).astype(int)
    exact = srt[k - 1].T                                                     # [E, Q]
    span = srt[-1] - srt[0]
    widths = []
    for passes in (1, 2, 3, 4):
        res = pop.propagate_host(quantiles=q, passes=passes, **kw)
        lo, hi = res.quantile_brackets[..., 0], res.quantile_brackets[..., 1]
        assert np.all(lo <= exact) and np.all(exact <= hi)
        assert np.all((lo <= res.quantiles) & (res.quantiles <= hi))
        widths.append(np.max((hi - lo) / span[:, None]))
    assert widths[0] <= 1 / 33 + 1e-12 and all(b < a / 4 for a, b in zip(widths, widths[1:]))
    res = pop.propagate_host(quantiles=(0.025, 0.5, 0.975), **kw)
    assert np.max((res.quantile_brackets[..., 1] - res.quantile_brackets[..., 0]) / span[:, None]) < 1 / 3900
    assert res.quantile_levels.tolist() == [0.025, 0.5, 0.975]


def test_quantiles_of_a_constant_output():
    res = pop.propagate_host(np.array([[2.0, 0.0], [3.0, 0.0]]), np.array([[1]]), BERNOULLI, 'Bernoulli Polynomials',
                             np.linspace(0, 1, 50)[:, None])
    assert np.array_equal(res.quantiles, [[2.0] * 3, [3.0] * 3])


# ---------------------------------------------------------------------------------------------------------
# shares
# ---------------------------------------------------------------------------------------------------------

def test_components_of_an_interaction_matrix():
    comps, of_term = pop.components_of(MTX)
    assert comps == [(0,), (1,), (2,), (0, 1), (1, 2)]
    assert of_term.tolist() == [0, 1, 2, 0, 3, 4, 0]
    assert pop.components_of(np.zeros((0, 3)))[0] == []


def test_shares_on_a_full_factorial_grid_are_the_variance_fractions():
    """Main effects plus one interaction of functions centred over the grid: the components are uncorrelated there."""
    g = (np.arange(12) + 0.5) / 12                                           # symmetric about 1/2: odd orders centre exactly
    grid = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    mtx = np.array([[1, 0, 0], [3, 0, 0], [0, 1, 0], [0, 0, 3], [1, 0, 1]])
    rng = np.random.default_rng(2)
    betas = rng.standard_normal((9, 6))
    res = pop.propagate_host(betas, mtx, BERNOULLI, 'Bernoulli Polynomials', grid, sensitivity=True, quantiles=None)
    assert res.components == [(0,), (1,), (2,), (0, 2)]
    X = basis_matrix(grid, mtx, BERNOULLI, 'Bernoulli Polynomials')
    Y = X @ betas.T
    parts = [X[:, [1, 2]] @ betas[:, [1, 2]].T, X[:, [3]] @ betas[:, [3]].T, X[:, [4]] @ betas[:, [4]].T,
             X[:, [5]] @ betas[:, [5]].T]
    direct = np.stack([f.var(axis=0) for f in parts], axis=1) / Y.var(axis=0)[:, None]
    assert np.allclose(res.shares, direct, atol=1e-12)
    assert np.allclose(res.shares.sum(axis=1), 1.0, atol=1e-12)
    assert np.allclose(res.var_gram, res.var, rtol=1e-11)
    by_input = np.stack([res.shares[:, 0] + res.shares[:, 3], res.shares[:, 1], res.shares[:, 2] + res.shares[:, 3]], axis=1)
    assert np.allclose(res.shares_by_input, by_input, atol=1e-15)


def test_shares_sum_to_one_on_a_correlated_population():
    kw, _, Y = case(S=300, E=12, seed=6)
    kw['inputs'][:, 1] = 0.5 * kw['inputs'][:, 0] + 0.5 * kw['inputs'][:, 1]
    res = pop.propagate_host(sensitivity=True, **kw)
    assert np.allclose(res.shares.sum(axis=1), 1.0, atol=1e-12)
    assert res.shares.shape == (12, 5) and res.shares_by_input.shape == (12, 3)
    assert np.allclose(res.var_gram, res.var, rtol=1e-10)


# ---------------------------------------------------------------------------------------------------------
# bounds over the draws
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [2, 39, 40, 200])
def test_bounds_follow_the_rule_of_evaluate(E):
    kw, data, _ = case(S=60, E=E, seed=E)
    res = pop.propagate_host(data=data, thresholds=[0.0, 0.5], sensitivity=True, **kw)
    cut = bounds_cut(E)
    for name in ('mean', 'var', 'min', 'max', 'exceed', 'quantiles', 'sse', 'rmse', 'r2', 'shares', 'shares_by_input'):
        srt = np.sort(res[name], axis=0)
        assert np.array_equal(res[name + '_bounds'], np.stack([srt[cut], srt[E - cut]], axis=-1)), name
        assert np.array_equal(res[name + '_mean'], res[name].mean(axis=0)), name
        assert res[name + '_bounds'].shape == res[name].shape[1:] + (2,)


def test_one_draw_or_no_request_returns_no_bounds():
    kw, _, _ = case(S=60, E=1)
    assert not [key for key in pop.propagate_host(**kw) if key.endswith('_bounds')]
    kw, _, _ = case(S=60, E=5)
    assert not [key for key in pop.propagate_host(ReturnBounds=False, **kw) if key.endswith('_bounds')]


def test_the_statement_of_the_counts_reports_values_next_to_a_cut():
    X = np.ones((4, 1))
    betas = np.array([[1.0], [2.0]])
    mom, above, near = pop.population_stats_host(X, betas, np.zeros(2), np.array([[1.0, 0.5], [2.0 + 1e-12, 3.0]]))
    assert above.tolist() == [[0, 4], [0, 0]] and near.tolist() == [[4, 0], [4, 0]]
    assert mom[:, 0].tolist() == [4.0, 8.0] and mom[:, 1].tolist() == [4.0, 16.0] and mom[:, 4:].tolist() == [[0, 0], [0, 0]]

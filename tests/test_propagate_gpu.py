"""fokl_population_stats (csrc/fokl_population.inc) and population.propagate on the device against their host statement.

Two references for the kernel:
  * exact -- columns, coefficients and shifts are small integers and the cuts lie at half-integers, so every value, sum and
    count is exactly representable whatever the order of summation: ``np.array_equal`` on every output.  This pins the
    lane map of the swapped MFMA operands (a lane holds four rows of ONE draw), the masking of rows past the end and of
    padding draws, and the fixed-order sum over the row chunks.
  * rounded -- continuous data against population_stats_host: moments to 1e-12 of the output's scale, min / max to 1e-13,
    counts within the number of values the statement reports next to a cut.
``DeviceContext.population_report`` says where the coefficients lived, so that both placements are known to have run.
"""
import warnings

import numpy as np
import pytest

from helpers import upload, load_columns
from fokl_gpy_amd import _capi, getKernels, FoKLRoutines
from fokl_gpy_amd import population as pop
from fokl_gpy_amd.embedded import basis_matrix
from oracle import fokl_oracle as O

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 1000, 100003)
DRAWS = (1, 15, 16, 17, 64, 1000, 1003)
WIDTHS = (1, 2, 5, 100, 128, 129, 300, 600)


def stage(ctx, cols, y=None):
    """cols [n, k] -> slots 2 .. k + 1 of a fresh dataset; -> the slot list and X of [intercept] + cols."""
    n = cols.shape[0]
    upload(ctx, np.linspace(0.0, 1.0, n).reshape(n, 1), np.zeros(n) if y is None else y, O.KERNEL_BERNOULLI)
    if cols.shape[1]:
        load_columns(ctx, cols)
    slots = np.concatenate([[_capi.SLOT_ONES], np.arange(2, 2 + cols.shape[1])]).astype(np.int32)
    return slots, np.concatenate([np.ones((n, 1)), cols], axis=1)


def integer_case(S, E, nc, K, seed):
    rng = np.random.default_rng(seed)
    cols = rng.integers(-3, 4, size=(S, nc - 1)).astype(np.float64)
    betas = rng.integers(-3, 4, size=(E, nc)).astype(np.float64)
    y = rng.integers(-20, 21, size=S).astype(np.float64)
    shift = rng.integers(-5, 6, size=E).astype(np.float64)
    spread = max(1, int(3 * np.sqrt(nc)))
    cuts = rng.integers(-spread, spread + 1, size=(E, K)).astype(np.float64) + 0.5
    return cols, betas, y, shift, cuts


def check_exact(ctx, S, E, nc, K, with_data, seed=0):
    cols, betas, y, shift, cuts = integer_case(S, E, nc, K, seed)
    slots, X = stage(ctx, cols, y)
    mom, above = ctx.population_stats(slots, betas, shift, cuts, with_data)
    ref_mom, ref_above, near = pop.population_stats_host(X, betas, shift, cuts, y if with_data else None)
    assert near.sum() == 0
    assert np.array_equal(mom, ref_mom), (S, E, nc, K, with_data)
    assert np.array_equal(above, ref_above), (S, E, nc, K, with_data)
    assert above.dtype == np.int64 and above.shape == (E, K) and mom.shape == (E, 6)
    rep = ctx.population_report()
    assert rep['coefficients'] == ('registers' if nc <= 128 else 'table')
    assert rep['draw_blocks'] == -(-E // 128) and rep['row_tiles'] == -(-S // 16)
    assert rep['grid'] == -(-rep['chunks'] // 8) * 8 * rep['draw_blocks']
    assert rep['chunks'] * rep['tiles_per_chunk'] >= rep['row_tiles'] > (rep['chunks'] - 1) * rep['tiles_per_chunk']
    return rep


def test_the_lane_map_a_lane_holds_rows_of_one_draw(device_ctx):
    """y[row][draw] = draw + 1000 row: were rows and draws (or a lane's four rows) placed otherwise, min, max and the sums
    of a draw would be another draw's."""
    S, E = 37, 21
    slots, X = stage(device_ctx, np.arange(S, dtype=np.float64)[:, None])
    betas = np.stack([np.arange(E, dtype=np.float64), np.full(E, 1000.0)], axis=1)
    cuts = np.arange(E, dtype=np.float64)[:, None] + 1000.0 * np.array([0, 4, 17, 36]) + 0.5
    mom, above = device_ctx.population_stats(slots, betas, np.zeros(E), cuts)
    d = np.arange(E)
    assert np.array_equal(mom[:, 2], d) and np.array_equal(mom[:, 3], d + 1000.0 * (S - 1))
    assert np.array_equal(mom[:, 0], S * d + 1000.0 * S * (S - 1) / 2)
    assert np.array_equal(mom[:, 1], ((d[None, :] + 1000.0 * np.arange(S)[:, None]) ** 2).sum(axis=0))
    assert np.array_equal(above, np.tile([S - 1, S - 5, S - 18, 0], (E, 1)))


@pytest.mark.parametrize('S', ROWS[:5])
@pytest.mark.parametrize('E', DRAWS)
def test_exact_over_rows_and_draws(device_ctx, S, E):
    check_exact(device_ctx, S, E, nc=5, K=1, with_data=bool((S + E) & 1), seed=S + E)


@pytest.mark.parametrize('E', (1, 64, 1003))
def test_exact_over_many_rows_the_tile_loop_goes_round(device_ctx, E):
    rep = check_exact(device_ctx, ROWS[5], E, nc=5, K=1, with_data=True, seed=E)
    assert rep['tiles_per_chunk'] > 1


@pytest.mark.parametrize('nc', WIDTHS)
@pytest.mark.parametrize('S, E', [(17, 17), (1000, 64)])
def test_exact_over_widths_both_coefficient_placements(device_ctx, nc, S, E):
    check_exact(device_ctx, S, E, nc, K=32, with_data=True, seed=nc)


@pytest.mark.parametrize('K', (0, 1, 8, 9, 32))
@pytest.mark.parametrize('with_data', (False, True))
def test_exact_over_cut_counts_with_and_without_data(device_ctx, K, with_data):
    check_exact(device_ctx, 1000, 17, 5, K, with_data, seed=K)
    check_exact(device_ctx, 16, 130, 300, K, with_data, seed=K + 1)


def test_exact_beyond_one_piece_of_columns(device_ctx):
    rep = check_exact(device_ctx, 40, 20, 1100, 3, True)
    assert rep['pieces'] == 2 and rep['coefficients'] == 'table'


def test_without_data_the_residual_sums_are_zero(device_ctx):
    cols, betas, y, shift, cuts = integer_case(100, 5, 3, 2, 0)
    slots, _ = stage(device_ctx, cols, y)
    mom, _ = device_ctx.population_stats(slots, betas, shift, cuts, False)
    assert np.array_equal(mom[:, 4:], np.zeros((5, 2)))


@pytest.mark.parametrize('S, E, nc, K', [(1000, 64, 100, 32), (100003, 200, 100, 32), (1000, 1003, 5, 1), (17, 1000, 600, 32),
                                         (100003, 17, 300, 1), (15, 15, 2, 0), (1, 1, 1, 1)])
def test_rounded_against_the_host_statement(device_ctx, S, E, nc, K):
    rng = np.random.default_rng(S + E + nc)
    cols = rng.standard_normal((S, nc - 1))
    betas = rng.standard_normal((E, nc)) / np.sqrt(nc)
    y = rng.standard_normal(S)
    slots, X = stage(device_ctx, cols, y)
    Ymean = X.mean(axis=0) @ betas.T
    shift = Ymean + 0.01 * rng.standard_normal(E)
    cuts = Ymean[:, None] + rng.standard_normal((E, K))
    mom, above = device_ctx.population_stats(slots, betas, shift, cuts, True)
    ref, ref_above, near = pop.population_stats_host(X, betas, shift, cuts, y)
    scale = max(np.abs(ref[:, 2:4]).max(), np.abs(y).max(), 1e-300)
    assert np.max(np.abs(mom[:, 0] - ref[:, 0])) <= 1e-12 * scale * S
    assert np.max(np.abs(mom[:, 1] - ref[:, 1])) <= 1e-12 * scale ** 2 * S
    assert np.max(np.abs(mom[:, 2:4] - ref[:, 2:4])) <= 1e-13 * scale
    assert np.max(np.abs(mom[:, 4] - ref[:, 4])) <= 1e-12 * scale * S
    assert np.max(np.abs(mom[:, 5] - ref[:, 5])) <= 1e-12 * scale ** 2 * S
    assert np.all(np.abs(above - ref_above) <= near)
    again = device_ctx.population_stats(slots, betas, shift, cuts, True)
    assert np.array_equal(again[0], mom) and np.array_equal(again[1], above)          # no atomics: the same bits


def test_refusals(device_ctx):
    cols, betas, y, shift, cuts = integer_case(50, 4, 3, 2, 0)
    slots, _ = stage(device_ctx, cols, y)
    with pytest.raises(ValueError):
        device_ctx.population_stats(slots, betas, shift, np.zeros((4, 33)))
    with pytest.raises(ValueError):
        device_ctx.population_stats(slots, betas[:, :2], shift, cuts)
    with pytest.raises(_capi.FoklNativeError):
        device_ctx.population_stats(np.array([0, 2, 9999], dtype=np.int32), betas, shift, cuts)
    assert device_ctx.population_report()['coefficients'] == 'none' and device_ctx.population_report()['grid'] == 0
    before = device_ctx.population_stats(slots, betas, shift, cuts, True)
    for bad in (np.nan, np.inf):                             # draws of a flagged chain, or overflowed ones: refused natively
        spoiled = betas.copy()
        spoiled[-1, -1] = bad
        with pytest.raises(_capi.FoklNativeError, match='fokl_population_stats: every coefficient must be finite') as exc:
            device_ctx.population_stats(slots, spoiled, shift, cuts, True)
        assert exc.value.code == -2
        assert device_ctx.population_report()['coefficients'] == 'none' and device_ctx.population_report()['grid'] == 0
        assert np.array_equal(device_ctx.read_slot(2), cols[:, 0]) and np.array_equal(device_ctx.read_slot(_capi.SLOT_Y), y)
        again = device_ctx.population_stats(slots, betas, shift, cuts, True)
        assert np.array_equal(again[0], before[0]) and np.array_equal(again[1], before[1])
    device_ctx.population_stats(slots, betas, shift, cuts)
    assert device_ctx.population_report()['coefficients'] == 'registers'


# ---------------------------------------------------------------------------------------------------------
# propagate on the device against propagate_host
# ---------------------------------------------------------------------------------------------------------

MTX = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [1, 1, 0], [0, 2, 1], [3, 0, 0]])


@pytest.mark.parametrize('kernel, phis', [('Bernoulli Polynomials', getKernels.bernoulli()), ('Cubic Splines', getKernels.sp500())])
def test_propagate_equals_its_host_statement(kernel, phis):
    rng = np.random.default_rng(3)
    S, E = 5003, 150
    x = rng.random((S, 3))
    mean = rng.standard_normal(8)
    betas = mean * (1 + 0.2 * rng.standard_normal((E, 8)))
    X = basis_matrix(x, MTX, phis, kernel)
    Y = X @ betas.T
    data = X @ mean + 0.1 * rng.standard_normal(S)
    thr = np.quantile(Y, [0.2, 0.7])
    kw = dict(betas=betas, mtx=MTX, phis=phis, kernel=kernel, inputs=x, data=data, thresholds=thr, sensitivity=True)
    dev, host = pop.propagate(**kw), pop.propagate_host(**kw)
    assert sorted(dev.keys()) == sorted(host.keys()) and dev.components == host.components
    scale = np.abs(Y).max()
    for name, tol in (('mean', 1e-12 * scale), ('var', 1e-12 * scale ** 2), ('min', 1e-13 * scale), ('max', 1e-13 * scale),
                      ('sse', 1e-12 * scale ** 2 * S), ('rmse', 1e-12 * scale), ('r2', 1e-11), ('exceed', 2.5 / S),
                      ('shares', 1e-9), ('shares_by_input', 1e-9), ('var_gram', 1e-10 * scale ** 2)):
        assert np.max(np.abs(dev[name] - host[name])) <= tol, name
        if name != 'var_gram':
            assert np.max(np.abs(dev[name + '_bounds'] - host[name + '_bounds'])) <= tol, name
    assert np.allclose(dev.var_gram, dev.var, rtol=1e-10)
    assert np.allclose(dev.shares.sum(axis=1), 1.0, atol=1e-10)
    srt = np.sort(Y, axis=0)
    exact = srt[np.ceil(np.array([0.025, 0.5, 0.975]) * S).astype(int) - 1].T
    lo, hi = dev.quantile_brackets[..., 0], dev.quantile_brackets[..., 1]
    slack = 1e-12 * scale
    assert np.all(lo - slack <= exact) and np.all(exact <= hi + slack)
    assert np.max((hi - lo) / (srt[-1] - srt[0])[:, None]) < 1 / 3900
    assert np.max(np.abs(dev.quantiles - host.quantiles)) <= np.max(hi - lo)
    assert dev.launches == host.launches == 5


def test_propagate_after_a_fit():
    rng = np.random.default_rng(2024)
    n = 2000
    x = rng.random((n, 3))
    y = np.sin(4 * x[:, 0]) + x[:, 1] * x[:, 2] + 0.05 * rng.standard_normal(n)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', burnin=60, draws=60, UserWarnings=False, ConsoleOutput=False)
        np.random.seed(7)
        model.fit(x, y, clean=True)
        state = np.random.get_state()[1].copy()
        res = model.propagate(data=model.data, sensitivity=True, thresholds=[float(np.median(y))])
        assert model.setnos is None and np.array_equal(np.random.get_state()[1], state)
        E = model.betas.shape[0]
        assert res.mean.shape == (E,) and res.shares.shape == (E, len(res.components))
        assert np.allclose(res.var_gram, res.var, rtol=1e-10)
        assert np.allclose(res.shares.sum(axis=1), 1.0, atol=1e-10)
        assert np.all(res.rmse < 0.2) and np.all(res.r2 > 0.9)
        assert 0.3 < res.exceed_mean[0] < 0.7
        host = pop.propagate_host(model.betas, model.mtx, model.phis, model.kernel, model.inputs, data=model.data)
        assert np.allclose(res.mean, host.mean, atol=1e-12) and np.allclose(res.rmse, host.rmse, rtol=1e-11)
        every_draw = model.evaluate(draws=E)                                 # the mean over all draws, row by row
        assert abs(res.mean.mean() - every_draw.mean()) < 1e-12 * max(1.0, np.abs(every_draw).max())
        # raw inputs with clean=True: the model's own normalisation
        again = model.propagate(inputs=x, clean=True, data=model.data, quantiles=None)
        assert np.allclose(again.mean, res.mean, atol=1e-12)

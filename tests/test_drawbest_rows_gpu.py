"""fokl_drawbest_rows (csrc/fokl_drawbest_device.inc) called directly, against its statement pooloptimum.ranks_host.

On ``integer_case`` data every f is an exact integer in any summation order, so index and value must be the statement's
bits: rows around a tile, widths around the register / table plans and up to the column limit, draws around a
workgroup's block of 128.  On continuous data the device's sums run in another order; a row may then differ from numpy's
only where two values tie to rounding, within the forward error bound of two dot products (derived, not measured):
tol_d = 2 gamma_nc max_s sum_k |x_sk beta_dk|, gamma_nc = nc u / (1 - nc u), u = 2^-53.
"""
import numpy as np
import pytest

from test_score_gpu import stage
from test_acquire_host import continuous_case, integer_case
from test_optimize_pool_host import inf_case
from fokl_gpy_amd import _capi
from fokl_gpy_amd import pooloptimum as po

pytestmark = pytest.mark.gpu

LIMIT = _capi.DRAWBEST_MAX_COLUMNS
ROWS = (1, 15, 16, 17, 1029)
WIDTHS = tuple(sorted({1, 3, 4, 5, 17, 128, 129, 513, 1280, LIMIT}))
DRAWS = (1, 15, 16, 17, 127, 128, 129, 1000)


def tolerance(X, betas):
    """tol [E]: the forward error bound of two dot products of nc terms, at the largest sum of magnitudes over the rows."""
    nc = X.shape[1]
    gamma = nc * 2.0 ** -53 / (1.0 - nc * 2.0 ** -53)
    return 2.0 * gamma * (np.abs(X) @ np.abs(betas).T).max(axis=0)


def check_report(ctx, S, nc, E, ranks):
    rep = ctx.drawbest_report()
    ncp = -(-nc // 4) * 4
    assert rep['instance'] == 'ran' and rep['ranks'] == ranks
    assert rep['row_tiles'] == -(-S // 16) and rep['draw_blocks'] == -(-E // 128)
    assert 1 <= rep['row_chunks'] <= rep['row_tiles'] and rep['row_chunks'] * rep['tiles_per_chunk'] >= rep['row_tiles']
    assert rep['grid'] == -(-rep['row_chunks'] // 8) * 8 * rep['draw_blocks'] and rep['merge_grid'] == -(-E // 256)
    assert rep['lds_bytes'] == 8 * 16 * ncp and rep['coefficients'] == ('registers' if ncp <= 128 else 'table')
    assert rep['launches'] == 2 * ranks                          # as DeviceContext.drawbest_rows' docstring states
    assert rep['kernel_us'] > 0
    return rep


def check_exact(ctx, S, nc, E, seed=0):
    """ranks 1 and 6, without and with a mask that removes the best rows of the first draws: the statement's bits."""
    X, betas, _ = integer_case(seed, S, nc, E)
    slots, staged = stage(ctx, X[:, 1:], np.zeros(S))
    assert np.array_equal(staged, X)
    mask = np.zeros(S, dtype=np.uint8)
    mask[np.unique(po.ranks_host(X, betas[:3])['index'])] = 1
    if mask.all():
        mask = None                                              # a pool of one row: nothing would be left
    for ranks in (1, 6):
        for m in (None, mask) if mask is not None else (None,):
            want = po.ranks_host(X, betas, ranks, m)
            got = ctx.drawbest_rows(slots, betas, m, ranks)
            assert got['index'].dtype == np.int64 and np.array_equal(got['index'], want['index']), (ranks, m is not None)
            assert got['value'].tobytes() == want['value'].tobytes(), (ranks, m is not None)
            check_report(ctx, S, nc, E, ranks)


@pytest.mark.parametrize('S', ROWS)
def test_exact_over_rows(device_ctx, S):
    check_exact(device_ctx, S, 17, 40, seed=S)


@pytest.mark.parametrize('nc', WIDTHS)
def test_exact_over_widths(device_ctx, nc):
    check_exact(device_ctx, 33, nc, 24, seed=nc)


@pytest.mark.parametrize('E', DRAWS)
def test_exact_over_draws(device_ctx, E):
    check_exact(device_ctx, 33, 5, E, seed=E)


def test_one_row_and_three_ranks_runs_out_after_the_first(device_ctx):
    X, betas, _ = integer_case(0, 1, 4, 9)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(1))
    got = device_ctx.drawbest_rows(slots, betas, None, 3)
    assert np.array_equal(got['index'], [[0] * 9, [-1] * 9, [-1] * 9])
    assert np.array_equal(got['value'][0], (X @ betas.T)[0]) and np.all(got['value'][1:] == -np.inf)


def test_same_bytes_whatever_the_grid(device_ctx):
    X, betas, _ = continuous_case(1)                             # 1029 rows = 65 tiles
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(X.shape[0]))
    own = device_ctx.drawbest_rows(slots, betas, None, 4)
    chunks = check_report(device_ctx, 1029, 17, 200, 4)['row_chunks']
    assert chunks > 3
    for cap in (1, 3):
        got = device_ctx.drawbest_rows(slots, betas, None, 4, grid_cap=cap)
        rep = check_report(device_ctx, 1029, 17, 200, 4)
        assert rep['row_chunks'] == cap and rep['tiles_per_chunk'] == -(-65 // cap)
        assert np.array_equal(got['index'], own['index']) and got['value'].tobytes() == own['value'].tobytes()
    again = device_ctx.drawbest_rows(slots, betas, None, 4)
    assert np.array_equal(again['index'], own['index']) and again['value'].tobytes() == own['value'].tobytes()


@pytest.mark.parametrize('S, nc, E', ((1029, 17, 200), (200, 301, 130)), ids=('registers', 'table'))
def test_continuous_data_within_the_rounding_of_two_dot_products(device_ctx, S, nc, E):
    X, betas, _ = continuous_case(2, S, nc, E)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(S))
    mask = np.zeros(S, dtype=np.uint8)
    mask[::7] = 1
    ranks = 5
    got = device_ctx.drawbest_rows(slots, betas, mask, ranks)
    want = po.ranks_host(X, betas, ranks, mask)
    F, tol, cols = X @ betas.T, tolerance(X, betas), np.arange(E)
    worst_value = worst_short = 0.0
    for r in range(ranks):
        rows = got['index'][r]
        assert np.all(rows >= 0) and not np.any(mask[rows])
        at = F[rows, cols]
        worst_value = max(worst_value, float(np.max(np.abs(got['value'][r] - at) / tol)))
        worst_short = max(worst_short, float(np.max((want['value'][r] - at) / tol)))
        assert np.all(np.abs(got['value'][r] - at) <= tol), r
        assert np.all(at >= want['value'][r] - tol), r
    print(f"S {S} nc {nc} E {E}: worst |value - f| / tol {worst_value:.3g}, worst shortfall / tol {worst_short:.3g}, rows that "
          f"differ from numpy's {int(np.sum(got['index'] != want['index']))} of {ranks * E}")
    for d in range(E):
        assert len(set(got['index'][:, d].tolist())) == ranks, d


def test_nan_never_ranks_and_infinities_compare_as_numbers(device_ctx):
    X, betas = inf_case()
    S = X.shape[0]
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(S))
    for ranks in (1, S):
        want = po.ranks_host(X, betas, ranks)
        got = device_ctx.drawbest_rows(slots, betas, None, ranks)
        assert np.array_equal(got['index'], want['index']) and got['value'].tobytes() == want['value'].tobytes()
    assert np.all(got['index'][S - 3:, 0] == -1) and got['index'][:3, 1].tolist() == [1, 8, 20]
    assert got['index'][S - 3:, 2].tolist() == [1, 8, 20] and np.all(got['value'][S - 3:, 2] == -np.inf)


def test_refusals_launch_nothing_and_leave_the_context_usable(device_ctx, monkeypatch):
    S = 40
    ones, _ = stage(device_ctx, np.zeros((S, 0)), np.zeros(S))
    device_ctx.timing_enable(True)
    device_ctx.timing_reset()
    try:
        with pytest.raises(_capi.FoklNativeError, match=f'{LIMIT + 1} columns want .* bytes of LDS.*at most {LIMIT} columns'):
            device_ctx.drawbest_rows(np.zeros(LIMIT + 1, dtype=np.int32), np.zeros((2, LIMIT + 1)))
        assert device_ctx.timing_get(_capi.K_DRAWBEST)['launches'] == 0
        rep = device_ctx.drawbest_report()
        assert rep['instance'] == 'none' and rep['launches'] == 0 and rep['ranks'] == 0 and rep['lds_bytes'] == 0
        for ranks in (0, _capi.DRAWBEST_MAX_RANKS + 1):
            with pytest.raises(_capi.FoklNativeError, match=f'ranks must be in 1..64, not {ranks}'):
                device_ctx.drawbest_rows(ones, np.ones((3, 1)), None, ranks)
        with pytest.raises(_capi.FoklNativeError, match='every coefficient must be finite'):
            device_ctx.drawbest_rows(ones, np.array([[1.0], [np.inf], [1.0]]))
        monkeypatch.setenv('FOKL_ACQUIRE_FREE_BYTES', str(64 << 20))
        with pytest.raises(_capi.FoklNativeError, match='64 MiB to spare.*FOKL_ACQUIRE_FREE_BYTES caps what counts'):
            device_ctx.drawbest_rows(ones, np.ones((3, 1)))
        monkeypatch.delenv('FOKL_ACQUIRE_FREE_BYTES')
        assert device_ctx.timing_get(_capi.K_DRAWBEST)['launches'] == 0
        assert device_ctx.drawbest_report()['instance'] == 'none'
        got = device_ctx.drawbest_rows(ones, np.array([[1.0], [-2.0], [0.0]]), None, 2)      # every row ties: the lowest index
        assert got['index'].tolist() == [[0, 0, 0], [1, 1, 1]] and got['value'].tolist() == [[1.0, -2.0, 0.0]] * 2
        t = device_ctx.timing_get(_capi.K_DRAWBEST)
        assert t['launches'] == 1 and t['flops'] > 0 and t['bytes'] > 0
        rep = device_ctx.drawbest_report()
        assert rep['launches'] == 4 and rep['pass_us'] > 0 and 0 <= rep['merge_us'] <= rep['kernel_us']
    finally:
        device_ctx.timing_enable(False)
    with pytest.raises(ValueError, match='one mask entry per uploaded row'):
        device_ctx.drawbest_rows(ones, np.ones((3, 1)), np.zeros(S + 1))

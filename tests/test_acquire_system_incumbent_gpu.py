"""fokl_acquire_system_incumbent (csrc/fokl_acquire_system_device.inc) called directly, against its statement
``acquire.incumbent_system_host``: per draw the best objective over the uploaded rows that are feasible in that draw, and
their number.  Integer data (every product and comparison exact): equal.  Continuous data: the same bytes whatever the grid.
"""
import numpy as np
import pytest

from test_acquire_host import continuous_case
from test_acquire_system_host import LIMITS, constraint_case
from test_acquire_system_select_gpu import integer_system, stage_models
from fokl_gpy_amd import _capi
from fokl_gpy_amd import acquire as aq

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 1029)


def check_exact(ctx, S, widths, E, grid_cap=0, seed=0, case=None):
    Xs, betas, _, lo, hi = case if case is not None else integer_system(seed, S, widths, E)
    slots = stage_models(ctx, Xs)
    best, count = ctx.acquire_system_incumbent(slots, betas, lo, hi, grid_cap)
    want_best, want_count = aq.incumbent_system_host(Xs, betas, lo, hi)
    assert count.dtype == np.int64 and np.array_equal(count, want_count), (S, widths, E, grid_cap)
    assert np.array_equal(best, want_best, equal_nan=True), (S, widths, E, grid_cap)
    assert np.array_equal(best == -np.inf, count == 0)
    rep = ctx.acquire_system_report()
    tiles = -(-S // 16)
    assert rep['instance'] == 'incumbent' and rep['constraints'] == len(widths) - 1 and rep['row_tiles'] == tiles
    assert 1 <= rep['grid'] <= tiles and rep['lds_bytes'] == 8 * 16 * sum(-(-w // 4) * 4 for w in widths)
    assert rep['launches'] == 2 and rep['kernel_us'] > 0 and rep['bound_grid'] == -(-E // 256)
    return rep, best, count


@pytest.mark.parametrize('S', ROWS)
def test_exact_over_every_tile_edge(device_ctx, S):
    check_exact(device_ctx, S, (17, 5), 40, seed=1)


def test_exact_on_both_sides_of_the_draw_group(device_ctx):
    """The group size comes from the report of a first call: one draw, one less than a group, a group, one more, and many
    groups with a partly used last one."""
    group = check_exact(device_ctx, 33, (5, 3), 7, seed=2)[0]['draw_group']
    assert group >= 16 and group % 16 == 0
    for E in (1, 15, 16, 17, group - 1, group, group + 1, 2 * group - 1, 2 * group + 1, 1000):
        check_exact(device_ctx, 33, (5, 3), E, seed=3)


@pytest.mark.parametrize('widths', ((1, 1), (3, 5), (5, 3, 1), (17, 9, 5, 4, 3, 2, 1, 1), (1276, 4)))
def test_exact_over_width_sets(device_ctx, widths):
    check_exact(device_ctx, 33, widths, 40, seed=4)


def test_a_draw_with_no_feasible_row_is_minus_infinity_and_zero(device_ctx):
    """A constant-only constraint model whose draws 64 .. 127 and the last one violate the limit."""
    S, E = 50, 200
    Xs, betas, b0, lo, hi = integer_system(5, S, (5, 1, 3), E)
    betas[1][:] = 0.0
    betas[1][64:128] = 5.0
    betas[1][E - 1] = -5.0
    _, best, count = check_exact(device_ctx, S, (5, 1, 3), E, case=(Xs, betas, b0, lo, hi))
    empty = np.zeros(E, dtype=bool)
    empty[64:128] = empty[E - 1] = True
    assert np.all(best[empty] == -np.inf) and np.all(count[empty] == 0)
    assert np.all(np.isfinite(best[~empty])) and np.all(count[~empty] > 0) and count.max() <= S


def test_a_feasible_row_that_is_not_finite_makes_its_draws_nan(device_ctx):
    S, E = 40, 24
    Xs, betas, b0, lo, hi = integer_system(6, S, (9, 3), E)
    ok = aq.feasible_rows([Xs[1] @ betas[1].T], lo, hi)
    assert ok[20].any() and not ok[20].all()
    slots = stage_models(device_ctx, Xs)
    col = Xs[0][:, 5].copy()
    col[20] = np.nan
    device_ctx.write_slot(int(slots[0][5]), col)
    Xs[0][:, 5] = col
    best, count = device_ctx.acquire_system_incumbent(slots, betas, lo, hi)
    want_best, want_count = aq.incumbent_system_host(Xs, betas, lo, hi)
    assert np.array_equal(np.isnan(best), ok[20]) and np.array_equal(best, want_best, equal_nan=True)
    assert np.array_equal(count, want_count)


def test_same_bytes_whatever_the_grid(device_ctx):
    X, betas, _ = continuous_case(1)
    Xc, betas_c = constraint_case(1)
    slots = stage_models(device_ctx, [X, Xc])
    runs = {}
    for cap in (0, 1, 3):
        runs[cap] = device_ctx.acquire_system_incumbent(slots, [betas, betas_c], LIMITS[:1], LIMITS[1:], cap)
        rep = device_ctx.acquire_system_report()
        assert rep['grid'] == (cap if cap else rep['grid']) and rep['row_tiles'] == 65
    want_best, want_count = aq.incumbent_system_host([X, Xc], [betas, betas_c], LIMITS[:1], LIMITS[1:])
    assert np.array_equal(runs[0][1], want_count) and np.allclose(runs[0][0], want_best, rtol=1e-12, atol=1e-12)
    for cap in (1, 3):
        assert runs[cap][0].tobytes() == runs[0][0].tobytes() and runs[cap][1].tobytes() == runs[0][1].tobytes()
    check_exact(device_ctx, 1029, (17, 5), 40, grid_cap=3, seed=7)
    check_exact(device_ctx, 1029, (17, 5), 40, grid_cap=1, seed=7)


def test_refusals_leave_the_context_usable(device_ctx):
    Xs, betas, b0, lo, hi = integer_system(8, 20, (3, 2), 8)
    slots = stage_models(device_ctx, Xs)
    with pytest.raises(_capi.FoklNativeError, match='the limits of constraint model 1 hold a NaN'):
        device_ctx.acquire_system_incumbent(slots, betas, [np.nan], hi)
    assert device_ctx.acquire_system_report()['instance'] == 'none'
    with pytest.raises(_capi.FoklNativeError, match='every coefficient must be finite'):
        device_ctx.acquire_system_incumbent(slots, [betas[0], np.full_like(betas[1], np.inf)], lo, hi)
    with pytest.raises(_capi.FoklNativeError, match='0 constraint models: it takes 1 to 7'):
        device_ctx.acquire_system_incumbent(slots[:1], betas[:1], [], [])
    best, count = device_ctx.acquire_system_incumbent(slots, betas, lo, hi)
    want = aq.incumbent_system_host(Xs, betas, lo, hi)
    assert np.array_equal(best, want[0]) and np.array_equal(count, want[1])

"""fokl_acquire_system_select (csrc/fokl_acquire_system_device.inc) called directly, against its statement
``acquire.select_system_host``.

As in test_acquire_select_gpu.py there are two kinds of data.  Exact: every model's columns are [1 | -3..3], its betas in
-2..2, b0 in -4..4 and the limits integers (test_acquire_host.integer_case per model), so every product, comparison and sum
is exact: ``np.array_equal`` on ALL fields -- picks, gains, incumbent_after, the feasible-draw counts, the traced g, the tiles
evaluated per pick and the traced evaluated-tile bytes.  Continuous (continuous_case with the constraint model of the host
file): where bits must agree between two DEVICE calls.  The models' raw columns are staged side by side with
test_score_gpu.stage; model k's slots are [SLOT_ONES, its own columns].
"""
import math

import numpy as np
import pytest

from test_acquire_host import continuous_case, integer_case
from test_acquire_select_gpu import DT, launches_of, same
from test_acquire_system_host import LIMITS, constraint_case
from test_score_gpu import stage
from fokl_gpy_amd import _capi
from fokl_gpy_amd import acquire as aq

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 1029)
WIDTHS = ((1, 1), (3, 5), (4, 4), (5, 3, 1), (17, 129), (17, 9, 5, 4, 3, 2, 1, 1), (1276, 4))
DRAWS = (1, 15, 16, 17, 16 * DT - 1, 16 * DT, 16 * DT + 1, 1000)
FIELDS = ('index', 'gain', 'incumbent_after', 'tiles_evaluated', 'feasible', 'trace_g', 'trace_eval')


def stage_models(ctx, Xs):
    """The models' columns (ones first in each) side by side in one dataset -> one slot list per model."""
    S = Xs[0].shape[0]
    stage(ctx, np.concatenate([X[:, 1:] for X in Xs], axis=1), np.zeros(S))
    slots, at = [], _capi.SLOT_FIRST_FREE
    for X in Xs:
        slots.append(np.concatenate([[_capi.SLOT_ONES], np.arange(at, at + X.shape[1] - 1)]).astype(np.int32))
        at += X.shape[1] - 1
    return slots


def integer_system(seed, S, widths, E):
    """(Xs, betas, b0, lo, hi): integer_case per model; for constraint k = 0, 1, .. lo_k = -(2 + 2 k) - floor(sqrt(width_k)),
    hi_k = 1 - lo_k, and for a constant-only FIRST constraint limits that cut its draws (-1, 1)."""
    Xs, betas, b0 = [], [], None
    for k, w in enumerate(widths):
        X, B, b = integer_case(seed + 1000 * k, S, w, E)
        Xs.append(X)
        betas.append(B)
        b0 = b if k == 0 else b0
    lo = np.array([-(2.0 + 2.0 * k) - math.floor(math.sqrt(w)) for k, w in enumerate(widths[1:])])      # k counts constraints from 0
    hi = 1.0 - lo
    if widths[1] == 1:
        lo[0], hi[0] = -1.0, 1.0
    return Xs, betas, b0, lo, hi


def share_of(Xs, betas, lo, hi):
    return float(aq.feasible_rows([X @ B.T for X, B in zip(Xs[1:], betas[1:])], lo, hi).mean())


def check_report(ctx, criterion, lazy, S, widths, picks, res):
    rep = ctx.acquire_system_report()
    padded = sum(-(-w // 4) * 4 for w in widths)
    tiles = -(-S // 16)
    assert rep['instance'] == criterion and rep['lazy'] == lazy and rep['constraints'] == len(widths) - 1
    assert rep['row_tiles'] == tiles and 1 <= rep['grid'] <= tiles and rep['lds_bytes'] == 8 * 16 * padded
    assert rep['draw_group'] == 16 * DT and rep['picks'] == picks
    assert rep['launches'] == launches_of(picks, lazy) and rep['kernel_us'] > 0
    assert rep['tiles_evaluated'] == int(res['tiles_evaluated'].sum())
    assert rep['tiles_evaluated_max_lazy'] == (int(res['tiles_evaluated'][1:].max()) if lazy and picks > 1 else 0)
    return rep


def check_exact(ctx, S, widths, E, grid_cap=0, seed=0, picks=None, case=None, share=(0.2, 0.8)):
    """Both criteria, lazy and not, the last pick traced, against select_system_host: every field, equal."""
    Xs, betas, b0, lo, hi = case if case is not None else integer_system(seed, S, widths, E)
    if share is not None:
        got = share_of(Xs, betas, lo, hi)
        assert share[0] <= got <= share[1], (got, widths)
    slots = stage_models(ctx, Xs)
    picks = min(S, 6) if picks is None else picks
    rep = None
    for criterion in aq.CRITERIA:
        for lazy in (False, True):
            where = (S, widths, E, criterion, lazy, grid_cap)
            res = ctx.acquire_system_select(slots, betas, b0, lo, hi, picks=picks, criterion=criterion, lazy=lazy,
                                            grid_cap=grid_cap, trace_pick=picks - 1)
            rep = check_report(ctx, criterion, lazy, S, widths, picks, res)
            host = aq.select_system_host(Xs, betas, b0, lo, hi, picks=picks, criterion=criterion, lazy=lazy, trace_pick=picks - 1)
            if not lazy:
                host['trace_eval'] = None
            for name in FIELDS:
                assert same(res[name], host[name]), (name,) + where
            assert np.all(res['index'] >= 0) and len(set(res['index'].tolist())) == picks, where
    return rep


@pytest.mark.parametrize('S', ROWS)
def test_exact_over_every_tile_edge(device_ctx, S):
    check_exact(device_ctx, S, (17, 5), 40, seed=1, share=None if S == 1 else (0.2, 0.8))


@pytest.mark.parametrize('widths', WIDTHS)
def test_exact_over_every_width_set(device_ctx, widths):
    """Each model's padding to 4 falls differently; eight models; (1276, 4) is exactly 160 KiB of LDS."""
    rep = check_exact(device_ctx, 33, widths, 40, seed=2)
    if widths == (1276, 4):
        assert rep['lds_bytes'] == 160 * 1024


@pytest.mark.parametrize('E', DRAWS)
def test_exact_over_every_draw_count(device_ctx, E):
    check_exact(device_ctx, 33, (5, 3), E, seed=3, share=None if E == 1 else (0.2, 0.8))


def test_a_whole_block_of_draws_infeasible_for_every_row(device_ctx):
    """A constant-only constraint model whose draws 64 .. 127 violate the limit: the second 64-draw block of every row has
    no feasible draw, the others are cut by a second model."""
    S, E = 33, 200
    Xs, betas, b0, lo, hi = integer_system(4, S, (5, 1, 3), E)
    betas[1][:] = 0.0
    betas[1][64:128] = 5.0
    ok = aq.feasible_rows([X @ B.T for X, B in zip(Xs[1:], betas[1:])], lo, hi)
    assert not ok[:, 64:128].any() and ok[:, :64].any() and ok[:, 128:].any()
    check_exact(device_ctx, S, (5, 1, 3), E, case=(Xs, betas, b0, lo, hi))


def test_one_column_more_than_lds_holds_is_refused_with_nothing_launched(device_ctx, monkeypatch):
    S = 40
    ones, _ = stage(device_ctx, np.zeros((S, 0)), np.zeros(S))
    wide, five, four = np.zeros(1276, dtype=np.int32), np.zeros(5, dtype=np.int32), np.zeros(4, dtype=np.int32)
    lo, hi = [-1.0], [1.0]
    device_ctx.timing_enable(True)
    device_ctx.timing_reset()
    try:
        with pytest.raises(_capi.FoklNativeError, match='1281 columns over 2 models.*want 164352 bytes of LDS.*163840'):
            device_ctx.acquire_system_select([wide, five], [np.zeros((2, 1276)), np.zeros((2, 5))], np.zeros(2), lo, hi)
        assert device_ctx.timing_get(_capi.K_ACQUIRE_SYSTEM)['launches'] == 0
    finally:
        device_ctx.timing_enable(False)
    rep = device_ctx.acquire_system_report()
    assert rep['instance'] == 'none' and rep['launches'] == 0 and rep['picks'] == 0 and rep['lds_bytes'] == 0
    res = device_ctx.acquire_system_select([wide, four], [np.zeros((2, 1276)), np.zeros((2, 4))], np.zeros(2), lo, hi)
    assert res['index'].tolist() == [0] and device_ctx.acquire_system_report()['lds_bytes'] == 160 * 1024

    one, b = np.ones((3, 1)), np.zeros(3)
    call = lambda **kw: device_ctx.acquire_system_select(kw.pop('slots', [ones, ones]), kw.pop('betas', [one, one]),
                                                         kw.pop('b', b), kw.pop('lo', lo), kw.pop('hi', hi), **kw)
    with pytest.raises(_capi.FoklNativeError, match='41 picks from a pool of 40 rows'):
        call(picks=41)
    with pytest.raises(_capi.FoklNativeError, match='picks must be at least 1'):
        call(picks=0)
    with pytest.raises(_capi.FoklNativeError, match='every coefficient must be finite'):
        call(betas=[one, one * np.array([[1.0], [np.nan], [1.0]])])
    for bad in (np.nan, np.inf):
        with pytest.raises(_capi.FoklNativeError, match=r'every incumbent must be finite or -inf \(draw 1 is not\)'):
            call(b=np.array([0.0, bad, 0.0]))
    with pytest.raises(_capi.FoklNativeError, match='the limits of constraint model 1 hold a NaN'):
        call(lo=[np.nan])
    with pytest.raises(_capi.FoklNativeError, match='0 constraint models: it takes 1 to 7'):
        device_ctx.acquire_system_select([ones], [one], b, [], [])
    with pytest.raises(_capi.FoklNativeError, match='8 constraint models: it takes 1 to 7'):
        device_ctx.acquire_system_select([ones] * 9, [one] * 9, b, [0.0] * 8, [1.0] * 8)
    with pytest.raises(_capi.FoklNativeError, match='model 1 has 0 columns'):
        call(slots=[ones, np.zeros(0, dtype=np.int32)], betas=[one, np.zeros((3, 0))])
    with pytest.raises(_capi.FoklNativeError, match='trace_pick must be -1'):
        call(picks=2, trace_pick=2)
    monkeypatch.setenv('FOKL_ACQUIRE_FREE_BYTES', str(64 << 20))
    with pytest.raises(_capi.FoklNativeError, match='64 MiB to spare.*FOKL_ACQUIRE_FREE_BYTES caps what counts'):
        call()
    monkeypatch.delenv('FOKL_ACQUIRE_FREE_BYTES')
    assert device_ctx.acquire_system_report()['instance'] == 'none'
    res = call(b=np.array([0.0, 0.5, 2.0]), betas=[one, np.array([[0.0], [0.0], [3.0]])], criterion='pi')    # usable afterwards
    assert res['index'].tolist() == [0] and res['gain'][0] == 2.0 / 3.0 and res['feasible'].tolist() == [2]
    res = call(b=np.array([0.0, 0.5, 0.9]), betas=[one, np.array([[0.0], [0.0], [3.0]])], criterion='pi')
    assert res['gain'][0] == 2.0 / 3.0                           # the third draw is above its incumbent, and infeasible


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_same_bytes_whatever_the_grid(device_ctx, criterion):
    X, betas, b0 = continuous_case(1)
    Xc, betas_c = constraint_case(1)
    slots = stage_models(device_ctx, [X, Xc])
    for lazy in (False, True):
        runs = {}
        for cap in (0, 1, 3):
            runs[cap] = device_ctx.acquire_system_select(slots, [betas, betas_c], b0, LIMITS[:1], LIMITS[1:], picks=8,
                                                         criterion=criterion, lazy=lazy, grid_cap=cap, trace_pick=7)
            rep = device_ctx.acquire_system_report()
            assert rep['grid'] == (cap if cap else rep['grid']) and rep['bound_grid'] == (cap if cap else -(-1029 // 256))
            assert rep['row_tiles'] == 65 and (cap == 0 or rep['row_tiles'] > rep['grid'])
        assert runs[0]['gain'][0] > 0.0 and 0 < runs[0]['feasible'][0] < 200
        for cap in (1, 3):
            for name in FIELDS:
                assert (runs[0][name] is None and runs[cap][name] is None) or \
                    runs[0][name].tobytes() == runs[cap][name].tobytes(), (name, cap, lazy)
    check_exact(device_ctx, 1029, (17, 5), 40, grid_cap=3, seed=4)
    check_exact(device_ctx, 1029, (17, 5), 40, grid_cap=1, seed=4)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('lazy', (False, True))
def test_infinite_limits_return_the_bytes_of_the_existing_entry_point(device_ctx, criterion, lazy):
    X, betas, b0 = continuous_case(2)
    Xc, betas_c = constraint_case(2)
    slots = stage_models(device_ctx, [X, Xc])
    free = device_ctx.acquire_select(slots[0], betas, b0, picks=8, criterion=criterion, lazy=lazy, trace_pick=7)
    res = device_ctx.acquire_system_select(slots, [betas, betas_c], b0, [-np.inf], [np.inf], picks=8, criterion=criterion,
                                           lazy=lazy, trace_pick=7)
    assert free['gain'][0] > 0.0 and np.all(res['feasible'] == 200)
    for name in ('index', 'gain', 'incumbent_after', 'tiles_evaluated', 'trace_g', 'trace_eval'):
        assert (free[name] is None and res[name] is None) or res[name].tobytes() == free[name].tobytes(), name


def test_a_picked_row_gains_exactly_zero_ever_after(device_ctx):
    """'ei' on continuous data: b rises to f* in the picked row's feasible draws, its infeasible draws never count, so the
    traced g at pick k is 0.0 at every earlier pick's row."""
    X, betas, b0 = continuous_case(0)
    Xc, betas_c = constraint_case(0)
    slots = stage_models(device_ctx, [X, Xc])
    picks = 5
    first = None
    for k in range(1, picks):
        res = device_ctx.acquire_system_select(slots, [betas, betas_c], b0, LIMITS[:1], LIMITS[1:], picks=picks, criterion='ei',
                                               lazy=False, trace_pick=k)
        first = res if first is None else first
        assert res['index'].tobytes() == first['index'].tobytes() and np.all(res['gain'][:k + 1] > 0.0)
        assert np.array_equal(res['trace_g'][res['index'][:k]], np.zeros(k)), k
        assert res['trace_g'][res['index'][k]] == res['gain'][k] == res['trace_g'].max()


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('grid_cap', (0, 1))
def test_heavy_ties_go_to_the_lowest_index_across_workgroups(device_ctx, criterion, grid_cap):
    """The heavy-tie case of test_acquire_select_gpu.py under a constant-only constraint model that is feasible in the even
    draws only: nine distinct rows among 1 029, every value an exact integer over E."""
    S, E = 1029, 32
    rng = np.random.default_rng(4)
    cols = rng.integers(-1, 2, size=(S, 2)).astype(np.float64)
    cols[:5] = 0.0
    betas = np.concatenate([np.zeros((E, 1)), rng.integers(1, 4, size=(E, 2))], axis=1).astype(np.float64)
    betas_c = np.where(np.arange(E) % 2 == 0, 0.0, 5.0)[:, None]
    X, Xc = np.concatenate([np.ones((S, 1)), cols], axis=1), np.ones((S, 1))
    b0 = np.zeros(E)
    slots = stage_models(device_ctx, [X, Xc])
    ok = np.broadcast_to(np.arange(E) % 2 == 0, (S, E))
    g0 = aq.gain_rows_system(X @ betas.T, ok, b0, criterion)
    top = np.flatnonzero(g0 == g0.max())
    assert top.size >= 64 and len(set(top // 256)) > 1 and len(set(top // 16)) > 8 and top[0] >= 5
    for lazy in (False, True):
        res = device_ctx.acquire_system_select(slots, [betas, betas_c], b0, [-1.0], [1.0], picks=4, criterion=criterion,
                                               lazy=lazy, grid_cap=grid_cap)
        host = aq.select_system_host([X, Xc], [betas, betas_c], b0, [-1.0], [1.0], picks=4, criterion=criterion, lazy=lazy)
        assert res['index'][0] == top[0] and res['gain'][0] == g0.max() and np.all(res['feasible'] == E // 2)
        for name in ('index', 'gain', 'incumbent_after', 'tiles_evaluated', 'feasible'):
            assert np.array_equal(res[name], host[name]), (name, lazy)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('lazy', (False, True))
def test_nan_rows_and_the_pool_taken_to_its_last_open_row(device_ctx, criterion, lazy):
    """Row 3 holds a NaN in a constraint column: infeasible everywhere, its gain is the number 0.0 and it can be picked.
    Rows 3 and 20 hold a NaN in an objective column: row 20 has feasible draws, so its gain is NaN and it never wins; with
    picks = S the last pick finds no row: index -1, gain -inf, 0 feasible draws."""
    S, E = 40, 24
    Xs, betas, b0, lo, hi = integer_system(7, S, (9, 3), E)
    assert aq.feasible_rows([Xs[1] @ betas[1].T], lo, hi)[20].any()
    slots = stage_models(device_ctx, Xs)
    for column, rows, model in ((1, [3], 1), (5, [3, 20], 0)):
        col = Xs[model][:, column].copy()
        col[rows] = np.nan
        device_ctx.write_slot(int(slots[model][column]), col)
        Xs[model][:, column] = col
    for k in (0, S - 1):
        res = device_ctx.acquire_system_select(slots, betas, b0, lo, hi, picks=S, criterion=criterion, lazy=lazy, trace_pick=k)
        host = aq.select_system_host(Xs, betas, b0, lo, hi, picks=S, criterion=criterion, lazy=lazy, trace_pick=k)
        assert sorted(res['index'][:39].tolist()) == sorted(set(range(S)) - {20})
        assert res['index'][39] == -1 and res['gain'][39] == -np.inf and res['feasible'][39] == 0
        assert np.array_equal(np.flatnonzero(np.isnan(res['trace_g'])), [20]) and res['trace_g'][3] == 0.0
        for name in ('index', 'gain', 'incumbent_after', 'tiles_evaluated', 'feasible', 'trace_g'):
            assert same(res[name], host[name]), (name, k)
        assert device_ctx.acquire_system_report()['launches'] == launches_of(S, lazy)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_lazy_accounting(device_ctx, criterion):
    """Integer data: the evaluated tiles of every pick are the statement's set.  Continuous data: index, gain and incumbent
    bytes of the full call, and some later pick evaluates fewer tiles than the pool has."""
    S, E, picks = 1029, 48, 5
    Xs, betas, b0, lo, hi = integer_system(5, S, (9, 5), E)
    slots = stage_models(device_ctx, Xs)
    for k in range(picks):
        res = device_ctx.acquire_system_select(slots, betas, b0, lo, hi, picks=picks, criterion=criterion, lazy=True, trace_pick=k)
        host = aq.select_system_host(Xs, betas, b0, lo, hi, picks=picks, criterion=criterion, lazy=True, trace_pick=k)
        assert np.array_equal(res['trace_eval'], host['trace_eval']), k
        assert np.array_equal(res['tiles_evaluated'], host['tiles_evaluated'])
        assert int(res['trace_eval'].sum()) == res['tiles_evaluated'][k]
    fewest = 65
    for seed in range(3):
        X, B, b = continuous_case(seed)
        Xc, Bc = constraint_case(seed)
        slots = stage_models(device_ctx, [X, Xc])
        full = device_ctx.acquire_system_select(slots, [B, Bc], b, LIMITS[:1], LIMITS[1:], picks=10, criterion=criterion, lazy=False)
        lazy = device_ctx.acquire_system_select(slots, [B, Bc], b, LIMITS[:1], LIMITS[1:], picks=10, criterion=criterion, lazy=True)
        rep = device_ctx.acquire_system_report()
        for name in ('index', 'gain', 'incumbent_after', 'feasible'):
            assert lazy[name].tobytes() == full[name].tobytes(), (name, seed)
        assert lazy['tiles_evaluated'][0] == 65 and np.all(full['tiles_evaluated'] == 65)
        assert rep['tiles_evaluated'] == int(lazy['tiles_evaluated'].sum()) and rep['launches'] == launches_of(10, True)
        fewest = min(fewest, int(lazy['tiles_evaluated'][1:].min()))
    print(f"{criterion}: the cheapest later pick evaluated {fewest} of 65 tiles")
    assert fewest < 65


def test_one_timed_region_of_its_own_slot(device_ctx):
    X, betas, b0 = continuous_case(2)
    Xc, betas_c = constraint_case(2)
    slots = stage_models(device_ctx, [X, Xc])
    device_ctx.timing_enable(True)
    device_ctx.timing_reset()
    try:
        device_ctx.acquire_system_select(slots, [betas, betas_c], b0, LIMITS[:1], LIMITS[1:], picks=5, lazy=True)
        t, other = device_ctx.timing_get(_capi.K_ACQUIRE_SYSTEM), device_ctx.timing_get(_capi.K_ACQUIRE)
        rep = device_ctx.acquire_system_report()
    finally:
        device_ctx.timing_enable(False)
    assert t['launches'] == 1 and other['launches'] == 0 and rep['launches'] == launches_of(5, True)
    assert rep['pass_us'] > 0 and rep['bound_us'] > 0 and rep['pivot_us'] > 0
    assert rep['kernel_us'] >= max(rep['pass_us'], rep['bound_us'], rep['pivot_us'])

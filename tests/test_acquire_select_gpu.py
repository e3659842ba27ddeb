"""fokl_acquire_select (csrc/fokl_acquire_device.inc) called directly, against its statement ``acquire.select_host``.

Two kinds of data:
  * exact -- columns, betas and b0 are small integers (test_acquire_host.integer_case), so every f, every difference and every
    sum is an exact integer in any order, b stays integer after every pick, and the one division by E is written alike on
    both sides: ``np.array_equal`` on ALL picks, gains, incumbent_after, the traced g, the tiles evaluated per pick and, under
    lazy, the traced evaluated-tile bytes.  A term dropped from a row's sum, a padding draw counted, a draw of the clamped
    last tile counted twice or a row's value landing in another lane changes an integer.
  * continuous (test_acquire_host.continuous_case) -- where bits must agree between two DEVICE calls: whatever the grid, lazy
    against full, and the picked rows' exact zeros.
Columns are staged with test_score_gpu.stage into the slots [SLOT_ONES, 2, 3, ...]: no model is needed, so every width up to
the LDS limit is reached.  ``DeviceContext.acquire_report`` says what ran.  Nothing depends on the number of CUs: where a
loop has to go round, ``grid_cap`` makes it.
"""
import numpy as np
import pytest

from test_acquire_host import continuous_case, integer_case
from test_score_gpu import stage
from fokl_gpy_amd import _capi
from fokl_gpy_amd import acquire as aq

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 1029)
WIDTHS = (1, 3, 4, 5, 17, 129, 512, 513, 1280)
DT = 4
DRAWS = (1, 15, 16, 17, 16 * DT - 1, 16 * DT, 16 * DT + 1, 1000)
FIELDS = ('index', 'gain', 'incumbent_after', 'tiles_evaluated', 'trace_g', 'trace_eval')
assert WIDTHS[-1] == _capi.ACQUIRE_MAX_COLUMNS


def launches_of(picks, lazy):
    """What the binding's docstring states: pass and pivot per pick, and under lazy bound and candidate pivot before them
    for every pick after the first."""
    return 2 + 4 * (picks - 1) if lazy else 2 * picks


def check_report(ctx, criterion, lazy, S, nc, picks, res):
    rep = ctx.acquire_report()
    ncp = -(-nc // 4) * 4
    tiles = -(-S // 16)
    assert rep['instance'] == criterion and rep['lazy'] == lazy and rep['row_tiles'] == tiles and 1 <= rep['grid'] <= tiles
    assert rep['lds_bytes'] == 8 * 16 * ncp and rep['dt'] == DT and rep['picks'] == picks
    assert rep['launches'] == launches_of(picks, lazy) and rep['kernel_us'] > 0
    assert rep['tiles_evaluated'] == int(res['tiles_evaluated'].sum())
    assert rep['tiles_evaluated_max_lazy'] == (int(res['tiles_evaluated'][1:].max()) if lazy and picks > 1 else 0)
    if not lazy:
        assert np.all(res['tiles_evaluated'] == tiles)
    return rep


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'))


def check_exact(ctx, S, nc, E, grid_cap=0, seed=0, picks=None):
    """Both criteria, lazy and not, the last pick traced, against select_host: every field, equal.  -> the last report."""
    X, betas, b0 = integer_case(seed, S, nc, E)
    slots, Xs = stage(ctx, X[:, 1:], np.zeros(S))
    assert np.array_equal(Xs, X)
    picks = min(S, 6) if picks is None else picks
    rep = None
    for criterion in aq.CRITERIA:
        for lazy in (False, True):
            where = (S, nc, E, criterion, lazy, grid_cap)
            res = ctx.acquire_select(slots, betas, b0, picks=picks, criterion=criterion, lazy=lazy, grid_cap=grid_cap,
                                     trace_pick=picks - 1)
            rep = check_report(ctx, criterion, lazy, S, nc, picks, res)
            host = aq.select_host(X, betas, b0, picks=picks, criterion=criterion, lazy=lazy, trace_pick=picks - 1)
            if not lazy:
                host['trace_eval'] = None
            for name in FIELDS:
                assert same(res[name], host[name]), (name,) + where
            assert np.all(res['index'] >= 0) and len(set(res['index'].tolist())) == picks, where
    return rep


@pytest.mark.parametrize('S', ROWS)
def test_exact_over_every_tile_edge(device_ctx, S):
    """1 row; 15 / 16 / 17 around one tile; 1 029 = 64 tiles and five rows of a 65th."""
    check_exact(device_ctx, S, 17, 40, seed=1)


@pytest.mark.parametrize('nc', WIDTHS)
def test_exact_over_every_width(device_ctx, nc):
    """1; 3 / 4 / 5 where the column padding to 4 parts; 17, 129; 512 (64 KiB of LDS, not raised) and 513 (the raised
    limit); 1 280, the widest tile 160 KiB of LDS hold.  33 rows: two tiles and one row of a third."""
    rep = check_exact(device_ctx, 33, nc, 24, seed=2)
    assert (rep['lds_bytes'] > 64 * 1024) == (nc > 512)


@pytest.mark.parametrize('E', DRAWS)
def test_exact_over_every_draw_count(device_ctx, E):
    """1, 15: padding draws inside the only 16-draw tile; 16, 17; 63, 64, 65: a block of DT tiles partly used, full, and one
    draw into the next block, whose tiles past dp are clamped, re-read and skipped; 1 000: sixteen blocks, the last with 40
    draws."""
    check_exact(device_ctx, 33, 5, E, seed=3)


def test_one_column_more_than_lds_holds_is_refused_with_nothing_launched(device_ctx, monkeypatch):
    S = 40
    slots, X = stage(device_ctx, np.zeros((S, 0)), np.zeros(S))
    wide = np.zeros(1281, dtype=np.int32)                            # 1 281 times the ones column
    device_ctx.timing_enable(True)
    device_ctx.timing_reset()
    try:
        with pytest.raises(_capi.FoklNativeError, match='1281 columns want 164352 bytes of LDS.*163840'):
            device_ctx.acquire_select(wide, np.zeros((2, 1281)), np.zeros(2), picks=1)
        assert device_ctx.timing_get(_capi.K_ACQUIRE)['launches'] == 0
    finally:
        device_ctx.timing_enable(False)
    rep = device_ctx.acquire_report()
    assert rep['instance'] == 'none' and rep['launches'] == 0 and rep['picks'] == 0
    one, b = np.ones((3, 1)), np.zeros(3)
    with pytest.raises(_capi.FoklNativeError, match='41 picks from a pool of 40 rows'):
        device_ctx.acquire_select(slots, one, b, picks=41)
    with pytest.raises(_capi.FoklNativeError, match='picks must be at least 1'):
        device_ctx.acquire_select(slots, one, b, picks=0)
    with pytest.raises(_capi.FoklNativeError, match='every coefficient must be finite'):
        device_ctx.acquire_select(slots, one * np.array([[1.0], [np.nan], [1.0]]), b, picks=1)
    for bad in (np.nan, np.inf):
        with pytest.raises(_capi.FoklNativeError, match=r'every incumbent must be finite or -inf \(draw 1 is not\)'):
            device_ctx.acquire_select(slots, one, np.array([0.0, bad, 0.0]), picks=1)
    with pytest.raises(_capi.FoklNativeError, match='trace_pick must be -1'):
        device_ctx.acquire_select(slots, one, b, picks=2, trace_pick=2)
    monkeypatch.setenv('FOKL_ACQUIRE_FREE_BYTES', str(64 << 20))
    with pytest.raises(_capi.FoklNativeError, match='64 MiB to spare.*FOKL_ACQUIRE_FREE_BYTES caps what counts'):
        device_ctx.acquire_select(slots, one, b, picks=1)
    monkeypatch.delenv('FOKL_ACQUIRE_FREE_BYTES')
    res = device_ctx.acquire_select(slots, one, np.array([0.0, 0.5, 2.0]), picks=1, criterion='pi')      # usable afterwards
    assert res['index'].tolist() == [0] and res['gain'][0] == 2.0 / 3.0


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_same_bytes_whatever_the_grid(device_ctx, criterion):
    """65 tiles over 1 and over 3 workgroups (22, 22, 21) against the device's own grid, on continuous data; exact too."""
    X, betas, b0 = continuous_case(1)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(X.shape[0]))
    for lazy in (False, True):
        runs = {}
        for cap in (0, 1, 3):
            runs[cap] = device_ctx.acquire_select(slots, betas, b0, picks=8, criterion=criterion, lazy=lazy, grid_cap=cap,
                                                  trace_pick=7)
            rep = device_ctx.acquire_report()
            assert rep['grid'] == (cap if cap else rep['grid']) and rep['bound_grid'] == (cap if cap else -(-1029 // 256))
            assert rep['row_tiles'] == 65 and (cap == 0 or rep['row_tiles'] > rep['grid'])
        assert runs[0]['gain'][0] > 0.0
        for cap in (1, 3):
            for name in FIELDS:
                assert (runs[0][name] is None and runs[cap][name] is None) or \
                    runs[0][name].tobytes() == runs[cap][name].tobytes(), (name, cap, lazy)
    check_exact(device_ctx, 1029, 17, 40, grid_cap=3, seed=4)
    check_exact(device_ctx, 1029, 17, 40, grid_cap=1, seed=4)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('grid_cap', (0, 1))
def test_heavy_ties_go_to_the_lowest_index_across_workgroups(device_ctx, criterion, grid_cap):
    """Two columns from {-1, 0, 1}: nine distinct rows among 1 029, so the maximum is attained by a hundred rows in every
    wavefront and workgroup, at every pick.  Every value is an exact integer over E, so the picks are the statement's."""
    S, E = 1029, 32
    rng = np.random.default_rng(4)
    cols = rng.integers(-1, 2, size=(S, 2)).astype(np.float64)
    cols[:5] = 0.0                                               # the first of the largest is not row 0
    betas = np.concatenate([np.zeros((E, 1)), rng.integers(1, 4, size=(E, 2))], axis=1).astype(np.float64)
    b0 = np.zeros(E)
    slots, X = stage(device_ctx, cols, np.zeros(S))
    g0 = aq.gain_rows(X @ betas.T, b0, criterion)
    top = np.flatnonzero(g0 == g0.max())
    assert top.size >= 64 and len(set(top // 256)) > 1 and len(set(top // 16)) > 8 and top[0] >= 5
    for lazy in (False, True):
        res = device_ctx.acquire_select(slots, betas, b0, picks=4, criterion=criterion, lazy=lazy, grid_cap=grid_cap)
        host = aq.select_host(X, betas, b0, picks=4, criterion=criterion, lazy=lazy)
        assert res['index'][0] == top[0] and res['gain'][0] == g0.max()
        for name in ('index', 'gain', 'incumbent_after', 'tiles_evaluated'):
            assert np.array_equal(res[name], host[name]), (name, lazy)
        # every later pick is again the lowest index of its own large tie
        b = b0
        for k in range(4):
            g = aq.gain_rows(X @ betas.T, b, criterion)
            g[res['index'][:k]] = -np.inf
            tie = np.flatnonzero(g == g.max())
            assert res['index'][k] == tie[0] and tie.size >= 32, k
            f = X[res['index'][k]] @ betas.T
            b = np.where(f > b, f if criterion == 'ei' else np.inf, b)


def test_a_picked_row_gains_exactly_zero_ever_after(device_ctx):
    """Continuous data, 'ei': b_d = max(b_d, f*_d) with f* from the product on the picked row's tile, so f - b <= 0 in every
    draw of every later pass, not 1e-17: the traced g at pick k is 0.0 at every earlier pick's row, for every k."""
    X, betas, b0 = continuous_case(0)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(X.shape[0]))
    picks = 6                                                    # the seventh gain of this case is 0.0
    first = None
    for k in range(1, picks):
        res = device_ctx.acquire_select(slots, betas, b0, picks=picks, criterion='ei', lazy=False, trace_pick=k)
        first = res if first is None else first
        assert res['index'].tobytes() == first['index'].tobytes() and np.all(res['gain'][:k + 1] > 0.0)
        assert np.array_equal(res['trace_g'][res['index'][:k]], np.zeros(k)), k
        assert res['trace_g'][res['index'][k]] == res['gain'][k] == res['trace_g'].max()
    lazy = device_ctx.acquire_select(slots, betas, b0, picks=picks, criterion='ei', lazy=True, trace_pick=picks - 1)
    fresh = lazy['trace_eval'][lazy['index'][:picks - 1] // 16].astype(bool)
    assert np.all(lazy['trace_g'][lazy['index'][:picks - 1][fresh]] == 0.0)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_lazy_accounting(device_ctx, criterion):
    """Integer data: the evaluated tiles of every pick are the statement's set.  Continuous data: index and gain bytes of the
    full call, and some later pick evaluates fewer tiles than the pool has."""
    S, nc, E, picks = 1029, 9, 48, 6
    X, betas, b0 = integer_case(5, S, nc, E)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(S))
    for k in range(picks):
        res = device_ctx.acquire_select(slots, betas, b0, picks=picks, criterion=criterion, lazy=True, trace_pick=k)
        host = aq.select_host(X, betas, b0, picks=picks, criterion=criterion, lazy=True, trace_pick=k)
        assert np.array_equal(res['trace_eval'], host['trace_eval']), k
        assert np.array_equal(res['tiles_evaluated'], host['tiles_evaluated'])
        assert int(res['trace_eval'].sum()) == res['tiles_evaluated'][k]
        assert device_ctx.acquire_report()['tiles_evaluated'] == int(host['tiles_evaluated'].sum())
    fewest = 65
    for seed in range(3):
        X, betas, b0 = continuous_case(seed)
        slots, _ = stage(device_ctx, X[:, 1:], np.zeros(X.shape[0]))
        full = device_ctx.acquire_select(slots, betas, b0, picks=12, criterion=criterion, lazy=False)
        lazy = device_ctx.acquire_select(slots, betas, b0, picks=12, criterion=criterion, lazy=True)
        rep = device_ctx.acquire_report()
        for name in ('index', 'gain', 'incumbent_after'):
            assert lazy[name].tobytes() == full[name].tobytes(), (name, seed)
        assert lazy['tiles_evaluated'][0] == 65 and np.all(full['tiles_evaluated'] == 65)
        assert rep['tiles_evaluated'] == int(lazy['tiles_evaluated'].sum()) and rep['launches'] == launches_of(12, True)
        fewest = min(fewest, int(lazy['tiles_evaluated'][1:].min()))
    print(f"{criterion}: the cheapest later pick evaluated {fewest} of 65 tiles")
    assert fewest < 65


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_the_pool_is_taken_to_its_last_row(device_ctx, criterion):
    check_exact(device_ctx, 17, 5, 24, seed=6, picks=17)
    X, betas, b0 = integer_case(6, 17, 5, 24)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(17))
    res = device_ctx.acquire_select(slots, betas, b0, picks=17, criterion=criterion)
    assert sorted(res['index'].tolist()) == list(range(17))
    with pytest.raises(_capi.FoklNativeError, match='18 picks from a pool of 17 rows'):
        device_ctx.acquire_select(slots, betas, b0, picks=18, criterion=criterion)


NAN_ROWS = (3, 20, 35)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('lazy', (False, True))
def test_nan_rows_never_win_and_the_empty_pick_is_minus_one(device_ctx, criterion, lazy):
    """Rows 3, 20 and 35 of 40 hold a NaN (3 and 20 share their tiles with finite rows); 40 picks are asked, 37 can be made.
    The NaN stays in its row's lane: the traced g is NaN there and nowhere else, and everything is the statement's."""
    S, nc, E = 40, 9, 24
    X, betas, b0 = integer_case(7, S, nc, E)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(S))
    col = X[:, 5].copy()
    col[list(NAN_ROWS)] = np.nan
    device_ctx.write_slot(int(slots[5]), col)
    X[:, 5] = col
    finite = sorted(set(range(S)) - set(NAN_ROWS))
    for k in (0, S - 1):
        res = device_ctx.acquire_select(slots, betas, b0, picks=S, criterion=criterion, lazy=lazy, trace_pick=k)
        host = aq.select_host(X, betas, b0, picks=S, criterion=criterion, lazy=lazy, trace_pick=k)
        assert sorted(res['index'][:37].tolist()) == finite
        assert np.all(res['index'][37:] == -1) and np.all(res['gain'][37:] == -np.inf)
        assert np.array_equal(np.flatnonzero(np.isnan(res['trace_g'])), NAN_ROWS)
        for name in ('index', 'gain', 'incumbent_after', 'tiles_evaluated', 'trace_g'):
            assert same(res[name], host[name]), (name, k)
        assert device_ctx.acquire_report()['launches'] == launches_of(S, lazy)


def test_one_timed_region_for_the_whole_queue(device_ctx):
    """All picks are queued behind one another: the call's launches are one entry of the kernel-time table, and the report's
    split by kernel is filled while timing is on."""
    X, betas, b0 = continuous_case(2)
    slots, _ = stage(device_ctx, X[:, 1:], np.zeros(X.shape[0]))
    device_ctx.timing_enable(True)
    device_ctx.timing_reset()
    try:
        device_ctx.acquire_select(slots, betas, b0, picks=5, criterion='ei', lazy=True)
        t = device_ctx.timing_get(_capi.K_ACQUIRE)
        rep = device_ctx.acquire_report()
    finally:
        device_ctx.timing_enable(False)
    assert t['launches'] == 1 and rep['launches'] == launches_of(5, True) == 18
    assert rep['pass_us'] > 0 and rep['bound_us'] > 0 and rep['pivot_us'] > 0
    assert rep['kernel_us'] >= max(rep['pass_us'], rep['bound_us'], rep['pivot_us'])
    device_ctx.acquire_select(slots, betas, b0, picks=5, criterion='ei', lazy=False)
    rep = device_ctx.acquire_report()
    assert rep['launches'] == 10 and rep['pass_us'] == rep['bound_us'] == rep['pivot_us'] == 0 and rep['kernel_us'] > 0

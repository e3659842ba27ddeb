"""fokl_design_select (csrc/fokl_design_device.inc) called directly, against its statement ``design.select_host``.

Two references for the three kernels:
  * exact -- columns, C0 and CMC0 are small integers (test_design_host.integer_case), so that v, w, u, a, v*, w*, p and q are
    exact integers whatever the order of a sum, and what follows them is the same sequence of correctly rounded operations
    on both sides (one division for the criterion, ``v - p * p / d`` and ``w - 2 p q / d + p p w* / (d d)`` left to right;
    the library is built without contraction).  ``np.array_equal`` on the first pick, the first downdate of every row and
    the second pick's index and gain: a term dropped from one row's sum, or moved to another row, changes an integer.  C is
    no longer integer after a pick, so the second v* is asked to the project's gate only.  This pins the lane map of the
    MFMA pass, the padding to 4 (k loop) and to 16 (matrix, LDS tile), the clamped block past ``jp`` of a partly used pass
    over the matrix, the LDS sizes above 64 KiB (more than 512 columns) and the width limit itself; with ties, the order
    across lanes, wavefronts, workgroups and partials; with NaN rows, that a row's NaN stays in its lane and never wins;
    and the pick that finds nothing (index -1, gain -inf, x* = 0).
  * rounded -- continuous, wide (129, 513, 768 columns) and well conditioned (cond(A0) <= 1e4 asserted, about 9), followed
    along the device's own picks against inv(A0 + X_D' X_D) formed from scratch, at test_design_gpu's GATE.
Columns are staged with test_score_gpu.stage into the slots [SLOT_ONES, 2, 3, ...]: no model is needed, so every width up
to FOKL_DESIGN_MAX_COLUMNS is reached.  ``DeviceContext.design_report`` says what ran.  Nothing depends on the number of
CUs: where a loop has to go round, ``grid_cap`` makes it.
"""
import numpy as np
import pytest

from test_design_gpu import GATE
from test_design_host import integer_case
from test_score_gpu import stage
from fokl_gpy_amd import _capi
from fokl_gpy_amd import design as dg

pytestmark = pytest.mark.gpu

WIDTHS = (1, 15, 16, 17, 63, 64, 65, 128, 129, 512, 513, 768)
ROWS = (1, 15, 16, 17, 1029)
assert WIDTHS[-1] == _capi.DESIGN_MAX_COLUMNS


def staged_integers(ctx, S, nc, seed=0):
    X, C0, CMC0 = (a.astype(np.float64) for a in integer_case(S, nc, seed))
    slots, Xs = stage(ctx, X[:, 1:], np.zeros(S))
    assert np.array_equal(Xs, X)
    return slots, X, C0, CMC0


def check_report(ctx, criterion, S, nc, picks, keep):
    rep = ctx.design_report()
    jp = -(-nc // 16) * 16
    assert rep['instance'] == criterion and rep['row_tiles'] == -(-S // 16) and 1 <= rep['grid'] <= rep['row_tiles']
    assert rep['lds_bytes'] == 8 * 16 * jp and rep['picks'] == picks and rep['refreshes'] == 0
    assert rep['launches'] == 1 + 2 * picks + (1 if keep else 0)
    return rep


def check_exact(ctx, S, nc, criterion, grid_cap=0, seed=0):
    """Two picks, and one pick with v (and w) kept, against select_host: bits, but for the second v*.  A pool of one row
    cannot give two picks without replicates (the call is refused): there, and only there, both sides run with replicates.
    -> the two device results."""
    slots, X, C0, CMC0 = staged_integers(ctx, S, nc, seed)
    if criterion == 'variance':
        CMC0 = None
    again = S == 1
    two = ctx.design_select(slots, C0, CMC0, picks=2, replicates=again, keep=False, grid_cap=grid_cap)
    rep = check_report(ctx, criterion, S, nc, 2, False)
    host = dg.select_host(X, C0, CMC0, picks=2, replicates=again)
    where = (S, nc, criterion, grid_cap)
    assert two['v'] is None and two['w'] is None
    assert np.array_equal(two['index'], host['index']) and np.all(two['index'] >= 0), where
    assert np.array_equal(two['gain'], host['gain']), where
    assert two['vstar'][0] == host['vstar'][0], where
    assert np.array_equal(two['x'], host['x']) and np.array_equal(two['x'], X[two['index']]), where
    assert abs(two['vstar'][1] - host['vstar'][1]) <= GATE * abs(host['vstar'][1]), where
    one = ctx.design_select(slots, C0, CMC0, picks=1, keep=True, grid_cap=grid_cap)
    check_report(ctx, criterion, S, nc, 1, True)
    host1 = dg.select_host(X, C0, CMC0, picks=1, keep=True)
    for name in ('index', 'gain', 'vstar', 'x', 'v'):
        assert np.array_equal(one[name], host1[name]), (name,) + where
    assert np.all(np.isfinite(one['v']))
    if criterion == 'ivr':
        assert np.array_equal(one['w'], host1['w']), where
    else:
        assert one['w'] is None
    return two, one, rep


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('nc', WIDTHS)
@pytest.mark.parametrize('S', (17, 1029))
def test_exact_over_every_width(device_ctx, S, nc, criterion):
    """1; 15 / 16 / 17 where the column padding to 4 and to 16 part; 63 / 64 / 65 and 128 / 129, a full pass of four 16-row
    blocks of the matrix and the step into the next, whose blocks past jp are clamped, re-read and skipped; 512 (64 KiB of
    LDS, not raised), 513 and 768 (66 and 96 KiB: the raised limit), 768 the kernels' width limit."""
    _, _, rep = check_exact(device_ctx, S, nc, criterion)
    assert (rep['lds_bytes'] > 64 * 1024) == (nc > 512)


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('nc', (17, 129))
@pytest.mark.parametrize('S', ROWS)
def test_exact_over_every_tile_edge(device_ctx, S, nc, criterion):
    check_exact(device_ctx, S, nc, criterion, seed=1)


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('nc', (65, 768))
def test_exact_when_the_tile_loop_and_the_step_loop_go_round_unevenly(device_ctx, nc, criterion):
    """65 tiles over 3 workgroups (22, 22, 21) and 1 029 rows over 3 x 256 lanes (two rounds, the second partly empty)."""
    S = 1029
    two, one, _ = check_exact(device_ctx, S, nc, criterion, seed=2)
    two3, one3, rep = check_exact(device_ctx, S, nc, criterion, grid_cap=3, seed=2)
    assert rep['grid'] == 3 and rep['step_grid'] == 3 and rep['row_tiles'] > rep['grid']
    for a, b in ((two, two3), (one, one3)):
        for name in ('index', 'gain', 'vstar', 'x', 'v', 'w'):
            assert (a[name] is None and b[name] is None) or a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('grid_cap', (0, 1))
def test_heavy_ties_go_to_the_lowest_index_across_workgroups(device_ctx, criterion, grid_cap):
    """Columns from {-1, 0, 1}, C0 = I, CMC0 = 2 I: v = 1 + a^2 + b^2 and w = 2 v take three values over 1 029 rows, so the
    maximum is attained by hundreds of rows in every wavefront and workgroup; after the first pick x* the rows that differ
    from x* in sign tie again (v = 3 - 1 / 4).  Every comparison is exact, so the device's picks are the statement's."""
    S = 1029
    cols = np.random.default_rng(4).integers(-1, 2, size=(S, 2)).astype(np.float64)
    cols[:5] = 0.0                                               # the first of the largest is not row 0
    slots, X = stage(device_ctx, cols, np.zeros(S))
    C0, CMC0 = np.eye(3), (2.0 * np.eye(3) if criterion == 'ivr' else None)
    v0 = 1.0 + cols[:, 0] ** 2 + cols[:, 1] ** 2
    crit0 = 2.0 * v0 / (1.0 + v0) if criterion == 'ivr' else v0
    top = np.flatnonzero(crit0 == crit0.max())
    assert top.size >= 8 and len(set(top // 256)) > 1 and len(set(top // 64)) > 1 and top[0] > 0
    host = dg.select_host(X, C0, CMC0, picks=1, keep=True)
    assert host['index'][0] == top[0]
    crit1 = host['w'] / (1.0 + host['v']) if criterion == 'ivr' else host['v'].copy()
    crit1[top[0]] = -np.inf
    top1 = np.flatnonzero(crit1 == crit1.max())
    assert top1.size >= 8 and len(set(top1 // 256)) > 1 and len(set(top1 // 64)) > 1
    res = device_ctx.design_select(slots, C0, CMC0, picks=2, keep=False, grid_cap=grid_cap)
    rep = device_ctx.design_report()
    assert rep['step_grid'] == (1 if grid_cap else -(-S // 256))
    assert res['index'].tolist() == [top[0], top1[0]]
    assert np.array_equal(res['gain'], [crit0.max(), crit1.max()])
    host2 = dg.select_host(X, C0, CMC0, picks=2)
    assert np.array_equal(res['index'], host2['index']) and np.array_equal(res['gain'], host2['gain'])
    assert np.array_equal(res['vstar'], host2['vstar'])          # 3 and 2.75: exact


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_replicates_mask_nothing(device_ctx, criterion):
    """An intercept alone: every row ties at every pick, so row 0 is taken twice with replicates -- which only an unmasked
    row can be -- and rows 0 and 1 without.  Then the 17-column integer case with replicates against the statement."""
    S = 1029
    for nc, seed in ((1, 3), (17, 3)):
        slots, X, C0, CMC0 = staged_integers(device_ctx, S, nc, seed)
        CMC0 = CMC0 if criterion == 'ivr' else None
        for replicates in (True, False):
            host = dg.select_host(X, C0, CMC0, picks=2, replicates=replicates)
            res = device_ctx.design_select(slots, C0, CMC0, picks=2, replicates=replicates)
            assert np.array_equal(res['index'], host['index']) and np.array_equal(res['gain'], host['gain']), (nc, replicates)
            assert res['vstar'][0] == host['vstar'][0] and np.array_equal(res['x'], host['x']), (nc, replicates)
            if nc == 1:
                assert res['index'].tolist() == ([0, 0] if replicates else [0, 1])


NAN_ROWS = (3, 20, 35)


def from_scratch(X, A0, M, picked, criterion):
    """(criterion, v) of every row of X after the picks ``picked`` from inv(A0 + X_D' X_D); picked rows -inf."""
    XD = X[np.asarray(picked, dtype=int)]
    C = np.linalg.inv(A0 + XD.T @ XD)
    v = np.einsum('sj,sj->s', X @ C, X)
    crit = np.einsum('sj,sj->s', X @ (C @ M @ C), X) / (1.0 + v) if criterion == 'ivr' else v.copy()
    crit[np.asarray(picked, dtype=int)] = -np.inf
    return crit, v


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('refresh_every', (0, 5))
def test_nan_rows_never_win_and_the_empty_pick_is_minus_one(device_ctx, criterion, refresh_every):
    """Rows 3, 20 and 35 of 40 hold a NaN (3 and 20 share their 16-row tiles with finite rows); 40 picks are asked, 37 can be
    made.  The NaN stays in its row's lane: the first pick is the statement's bit for bit.  The last three picks find
    nothing."""
    S, nc = 40, 17
    slots, X, C0, CMC0 = staged_integers(device_ctx, S, nc)
    if criterion == 'variance':
        CMC0 = None
    col = X[:, 5].copy()
    col[list(NAN_ROWS)] = np.nan
    device_ctx.write_slot(int(slots[5]), col)
    X[:, 5] = col
    res = device_ctx.design_select(slots, C0, CMC0, picks=S, refresh_every=refresh_every, keep=True)
    rep = device_ctx.design_report()
    assert rep['refreshes'] == ((S - 1) // refresh_every if refresh_every else 0)
    host = dg.select_host(X, C0, CMC0, picks=S, refresh_every=refresh_every, keep=True)
    finite = sorted(set(range(S)) - set(NAN_ROWS))
    made = len(finite)
    assert sorted(res['index'][:made].tolist()) == finite
    for name in ('index', 'gain', 'vstar', 'x'):
        assert np.array_equal(res[name][:1], host[name][:1]), name
        assert np.array_equal(res[name][made:], host[name][made:]), name
    assert np.all(res['index'][made:] == -1) and np.all(res['gain'][made:] == -np.inf)
    assert np.array_equal(res['vstar'][made:], np.zeros(S - made)) and not res['x'][made:].any()
    assert np.array_equal(np.flatnonzero(np.isnan(res['v'])), NAN_ROWS)
    if criterion == 'ivr':
        assert np.array_equal(np.flatnonzero(np.isnan(res['w'])), NAN_ROWS)
    # every pick that was made, along the device's own path, from scratch over the finite rows
    A0 = np.linalg.inv(C0)
    assert np.linalg.cond(A0) <= 1e4
    M = A0 @ CMC0 @ A0 if criterion == 'ivr' else None
    Xf = X[finite]
    place = {r: k for k, r in enumerate(finite)}
    worst_pick = worst_gain = 0.0
    for k in range(made):
        crit, v = from_scratch(Xf, A0, M, [place[int(r)] for r in res['index'][:k]], criterion)
        i = place[int(res['index'][k])]
        worst_pick = max(worst_pick, 1.0 - crit[i] / crit.max())
        worst_gain = max(worst_gain, abs(res['gain'][k] - crit[i]) / abs(crit[i]))
        assert crit[i] >= crit.max() * (1.0 - GATE), k
        assert abs(res['gain'][k] - crit[i]) <= GATE * abs(crit[i]), k
        assert abs(res['vstar'][k] - v[i]) <= GATE * abs(v[i]), k
    print(f"NaN rows, {criterion}, refresh {refresh_every}: worst shortfall of a pick {worst_pick:.3g}, worst relative error "
          f"of a gain {worst_gain:.3g}")


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_a_matrix_of_nan_picks_nothing_and_leaves_the_context_usable(device_ctx, criterion):
    S, nc = 40, 17
    slots, X, C0, CMC0 = staged_integers(device_ctx, S, nc)
    if criterion == 'variance':
        CMC0 = None
    before = device_ctx.design_select(slots, C0, CMC0, picks=2, keep=True)
    res = device_ctx.design_select(slots, np.full((nc, nc), np.nan), CMC0, picks=2, keep=True)
    assert np.all(res['index'] == -1) and np.all(res['gain'] == -np.inf) and not res['x'].any()
    assert np.all(np.isnan(res['v']))
    assert device_ctx.design_report()['launches'] == 6
    after = device_ctx.design_select(slots, C0, CMC0, picks=2, keep=True)
    for name in ('index', 'gain', 'vstar', 'x', 'v'):
        assert before[name].tobytes() == after[name].tobytes(), name
    assert np.array_equal(after['index'], dg.select_host(X, C0, CMC0, picks=2)['index'])


_ROUNDED = {}


def rounded_case(nc):
    """(pool columns without the ones, A0, C0, M, CMC0) of the nc-column continuous case; made once and never changed."""
    if nc not in _ROUNDED:
        rng = np.random.default_rng(nc)
        T = 4 * nc
        Xt = np.concatenate([np.ones((T, 1)), rng.uniform(-1.0, 1.0, size=(T, nc - 1))], axis=1)
        G = Xt.T @ Xt
        A0 = G + np.eye(nc)
        assert np.linalg.cond(A0) <= 1e4
        C0 = np.linalg.inv(A0)
        C0 = 0.5 * (C0 + C0.T)
        M = G / T
        CMC0 = C0 @ M @ C0
        CMC0 = 0.5 * (CMC0 + CMC0.T)
        cols = rng.uniform(-1.0, 1.0, size=(1029, nc - 1))
        for a in (cols, A0, C0, M, CMC0):
            a.setflags(write=False)
        _ROUNDED[nc] = (cols, A0, C0, M, CMC0)
    return _ROUNDED[nc]


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('refresh_every', (0, 5))
@pytest.mark.parametrize('nc', (129, 513, 768))
def test_rounded_and_wide_along_the_devices_own_path(device_ctx, nc, refresh_every, criterion):
    """test_design_gpu.follow_the_device at widths a four-input model does not reach, at its gate and under its condition
    (the worst figures are printed; DESIGN.md records them)."""
    picks = 12
    cols, A0, C0, M, CMC0 = rounded_case(nc)
    slots, X = stage(device_ctx, cols, np.zeros(cols.shape[0]))
    res = device_ctx.design_select(slots, C0, CMC0 if criterion == 'ivr' else None, picks=picks, refresh_every=refresh_every)
    assert len(set(res['index'].tolist())) == picks and res['index'].min() >= 0
    worst_pick = worst_gain = 0.0
    for k in range(picks):
        crit, v = from_scratch(X, A0, M, res['index'][:k], criterion)
        i = int(res['index'][k])
        worst_pick = max(worst_pick, 1.0 - crit[i] / crit.max())
        worst_gain = max(worst_gain, abs(res['gain'][k] - crit[i]) / abs(crit[i]), abs(res['vstar'][k] - v[i]) / abs(v[i]))
    print(f"S {X.shape[0]} nc {nc} picks {picks} {criterion} refresh {refresh_every}: worst shortfall of a pick "
          f"{worst_pick:.3g}, worst relative error of a gain or v* {worst_gain:.3g}")
    assert worst_pick <= GATE and worst_gain <= GATE
    XD = X[res['index']]
    logdet = np.linalg.slogdet(A0 + XD.T @ XD)[1] - np.linalg.slogdet(A0)[1]
    assert abs(logdet - np.sum(np.log1p(res['vstar']))) <= 1e-9 * picks
    assert np.array_equal(res['x'], XD)
    rep = device_ctx.design_report()
    assert rep['instance'] == criterion and rep['refreshes'] == ((picks - 1) // refresh_every if refresh_every else 0)
    assert rep['launches'] == 1 + rep['refreshes'] + 2 * picks and rep['lds_bytes'] == 8 * 16 * (-(-nc // 16) * 16)

"""fokl_predict at its edges: the three prediction kernels (csrc/fokl_predict.inc) against numpy.

Two references, everywhere:
  * exact -- columns and draw coefficients are small integers, so every prediction is an exactly representable integer
    whatever the order of summation or the use of FMA, the sum over the draws is exact, the mean is one correctly rounded
    division and the bounds are numpy's order statistics: ``np.array_equal`` on every path.  Small ranges give many ties.
  * rounded -- continuous data against a ``np.longdouble`` product, element by element within a few
    eps * (|X| @ |betas|') (the bound of test_device_dgemm_is_the_host_dgemm_to_rounding, never the global maximum);
    a bound must be one of its row's predictions and hold the right rank among them, predictions closer together than
    the bound allowed for.
Which kernel a call must take is computed here from the dispatcher's documented rule and asserted through
``DeviceContext.predict_report``, which also says whether a kernel's grid-stride loop went round again and how many
tiles of the matrix-pipe kernel took its exact fallback pass.
"""
import warnings

import numpy as np
import pytest

from helpers import upload, load_columns
from fokl_gpy_amd import _capi, getKernels, FoKLRoutines
from oracle import fokl_oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LDS_LIMIT = 150 * 1024
WIDTHS = (1, 2, 3, 4, 5, 13, 64, 255, 298, 299, 300, 301, 586, 768)


def evaluate_cut(draws):
    return int(np.floor(draws * 0.025) + 1)


def expected_kernel(nc, draws, cut, valu_forced=False):
    """(kernel, wide) fokl_predict must choose: the rule of its dispatcher, restated."""
    if cut is None:
        return _capi.PREDICT_VALU_LDS, (nc + 2) * 512 > LDS_LIMIT
    klo, khi = cut + 1, cut
    ncp = (nc + 3) & ~3
    lds_mfma = (ncp * 16 + 2 * max(32, klo) * 64) * 8
    if draws >= 64 and lds_mfma <= LDS_LIMIT and not valu_forced:
        return _capi.PREDICT_MFMA, False
    global_lists = klo > 128 or (nc + klo + khi) * 512 > LDS_LIMIT
    wide = (nc + (0 if global_lists else klo + khi)) * 512 > LDS_LIMIT
    if wide:
        global_lists = klo > 128
    return (_capi.PREDICT_VALU_GLOBAL if global_lists else _capi.PREDICT_VALU_LDS), wide


def stage(ctx, cols, y=None):
    """cols [n, k] -> slots 2 .. k + 1 of a fresh dataset; -> the slot list and X of [intercept] + cols."""
    n = cols.shape[0]
    upload(ctx, np.linspace(0.0, 1.0, n).reshape(n, 1), np.zeros(n) if y is None else y, O.KERNEL_BERNOULLI)
    if cols.shape[1]:
        load_columns(ctx, cols)
    slots = np.concatenate([[_capi.SLOT_ONES], np.arange(2, 2 + cols.shape[1])]).astype(np.int32)
    return slots, np.concatenate([np.ones((n, 1)), cols], axis=1)


def run(ctx, slots, betas, cut, valu=False, monkeypatch=None):
    """One fokl_predict call -> (mean, bounds or None); asserts the kernel the dispatcher had to take."""
    if valu:
        monkeypatch.setenv('FOKL_PREDICT_PATH', 'valu')
    try:
        out = ctx.predict(slots, betas, cut)
    finally:
        if valu:
            monkeypatch.delenv('FOKL_PREDICT_PATH')
    ran = ctx.predict_report()
    draws, nc = betas.shape
    assert (ran['kernel'], ran['wide']) == expected_kernel(nc, draws, cut, valu), (nc, draws, cut, valu, ran)
    rows = 16 if ran['kernel'] == _capi.PREDICT_MFMA else 64
    assert ran['tiles'] == (ctx.n + rows - 1) // rows and 1 <= ran['grid'] <= ran['tiles']
    if ran['kernel'] == _capi.PREDICT_MFMA:
        assert ran['tiles_done'] == ran['tiles'] and 0 <= ran['tiles_fallback'] <= ran['tiles']
    else:
        assert ran['tiles_done'] == 0 and ran['tiles_fallback'] == 0
    return (out[0], out[1]) if cut is not None else (out, None)


def exact_reference(X, betas, cut):
    """Integer data: (mean, bounds) as numpy has them, every value exact (float64 products and sums of small integers)."""
    mod = X @ betas.T
    assert np.max(np.abs(mod)) * betas.shape[0] < 2.0 ** 52 and np.array_equal(mod, np.rint(mod))
    mean = mod.sum(axis=1) / betas.shape[0]
    if cut is None:
        return mean, None
    srt = np.sort(mod, axis=1)
    return mean, np.stack([srt[:, cut], srt[:, betas.shape[0] - cut]], axis=1)


def check_exact(X, betas, cut, mean, bounds):
    want_mean, want_bounds = exact_reference(X, betas, cut)
    assert np.array_equal(mean, want_mean)
    if cut is not None:
        assert np.array_equal(bounds[:, 0], want_bounds[:, 0])
        assert np.array_equal(bounds[:, 1], want_bounds[:, 1])


def check_rounded(X, betas, cut, mean, bounds, slack=8.0, chunk=16384):
    """Continuous data against the longdouble product, in row chunks (the product of many rows is large)."""
    draws = betas.shape[0]
    bl, ba = betas.T.astype(np.longdouble), np.abs(betas.T)
    for r0 in range(0, X.shape[0], chunk):
        xs = X[r0:r0 + chunk]
        mod = xs.astype(np.longdouble) @ bl
        tol = slack * EPS * (np.abs(xs) @ ba)                             # per element
        got = mean[r0:r0 + chunk]
        # (the sum over the draws adds one rounding of the running total per draw on top of the elements' own: they add up
        # like a random walk, and the exact cases pin the mean to the last bit)
        assert np.all(np.abs(got - mod.mean(axis=1)) <= tol.mean(axis=1) + EPS * np.abs(mod).mean(axis=1) * (2 + np.sqrt(draws))), r0
        if cut is None:
            continue
        for side, rank in ((0, cut), (1, draws - cut)):
            v = bounds[r0:r0 + chunk, side][:, None].astype(np.longdouble)
            assert np.all(np.min(np.abs(mod - v) - tol, axis=1) <= 0), (r0, side)       # it is one of the row's predictions
            surely_below = np.sum(mod + tol < v, axis=1)
            maybe_at_or_below = np.sum(mod - tol <= v, axis=1)
            assert np.all(surely_below <= rank) and np.all(maybe_at_or_below >= rank + 1), (r0, side)


def integer_case(rng, n, nc, draws, span=3):
    cols = rng.integers(-span, span + 1, size=(n, nc - 1)).astype(np.float64)
    betas = rng.integers(-span, span + 1, size=(draws, nc)).astype(np.float64)
    return cols, betas


def real_case(rng, n, nc, draws):
    cols = rng.standard_normal((n, nc - 1))
    betas = rng.standard_normal((draws, nc)) * np.linspace(1.0, 0.2, nc) + rng.standard_normal(nc)
    return cols, betas


# ---------------------------------------------------------------------------------------------------------
# widths: no model is too wide (the VALU kernel reads the basis values from the columns when LDS cannot hold them)
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nc', WIDTHS)
def test_widths(device_ctx, nc, monkeypatch):
    rng = np.random.default_rng(1000 + nc)
    n = 150
    many = nc in (1, 13, 300, 301)                       # 6 200 draws (lists in device memory) for a few widths only
    for make, check in ((integer_case, check_exact), (real_case, check_rounded)):
        cols, _ = make(rng, n, nc, 1)
        slots, X = stage(device_ctx, cols)
        for draws in (1, 40, 100) + ((6200,) if many else ()):
            betas = make(rng, n, nc, draws)[1]
            cut = None if draws == 1 else evaluate_cut(draws)
            mean, bounds = run(device_ctx, slots, betas, cut)
            check(X, betas, cut, mean, bounds)
            if draws == 100:                                 # the VALU kernel's answer to the same call
                mean_v, bounds_v = run(device_ctx, slots, betas, cut, valu=True, monkeypatch=monkeypatch)
                check(X, betas, cut, mean_v, bounds_v)
                if check is check_exact:
                    assert np.array_equal(mean, mean_v) and np.array_equal(bounds, bounds_v)


# ---------------------------------------------------------------------------------------------------------
# draw counts: remainders of the four-draw groups, the hand-over at 64, the padded draws of the matrix-pipe kernel
# ---------------------------------------------------------------------------------------------------------

DRAW_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 79, 80, 81, 333, 1000, 1001)


@pytest.mark.parametrize('kind', ['integer', 'ternary', 'nearly_equal', 'positive', 'negative', 'real'])
def test_draw_counts(device_ctx, kind, monkeypatch):
    rng = np.random.default_rng(sum(map(ord, kind)))
    n, nc = 203, 13
    cols, _ = (real_case if kind == 'real' else integer_case)(rng, n, nc, 1)
    slots, X = stage(device_ctx, cols)
    check = check_rounded if kind == 'real' else check_exact
    for draws in DRAW_COUNTS:
        if kind == 'real':
            betas = real_case(rng, n, nc, draws)[1]
        elif kind == 'ternary':                              # coefficients in {-1, 0, 1}: ties everywhere
            betas = rng.integers(-1, 2, size=(draws, nc)).astype(np.float64)
        elif kind == 'nearly_equal':                         # all draws equal except a few
            betas = np.tile(rng.integers(-3, 4, size=(1, nc)).astype(np.float64), (draws, 1))
            odd = rng.permutation(draws)[:min(5, draws // 2)]
            betas[odd] = rng.integers(-3, 4, size=(odd.shape[0], nc))
        else:
            betas = integer_case(rng, n, nc, draws)[1]
            # every prediction strictly positive / negative through a large intercept: a zero-padded draw that were
            # counted would be the smallest / largest value of its row and show in the bounds
            if kind == 'positive':
                betas[:, 0] = 1000.0
            elif kind == 'negative':
                betas[:, 0] = -1000.0
        cut = None if draws == 1 else evaluate_cut(draws)
        mean, bounds = run(device_ctx, slots, betas, cut)
        check(X, betas, cut, mean, bounds)
        if kind == 'positive':
            assert np.all(mean > 0) and (cut is None or np.all(bounds > 0))
        if kind == 'negative':
            assert np.all(mean < 0) and (cut is None or np.all(bounds < 0))
        if draws >= 64:
            mean_v, bounds_v = run(device_ctx, slots, betas, cut, valu=True, monkeypatch=monkeypatch)
            if kind == 'real':
                check(X, betas, cut, mean_v, bounds_v)
            else:
                assert np.array_equal(mean, mean_v) and np.array_equal(bounds, bounds_v)


# ---------------------------------------------------------------------------------------------------------
# cuts: the documented range 1 <= cut < draws, and the seams of the dispatcher
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['integer', 'real'])
def test_cuts_at_100_draws(device_ctx, kind, monkeypatch):
    rng = np.random.default_rng(77)
    n, nc, draws = 203, 7, 100
    make, check = (integer_case, check_exact) if kind == 'integer' else (real_case, check_rounded)
    cols, betas = make(rng, n, nc, draws)
    slots, X = stage(device_ctx, cols)
    for cut in (1, 2, 3, 31, 32, 50, 98, 99):               # klo = 32 -> 33 is where max(PM_CAP, klo) becomes klo
        mean, bounds = run(device_ctx, slots, betas, cut)
        check(X, betas, cut, mean, bounds)
        mean_v, bounds_v = run(device_ctx, slots, betas, cut, valu=True, monkeypatch=monkeypatch)
        check(X, betas, cut, mean_v, bounds_v)
        if kind == 'integer':
            assert np.array_equal(mean, mean_v) and np.array_equal(bounds, bounds_v)


@pytest.mark.parametrize('kind', ['integer', 'real'])
def test_cuts_around_the_list_seams_at_6200_draws(device_ctx, kind, monkeypatch):
    """9 columns, 6 200 draws: the matrix-pipe kernel's LDS holds lists of up to 148 values per lane (149 and more go to
    the VALU kernel with lists in device memory); the VALU kernel's own lists leave LDS after 128."""
    rng = np.random.default_rng(78)
    n, nc, draws = 130, 9, 6200
    make, check = (integer_case, check_exact) if kind == 'integer' else (real_case, check_rounded)
    cols, betas = make(rng, n, nc, draws)
    slots, X = stage(device_ctx, cols)
    for klo in (127, 128, 129, 147, 148, 149, 150, 157):
        cut = klo - 1
        assert expected_kernel(nc, draws, cut)[0] == (_capi.PREDICT_MFMA if klo <= 148 else _capi.PREDICT_VALU_GLOBAL)
        assert expected_kernel(nc, draws, cut, True)[0] == (_capi.PREDICT_VALU_LDS if klo <= 128 else _capi.PREDICT_VALU_GLOBAL)
        mean, bounds = run(device_ctx, slots, betas, cut)
        check(X, betas, cut, mean, bounds)
        mean_v, bounds_v = run(device_ctx, slots, betas, cut, valu=True, monkeypatch=monkeypatch)
        check(X, betas, cut, mean_v, bounds_v)
        if kind == 'integer':
            assert np.array_equal(mean, mean_v) and np.array_equal(bounds, bounds_v)


def test_the_matrix_pipe_kernel_hands_wide_models_back_where_its_lds_ends(device_ctx):
    """klo <= 32: (ncp * 16 + 4096) * 8 bytes reach 150 KiB at 944 padded columns and pass it at 948."""
    rng = np.random.default_rng(79)
    n, draws, cut = 70, 64, 2
    cols, _ = integer_case(rng, n, 949, 1)
    slots, X = stage(device_ctx, cols)
    for nc in (940, 944, 945, 949):
        assert expected_kernel(nc, draws, cut) == ((_capi.PREDICT_MFMA, False) if nc <= 944 else (_capi.PREDICT_VALU_LDS, True))
        betas = rng.integers(-3, 4, size=(draws, nc)).astype(np.float64)
        mean, bounds = run(device_ctx, slots[:nc], betas, cut)
        check_exact(X[:, :nc], betas, cut, mean, bounds)


# ---------------------------------------------------------------------------------------------------------
# rows: ragged last tiles, and enough rows that every kernel's grid-stride loop goes round again
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 15, 16, 17, 63, 64, 65, 4099])
def test_row_counts(device_ctx, n, monkeypatch):
    rng = np.random.default_rng(n)
    nc = 6
    for make, check in ((integer_case, check_exact), (real_case, check_rounded)):
        cols, _ = make(rng, n, nc, 1)
        slots, X = stage(device_ctx, cols)
        for draws, cut in ((1, None), (40, 2), (80, 3), (200, 160)):
            betas = make(rng, n, nc, draws)[1]
            mean, bounds = run(device_ctx, slots, betas, cut)
            check(X, betas, cut, mean, bounds)
            if draws == 80:
                mean_v, bounds_v = run(device_ctx, slots, betas, cut, valu=True, monkeypatch=monkeypatch)
                check(X, betas, cut, mean_v, bounds_v)


def test_every_kernel_loops_over_more_tiles_than_its_grid(device_ctx, monkeypatch):
    """300 007 rows (70 001 for the lists in device memory): more 16-row tiles, 64-row blocks than any grid here, so every
    wavefront takes a second trip.  The first trip's rows carry the more extreme predictions, in both directions: a list
    entry, a candidate count or a running total left over from it would sit among a later row's extremes."""
    rng = np.random.default_rng(300007)
    n, nc, draws, cut = 300_007, 6, 80, 3
    cols, betas = integer_case(rng, n, nc, draws)
    cols[:70_000] *= 7.0
    slots, X = stage(device_ctx, cols)
    mod = X @ betas.T
    want_mean = mod.sum(axis=1) / draws
    srt = np.sort(mod, axis=1)
    del mod
    for this_cut, valu in ((None, False), (cut, False), (cut, True)):
        b = betas if this_cut is not None else betas[:1]
        mean, bounds = run(device_ctx, slots, b, this_cut, valu=valu, monkeypatch=monkeypatch)
        ran = device_ctx.predict_report()
        assert ran['tiles'] > ran['grid'], ran                       # the loop really went round again
        if this_cut is None:
            assert np.array_equal(mean, X @ b[0])
            continue
        assert ran['kernel'] == (_capi.PREDICT_VALU_LDS if valu else _capi.PREDICT_MFMA)
        assert np.array_equal(mean, want_mean)
        assert np.array_equal(bounds[:, 0], srt[:, cut]) and np.array_equal(bounds[:, 1], srt[:, draws - cut])
    del srt

    # continuous data over the same rows, mean only and on the matrix pipe
    cols_r, betas_r = real_case(rng, n, nc, draws)
    slots, X = stage(device_ctx, cols_r)
    mean, bounds = run(device_ctx, slots, betas_r, cut)
    check_rounded(X, betas_r, cut, mean, bounds)
    mean, _ = run(device_ctx, slots, betas_r[:1], None)
    check_rounded(X, betas_r[:1], None, mean, None)

    # lists in device memory: 200 draws, cut = 160 keeps the matrix-pipe kernel out (its LDS ends at 148 per lane)
    n, draws, cut = 70_001, 200, 160
    cols, betas = integer_case(rng, n, nc, draws)
    cols[:20_000] *= 7.0
    slots, X = stage(device_ctx, cols)
    mean, bounds = run(device_ctx, slots, betas, cut)
    ran = device_ctx.predict_report()
    assert ran['kernel'] == _capi.PREDICT_VALU_GLOBAL and ran['tiles'] > ran['grid'], ran
    check_exact(X, betas, cut, mean, bounds)


# ---------------------------------------------------------------------------------------------------------
# slots
# ---------------------------------------------------------------------------------------------------------

def test_slot_lists_in_any_order_and_after_the_pool_has_grown(device_ctx, monkeypatch):
    rng = np.random.default_rng(5)
    n = 333
    cols, _ = integer_case(rng, n, 11, 1)
    y = rng.integers(-3, 4, n).astype(np.float64)
    stage(device_ctx, cols, y)
    by_slot = {_capi.SLOT_ONES: np.ones(n), _capi.SLOT_Y: y, **{2 + j: cols[:, j] for j in range(10)}}
    # neither contiguous nor ordered, one slot twice, the intercept in the middle, the data column as a column
    slots = np.array([9, 3, _capi.SLOT_ONES, 11, 3, _capi.SLOT_Y, 2, 7], dtype=np.int32)
    X = np.stack([by_slot[int(s)] for s in slots], axis=1)
    for grown in (False, True):
        if grown:
            before = device_ctx.slot_capacity
            device_ctx.reserve_slots(before + 300)               # new chunks, a new table of slot addresses
            assert device_ctx.slot_capacity >= before + 300
        for draws, cut in ((1, None), (40, 2), (100, 3)):
            betas = rng.integers(-3, 4, size=(draws, slots.shape[0])).astype(np.float64)
            mean, bounds = run(device_ctx, slots, betas, cut)
            check_exact(X, betas, cut, mean, bounds)
            if draws == 100:
                mean, bounds = run(device_ctx, slots, betas, cut, valu=True, monkeypatch=monkeypatch)
                check_exact(X, betas, cut, mean, bounds)


# ---------------------------------------------------------------------------------------------------------
# refusals: argument errors returned before any launch
# ---------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_leave_the_context_usable(device_ctx):
    rng = np.random.default_rng(6)
    n = 100
    cols, betas = integer_case(rng, n, 5, 50)
    slots, X = stage(device_ctx, cols)
    nothing = dict(kernel=_capi.PREDICT_NONE, wide=False, grid=0, tiles=0, tiles_done=0, tiles_fallback=0)

    def refused(code, sl, b, cut):
        with pytest.raises(_capi.FoklNativeError) as err:
            device_ctx.predict(sl, b, cut)
        assert err.value.code == code
        assert device_ctx.predict_report() == nothing

    ERR_ARG, ERR_STATE = -2, -3
    for sl, b, cut in ((slots, betas, 0), (slots, betas, 50), (slots, betas, 51), (slots, betas, -1),
                       (slots, betas[:0], None), (slots[:0], betas[:, :0], None),
                       (np.array([0, 2, device_ctx.slot_capacity, 3, 4], dtype=np.int32), betas, 2),
                       (np.array([0, 2, -1, 3, 4], dtype=np.int32), betas, None)):
        run(device_ctx, slots, betas, 2)                         # (something to report, so that the refusal's zeros show)
        refused(ERR_ARG, sl, b, cut)
    mean, bounds = run(device_ctx, slots, betas, 2)
    check_exact(X, betas, 2, mean, bounds)
    mean, _ = run(device_ctx, slots, betas[:1], None)
    check_exact(X, betas[:1], None, mean, None)

    fresh = _capi.DeviceContext(device_ctx.device)               # a context without a dataset
    try:
        out = np.zeros(n)
        rc = fresh._lib.fokl_predict(fresh._h, _capi._ptr(slots), 5, _capi._ptr(betas), 50, 0, _capi._ptr(out), None)
        assert rc == ERR_STATE and b'fokl_upload' in fresh._lib.fokl_last_error(fresh._h)
        assert fresh.predict_report() == nothing
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------
# which pass ran
# ---------------------------------------------------------------------------------------------------------

def test_the_filter_pass_serves_gaussian_draws_and_the_fallback_the_rest(device_ctx):
    rng = np.random.default_rng(2024)
    n, nc, draws = 3000, 13, 1000
    cols = rng.standard_normal((n, nc - 1))
    slots, X = stage(device_ctx, cols)
    cut = evaluate_cut(draws)
    tiles = (n + 15) // 16

    betas = rng.standard_normal((draws, nc))
    mean, bounds = run(device_ctx, slots, betas, cut)
    ran = device_ctx.predict_report()
    assert ran['kernel'] == _capi.PREDICT_MFMA and ran['tiles_done'] == tiles
    assert ran['tiles_fallback'] < tiles / 5, ran                # (a lane holds 32 candidates and expects about 15)
    check_rounded(X, betas, cut, mean, bounds)

    same = np.tile(rng.standard_normal((1, nc)), (draws, 1))     # sigma = 0: nothing lies beyond mean -/+ z sigma
    mean, bounds = run(device_ctx, slots, same, cut)
    assert device_ctx.predict_report()['tiles_fallback'] == tiles
    check_rounded(X, same, cut, mean, bounds)

    mean, bounds = run(device_ctx, slots, betas[:100], 99)       # the lists hold every draw: no filter can serve that
    assert device_ctx.predict_report()['tiles_fallback'] == tiles
    check_rounded(X, betas[:100], 99, mean, bounds)


# ---------------------------------------------------------------------------------------------------------
# through the class
# ---------------------------------------------------------------------------------------------------------

def _model(rng, m, terms, max_order, draws):
    """A FoKL object handed ``betas`` and ``mtx`` of a model of ``terms`` distinct terms (+ intercept) over m inputs."""
    grid = np.stack(np.meshgrid(*[np.arange(max_order + 1)] * m, indexing='ij'), axis=-1).reshape(-1, m)[1:]
    mtx = grid[rng.permutation(grid.shape[0])[:terms]].astype(np.int64)
    assert mtx.shape[0] == terms and np.unique(mtx, axis=0).shape[0] == terms
    mean = rng.standard_normal(terms + 1) / np.arange(1, terms + 2) ** 0.5
    betas = mean * (1 + 0.2 * rng.standard_normal((draws, terms + 1)))
    model = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', UserWarnings=False, ConsoleOutput=False)
    model.betas, model.mtx, model.draws = betas, mtx, draws
    model.minmax = [[0.0, 1.0]] * m
    return model


def _oracle_bound(model, x, betas_abs):
    cols = O.build_columns_c(x, None, getKernels.bernoulli(), O.KERNEL_BERNOULLI, np.asarray(model.mtx, dtype=np.int32))
    return 32 * EPS * (np.concatenate([np.ones((x.shape[0], 1)), np.abs(cols)], axis=1) @ betas_abs)


def test_evaluate_and_coverage3_on_wide_models_and_many_rows():
    rng = np.random.default_rng(320)
    phis = getKernels.bernoulli()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # 320 columns: more than LDS holds per row -- the everyday mean-only call, then bounds on either kernel
        model = _model(rng, 4, 319, 4, 100)
        x = rng.random((2000, 4))
        for draws, bounds_wanted in ((100, False), (40, True), (100, True)):
            model.setnos = setnos = rng.permutation(100)[:draws]
            got = model.evaluate(x, draws=draws, ReturnBounds=bounds_wanted)
            want = O.evaluate(x, model.betas, model.mtx, phis, O.KERNEL_BERNOULLI, draws, setnos, return_bounds=bounds_wanted)
            tol = _oracle_bound(model, x, np.abs(model.betas[setnos]).max(axis=0))
            if bounds_wanted:
                assert np.all(np.abs(got[0] - want[0]) <= tol) and np.all(np.abs(got[1] - want[1]) <= tol[:, None])
            else:
                assert np.all(np.abs(got - want) <= tol)

        # 300 000 rows of a 12-term model, checked on a sample and at both ends
        model = _model(rng, 4, 12, 3, 100)
        n = 300_000
        x = rng.random((n, 4))
        model.setnos = setnos = np.arange(100)
        mean, bounds = model.evaluate(x, ReturnBounds=True)
        sample = np.unique(np.concatenate([np.arange(70), np.arange(n - 70, n), rng.integers(0, n, 5000)]))
        want = O.evaluate(x[sample], model.betas, model.mtx, phis, O.KERNEL_BERNOULLI, 100, setnos, return_bounds=True)
        tol = _oracle_bound(model, x[sample], np.abs(model.betas).max(axis=0))
        assert np.all(np.abs(mean[sample] - want[0]) <= tol) and np.all(np.abs(bounds[sample] - want[1]) <= tol[:, None])
        assert np.all(bounds[:, 0] <= mean) and np.all(mean <= bounds[:, 1])

        # coverage3: the same numbers, and the reference's RMSE expression (FR:1193: |mean(mean) - mean(data)|)
        data = mean + 0.1 * rng.standard_normal(n)
        model.inputs, model.data = x, data
        mean_c, bounds_c, rmse = model.coverage3()
        assert np.array_equal(mean_c, mean) and np.array_equal(bounds_c, bounds)
        assert rmse == O.coverage_rmse(mean, data)
        assert abs(rmse - abs(np.mean(mean - data))) <= 8 * EPS * np.mean(np.abs(mean) + np.abs(data))

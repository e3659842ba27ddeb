"""fokl_score_rows (csrc/fokl_score_device.inc) and score.score on the device against their host statement.

Two references for the kernel:
  * exact -- columns, coefficients and y are small integers and every sigsqd is 0.5, so that h = 0.5 / sigsqd = 1 and
    r = -ll = (y - X beta)^2 + log(pi) / 2 is the same sequence of correctly rounded operations on both sides whatever the
    order of the product's sum: ``np.array_equal`` on tail_out (the sorted top M + 1 of r - max r), on max r and on M'.  This
    pins the lane map (a lane holds four draws of ONE row), the masking of rows past the end and of padding draws, the
    threshold test, the eviction from the list and the sort, with heavy ties (a width of 1 leaves seven distinct values).
  * rounded -- continuous data against score_rows_host: lppd, ll_mean and p_waic to the project's 1e-12 of the scale,
    elpd_loo, khat and sigma to 100 times the statement's own rounding sensitivity as test_score_host measures it on the
    conjugate case (conjugate_sensitivity: ll perturbed by 1e-15 relative moves them by about 2e-15, 3e-14 and 5e-15, so
    the bounds are about 2e-13, 3e-12 and 5e-13 whatever the case under test), because the device's exp, log and log1p
    differ from libm's by a few ulp.  Nothing here is tuned against the kernel.
``DeviceContext.score_report`` says what ran.
"""
import warnings

import numpy as np
import pytest

from helpers import upload, load_columns
from test_score_host import conjugate_sensitivity
from fokl_gpy_amd import _capi, FoKLRoutines
from fokl_gpy_amd import score as sc
from oracle import fokl_oracle as O

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 1000, 100003)
DRAWS = (25, 63, 64, 65, 1000, 1003)
WIDTHS = (1, 5, 128, 129, 300, 600)
LARGEST = sc.max_draws_loo()                                 # 29 013: M + 1 = FOKL_SCORE_MAX_TAIL


def stage(ctx, cols, y):
    """cols [n, k] -> slots 2 .. k + 1 of a fresh dataset with data y; -> the slot list and X of [intercept] + cols."""
    n = cols.shape[0]
    upload(ctx, np.linspace(0.0, 1.0, n).reshape(n, 1), y, O.KERNEL_BERNOULLI)
    if cols.shape[1]:
        load_columns(ctx, cols)
    slots = np.concatenate([[_capi.SLOT_ONES], np.arange(2, 2 + cols.shape[1])]).astype(np.int32)
    return slots, np.concatenate([np.ones((n, 1)), cols], axis=1)


def lds_bytes(nc, E, want_loo=True):
    ncp = -(-nc // 4) * 4
    return 8 * (16 * ncp + (16 * (sc.tail_len(E) + 1) + 16 * 64 if want_loo else 16))


def exact_reference(X, y, betas, sig):
    """(tail [S, M + 1], max r [S], M' [S]) of the statement, by whole-array numpy."""
    r = -sc.log_likelihood(X, y, betas, sig)
    E = r.shape[1]
    M = sc.tail_len(E)
    rmax = r.max(axis=1)
    top = np.sort(r - rmax[:, None], axis=1)[:, E - M - 1:]
    u = np.maximum(top[:, :1], sc.LOG_DBL_MIN)
    return top, rmax, (top[:, 1:] > u).sum(axis=1)


def check_exact(ctx, S, E, nc, seed=0):
    rng = np.random.default_rng(seed)
    cols = rng.integers(-3, 4, size=(S, nc - 1)).astype(np.float64)
    betas = rng.integers(-3, 4, size=(E, nc)).astype(np.float64)
    y = rng.integers(-20, 21, size=S).astype(np.float64)
    sig = np.full(E, 0.5)
    slots, X = stage(ctx, cols, y)
    stats, tail = ctx.score_rows(slots, betas, sig, True, True)
    top, rmax, n_tail = exact_reference(X, y, betas, sig)
    assert tail.shape == top.shape and np.array_equal(tail, top), (S, E, nc)
    assert np.array_equal(stats[:, 6], rmax) and np.array_equal(stats[:, 7], n_tail), (S, E, nc)
    assert np.all(np.isfinite(stats[:, :3]))
    rep = ctx.score_report()
    assert rep['instance'] == 'waic_loo' and rep['row_tiles'] == -(-S // 16) and 1 <= rep['grid'] <= rep['row_tiles']
    assert rep['tail_capacity'] == sc.tail_len(E) + 1 and rep['lds_bytes'] == lds_bytes(nc, E)
    assert rep['raw_rows'] == int(np.isinf(stats[:, 4]).sum()) and rep['kernel_ms'] > 0.0
    assert np.array_equal(np.isinf(stats[:, 4]), (n_tail <= 4) | (stats[:, 5] == 0.0))
    return rep, stats


def test_the_lane_map_a_lane_holds_draws_of_one_row(device_ctx):
    """yhat[row][draw] = draw + 1000 row and y = 0: r - log(pi) / 2 = (draw + 1000 row)^2 names its row and its draw; were
    rows and draws (or a lane's four draws) placed otherwise, a row's tail would hold another row's values."""
    S, E = 37, 41
    slots, X = stage(device_ctx, np.arange(S, dtype=np.float64)[:, None], np.zeros(S))
    betas = np.stack([np.arange(E, dtype=np.float64), np.full(E, 1000.0)], axis=1)
    sig = np.full(E, 0.5)
    stats, tail = device_ctx.score_rows(slots, betas, sig, True, True)
    M = sc.tail_len(E)
    c = -sc.likelihood_constants(sig)[0][0]
    r = (np.arange(E)[None, :] + 1000.0 * np.arange(S)[:, None]) ** 2 + c
    assert np.array_equal(stats[:, 6], r[:, -1])
    assert np.array_equal(tail, r[:, E - M - 1:] - r[:, -1:])
    n_tail = (tail[:, 1:] > np.maximum(tail[:, :1], sc.LOG_DBL_MIN)).sum(axis=1)   # beyond row 0 the weights underflow: M' = 1
    assert np.array_equal(stats[:, 7], n_tail) and n_tail[0] == M and np.all(n_tail[1:] == 1)


@pytest.mark.parametrize('S', ROWS[:5])
@pytest.mark.parametrize('E', DRAWS)
def test_exact_over_rows_and_draws(device_ctx, S, E):
    check_exact(device_ctx, S, E, nc=5, seed=S + E)


@pytest.mark.parametrize('E', (25, 64, 1003))
def test_exact_over_many_rows_the_tile_loop_goes_round(device_ctx, E):
    rep, _ = check_exact(device_ctx, ROWS[5], E, nc=5, seed=E)
    assert rep['row_tiles'] > rep['grid']


@pytest.mark.parametrize('S', (1, 17))
def test_exact_at_the_largest_number_of_draws(device_ctx, S):
    rep, _ = check_exact(device_ctx, S, LARGEST, nc=5, seed=S)
    assert rep['tail_capacity'] == _capi.SCORE_MAX_TAIL == 512


@pytest.mark.parametrize('nc', WIDTHS)
@pytest.mark.parametrize('S, E', [(17, 65), (1000, 64)])
def test_exact_over_widths_with_heavy_ties(device_ctx, nc, S, E):
    _, stats = check_exact(device_ctx, S, E, nc, seed=nc)
    if nc == 1:                                              # seven distinct predictions: ties everywhere
        assert np.mean(stats[:, 7] < sc.tail_len(E)) > 0.5


def continuous_case(S, E, nc, seed):
    rng = np.random.default_rng(seed)
    cols = rng.standard_normal((S, nc - 1))
    mean = rng.standard_normal(nc) / np.sqrt(nc)
    betas = mean + 0.05 * rng.standard_normal((E, nc)) / np.sqrt(nc)
    X = np.concatenate([np.ones((S, 1)), cols], axis=1)
    y = X @ mean + 0.5 * rng.standard_normal(S)
    sig = 0.25 * (1.0 + 0.2 * rng.random(E))
    return cols, betas, y, sig


@pytest.mark.parametrize('S, E, nc', [(500, 1000, 100), (1000, 64, 5), (17, 4000, 300), (100, 1003, 129), (33, 25, 1),
                                      (2003, 200, 20)])
def test_rounded_against_the_host_statement(device_ctx, S, E, nc):
    cols, betas, y, sig = continuous_case(S, E, nc, S + E + nc)
    slots, X = stage(device_ctx, cols, y)
    stats, tail = device_ctx.score_rows(slots, betas, sig, True, True)
    ref, ref_tail = sc.score_rows_host(X, y, betas, sig, want_tail=True)
    ll = sc.log_likelihood(X, y, betas, sig)
    scale = max(np.abs(ll).max(), 1.0)
    moved = conjugate_sensitivity()
    err = np.abs(stats - ref)
    finite = np.isfinite(ref[:, 4])
    print(f"S {S} E {E} nc {nc}: lppd {err[:, 0].max():.2e} ll_mean {err[:, 1].max():.2e} p_waic {err[:, 2].max():.2e} of scale "
          f"{scale:.1f}; elpd_loo {err[:, 3].max():.2e} khat {err[finite, 4].max():.2e} sigma {err[:, 5].max():.2e} against "
          f"the conjugate case's sensitivity {moved} x 100; max khat {ref[finite, 4].max():.2f}")
    assert np.array_equal(np.isfinite(stats[:, 4]), finite) and np.array_equal(stats[:, 7], ref[:, 7])
    assert err[:, 0].max() <= 1e-12 * scale and err[:, 1].max() <= 1e-12 * scale and err[:, 2].max() <= 1e-12 * scale ** 2
    assert err[:, 6].max() <= 1e-12 * scale and np.max(np.abs(tail - ref_tail)) <= 1e-12 * scale
    assert err[:, 3].max() <= 100.0 * moved[0]
    assert err[finite, 4].max() <= 100.0 * moved[1]
    assert err[:, 5].max() <= 100.0 * moved[2]
    again, again_tail = device_ctx.score_rows(slots, betas, sig, True, True)
    assert np.array_equal(again, stats) and np.array_equal(again_tail, tail)                # no atomics: the same bits


def test_without_loo_the_psis_columns_are_zero_and_no_list_is_kept(device_ctx):
    cols, betas, y, sig = continuous_case(300, 20, 7, 1)                                    # fewer than 25 draws: no limit
    slots, X = stage(device_ctx, cols, y)
    stats = device_ctx.score_rows(slots, betas, sig, False)
    ref = sc.score_rows_host(X, y, betas, sig, want_loo=False)
    scale = max(np.abs(sc.log_likelihood(X, y, betas, sig)).max(), 1.0)
    assert np.array_equal(stats[:, 3:], np.zeros((300, 5)))
    assert np.max(np.abs(stats[:, :2] - ref[:, :2])) <= 1e-12 * scale and np.max(np.abs(stats[:, 2] - ref[:, 2])) <= 1e-12 * scale ** 2
    rep = device_ctx.score_report()
    assert rep['instance'] == 'waic' and rep['tail_capacity'] == 0 and rep['raw_rows'] == 0
    assert rep['lds_bytes'] == lds_bytes(7, 20, want_loo=False)
    assert np.array_equal(device_ctx.score_rows(slots, betas, sig, False), stats)
    one = device_ctx.score_rows(slots, betas[:1], sig[:1], False)                           # a single draw: lppd = ll, p_waic = 0
    assert np.array_equal(one[:, 2], np.zeros(300)) and np.array_equal(one[:, 0], one[:, 1])


def test_copies_of_a_single_draw_take_the_raw_branch(device_ctx):
    cols, betas, y, sig = continuous_case(50, 64, 9, 2)
    slots, X = stage(device_ctx, cols, y)
    stats = device_ctx.score_rows(slots, np.tile(betas[:1], (64, 1)), np.full(64, 0.3), True)
    ll = sc.log_likelihood(X, y, betas[:1], [0.3])[:, 0]
    assert np.array_equal(stats[:, 2], np.zeros(50)) and np.all(stats[:, 4] == np.inf) and np.all(stats[:, 7] == 0)
    assert np.max(np.abs(stats[:, [0, 1, 3]] - ll[:, None])) <= 1e-12 * max(np.abs(ll).max(), 1.0)
    assert device_ctx.score_report()['raw_rows'] == 50


def test_refusals_leave_the_dataset_intact(device_ctx):
    ctx = device_ctx
    cols, betas, y, sig = continuous_case(200, 30, 4, 3)
    slots, X = stage(ctx, cols, y)
    before = ctx.score_rows(slots, betas, sig, True)

    def intact():
        assert ctx.score_report()['instance'] == 'none' and ctx.score_report()['grid'] == 0
        assert np.array_equal(ctx.read_slot(2), cols[:, 0]) and np.array_equal(ctx.read_slot(_capi.SLOT_Y), y)
        assert np.array_equal(ctx.score_rows(slots, betas, sig, True), before)

    E = LARGEST + 1                                          # a tail beyond the list's capacity
    with pytest.raises(_capi.FoklNativeError, match='FOKL_SCORE_MAX_TAIL = 512') as exc:
        ctx.score_rows(slots, np.tile(betas[:1], (E, 1)), np.full(E, 0.3), True)
    assert exc.value.code == -2
    intact()
    assert ctx.score_rows(slots, np.tile(betas[:1], (E, 1)), np.full(E, 0.3), False).shape == (200, 8)   # no limit without loo
    with pytest.raises(_capi.FoklNativeError, match='at least 25 draws') as exc:
        ctx.score_rows(slots, betas[:24], sig[:24], True)
    assert exc.value.code == -2
    intact()
    with pytest.raises(_capi.FoklNativeError, match='positive') as exc:
        ctx.score_rows(slots, betas, -sig, True)
    assert exc.value.code == -2
    for bad in (np.nan, np.inf):                             # draws of a flagged chain, or overflowed ones: refused natively
        spoiled = betas.copy()
        spoiled[17, 2] = bad
        for want_loo in (True, False):
            with pytest.raises(_capi.FoklNativeError, match='fokl_score_rows: every coefficient must be finite') as exc:
                ctx.score_rows(slots, spoiled, sig, want_loo)
            assert exc.value.code == -2
            intact()
    with pytest.raises(_capi.FoklNativeError, match='slot'):
        ctx.score_rows(np.array([0, 2, 3, 9999], dtype=np.int32), betas, sig, True)
    with pytest.raises(ValueError):
        ctx.score_rows(slots, betas[:, :2], sig, True)
    with pytest.raises(ValueError):
        ctx.score_rows(slots, betas, sig[:-1], True)
    intact()


def test_a_tail_out_beyond_free_memory_is_refused(device_ctx, monkeypatch):
    """82 MB of tail_out where 100 MiB of the device count as free (FOKL_SCORE_FREE_BYTES caps what the call takes
    hipMemGetInfo's answer for) and 64 MiB are to stay spare: refused before anything is allocated, with every buffer of
    its full size, so that a call that was not refused would do no harm.  Without tail_out, and without the cap, the same
    call runs."""
    ctx = device_ctx
    S = 20000
    rng = np.random.default_rng(8)
    y = rng.standard_normal(S)
    upload(ctx, np.linspace(0.0, 1.0, S).reshape(S, 1), y, O.KERNEL_BERNOULLI)
    slots = np.array([_capi.SLOT_ONES], dtype=np.int32)
    betas, sig = 0.1 * rng.standard_normal((LARGEST, 1)), np.full(LARGEST, 0.5)
    monkeypatch.setenv('FOKL_SCORE_FREE_BYTES', str(100 << 20))
    with pytest.raises(_capi.FoklNativeError, match=f'{S * 512 * 8} bytes of tail_out.*free \\(pass no tail_out') as exc:
        ctx.score_rows(slots, betas, sig, True, True)
    assert exc.value.code == -2
    assert ctx.score_report()['instance'] == 'none' and ctx.n == S
    assert np.array_equal(ctx.read_slot(_capi.SLOT_Y), y)
    stats = ctx.score_rows(slots, betas, sig, True)                                        # no tail_out: it fits
    assert ctx.score_report()['instance'] == 'waic_loo'
    monkeypatch.setenv('FOKL_SCORE_FREE_BYTES', str(1 << 20))                              # not even the statistics fit
    with pytest.raises(_capi.FoklNativeError, match='0 bytes of tail_out.*score the rows in parts') as exc:
        ctx.score_rows(slots, betas[:25], sig[:25], False)
    assert exc.value.code == -2
    monkeypatch.delenv('FOKL_SCORE_FREE_BYTES')
    again, tail = ctx.score_rows(slots, betas, sig, True, True)                            # the device itself has the room
    assert np.array_equal(again, stats) and tail.shape == (S, 512) and np.all(tail[:, -1] == 0.0)


# ---------------------------------------------------------------------------------------------------------
# score on the device against score_host, after a fit
# ---------------------------------------------------------------------------------------------------------

def test_score_after_a_fit_and_a_resample():
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
        with pytest.raises(ValueError, match='resample'):
            model.score()
        post = model.resample(chains=4, draws=100, burnin=20, seed=5)
        assert not post.flagged.any()
        res = model.score(post)
        assert model.setnos is None and np.array_equal(np.random.get_state()[1], state)
        host = sc.score_host(post.betas, post.sigsqd, model.mtx, model.phis, model.kernel, model.inputs, model.data)
        assert sorted(res.keys()) == sorted(host.keys()) and res.rows == n and res.draws == 400
        for name in ('lppd', 'elpd_waic', 'p_waic', 'se_waic', 'elpd_loo', 'p_loo', 'se_loo'):
            assert res[name] == pytest.approx(host[name], rel=1e-9, abs=1e-9), name
        for name in ('lppd', 'll_mean', 'p_waic', 'elpd_loo', 'khat'):
            assert np.allclose(res.pointwise[name], host.pointwise[name], rtol=1e-8, atol=1e-8), name
        assert res.khat_bad == host.khat_bad and res.elpd_loo <= res.lppd and res.p_loo > 0.0
        thin = model.score(post, draws=np.arange(0, 400, 2), method='waic')
        assert thin.draws == 200 and 'elpd_loo' not in thin
        # a deliberately under-fitted model: the first term only, with a posterior of its own
        small_post = model.resample(mtx=model.mtx[:1], chains=4, draws=100, burnin=20, seed=5)
        small = model.score(small_post, mtx=model.mtx[:1])
        verdict = sc.compare(res, small)
        assert verdict.measure == 'elpd_loo' and small.elpd_loo < res.elpd_loo and verdict.elpd_diff > 2.0 * verdict.se_diff
        # held-out rows: the log predictive density only, raw inputs normalised as the model's were
        held = model.score(post, inputs=x, data=model.data, clean=True, method='lpd')
        assert held.method == ('lpd',) and 'elpd_loo' not in held and held.lppd == pytest.approx(res.lppd, rel=1e-12)
        x_test = 0.05 + 0.9 * rng.random((501, 3))
        y_test = np.sin(4 * x_test[:, 0]) + x_test[:, 1] * x_test[:, 2] + 0.05 * rng.standard_normal(501)
        new = model.score(post, inputs=x_test, data=y_test, clean=True, method='lpd')
        assert new.rows == 501 and np.isfinite(new.lppd) and new.lppd / 501 > res.lppd / n - 1.0

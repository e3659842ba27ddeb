"""fokl_predictive_rows (csrc/fokl_predictive_device.inc) and predictive.predictive on the device against their host statement.

Two references for the kernel:
  * exact -- columns, coefficients and y are small integers, every sigsqd is 1 (sd = 1) and z is passed as integers through
    the low-level ``predictive_rows`` with ``max_passes = 0``: s1, s2, min mu, max mu and the brackets lo, hi are integer
    arithmetic whatever the order of the sums, ``np.array_equal`` against whole-array numpy.  This pins the lane map (a lane
    holds four draws of ONE row), the masking of rows past the end and of padding draws, and the merge of the quarters.
  * rounded -- continuous data against predictive_rows_host: pit, mean and var to 100 times the statement's own rounding
    sensitivity on that very case (test_predictive_host.rounding_sensitivity: every mu perturbed by 1e-15 sum |X beta|),
    every device q inside the statement's pass-0 bracket with |F_host(q_dev) - p| <= ftol + 100 times the sensitivity of F,
    the device's own residual equal to F_host(q_dev) - p to the same bound.  The test computes the sensitivity on the
    host: nothing here is tuned against the kernel.
``DeviceContext.predictive_report`` says what ran.
"""
import warnings

import numpy as np
import pytest

from helpers import upload
from test_score_gpu import stage, continuous_case
from test_predictive_host import rounding_sensitivity
from fokl_gpy_amd import _capi, FoKLRoutines
from fokl_gpy_amd import predictive as pd
from fokl_gpy_amd.embedded import basis_matrix
from oracle import fokl_oracle as O

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 1000)
DRAWS = (1, 15, 16, 17, 63, 64, 65, 1003)
WIDTHS = (1, 5, 128, 129, 300)
QS = (0, 1, 3, 8)
Z_INT = {0: [], 1: [2], 3: [-2, 0, 2], 8: [-4, -3, -2, -1, 1, 2, 3, 4]}


def lds_bytes(nc):
    return 8 * (16 * (-(-nc // 4) * 4) + 16)


def split(block, Q):
    return block[:, :6], block[:, 6:].reshape(block.shape[0], Q, 5)


def check_exact(ctx, S, E, nc, Q, seed=0):
    rng = np.random.default_rng(seed)
    cols = rng.integers(-3, 4, size=(S, nc - 1)).astype(np.float64)
    betas = rng.integers(-3, 4, size=(E, nc)).astype(np.float64)
    y = rng.integers(-20, 21, size=S).astype(np.float64)
    sd, rinv = pd.scales(np.ones(E))
    z = np.array(Z_INT[Q], dtype=np.float64)
    p = (np.arange(Q) + 1.0) / (Q + 1.0)
    slots, X = stage(ctx, cols, y)
    head, per = split(ctx.predictive_rows(slots, betas, sd, rinv, True, p, z, max_passes=0), Q)
    mu = X @ betas.T
    d = mu - mu[:, :1]
    assert np.array_equal(head[:, 0], mu[:, 0]) and np.array_equal(head[:, 1], d.sum(axis=1)), (S, E, nc, Q)
    assert np.array_equal(head[:, 2], (d * d).sum(axis=1)), (S, E, nc, Q)
    assert np.array_equal(head[:, 3], mu.min(axis=1)) and np.array_equal(head[:, 4], mu.max(axis=1)), (S, E, nc, Q)
    assert np.array_equal(per[:, :, 2], mu.min(axis=1)[:, None] + z) and np.array_equal(per[:, :, 3], mu.max(axis=1)[:, None] + z)
    assert np.all(np.isinf(per[:, :, 1])) and np.all(per[:, :, 4] == 0)
    assert np.all(per[:, :, 2] <= per[:, :, 0]) and np.all(per[:, :, 0] <= per[:, :, 3])
    host = pd.predictive_rows_host(X, betas, sd, rinv, y, p, z, max_passes=0)
    assert np.max(np.abs(head[:, 5] - host[:, 5])) <= 1e-14          # erfc on both sides, a few ulp of a value <= 1
    if Q:
        assert np.allclose(per[:, :, 0], split(host, Q)[1][:, :, 0], rtol=1e-14, atol=1e-14)     # the first trial: one sqrt
    rep = ctx.predictive_report()
    assert rep['instance'] == ('pit_quantiles' if Q else 'pit') and rep['with_data'] and rep['with_quantiles'] == bool(Q)
    assert rep['row_tiles'] == -(-S // 16) and 1 <= rep['grid'] <= rep['row_tiles'] and rep['lds_bytes'] == lds_bytes(nc)
    assert rep['quantiles'] == Q and rep['passes_max'] == 0 and rep['passes_sum'] == 0 and rep['unresolved'] == S * Q
    return rep


def test_the_lane_map_a_lane_holds_draws_of_one_row(device_ctx):
    """mu[row][draw] = draw + 1000 row: every minimum, maximum and bracket names its row; were rows and draws (or a lane's
    four draws) placed otherwise, a row would show another row's minimum."""
    S, E = 37, 41
    slots, X = stage(device_ctx, np.arange(S, dtype=np.float64)[:, None], np.zeros(S))
    betas = np.stack([np.arange(E, dtype=np.float64), np.full(E, 1000.0)], axis=1)
    sd, rinv = pd.scales(np.ones(E))
    z = np.array([-2.0, 0.0, 2.0])
    head, per = split(device_ctx.predictive_rows(slots, betas, sd, rinv, False, [0.1, 0.5, 0.9], z, max_passes=0), 3)
    base = 1000.0 * np.arange(S)
    assert np.array_equal(head[:, 0], base) and np.array_equal(head[:, 3], base) and np.array_equal(head[:, 4], base + E - 1)
    assert np.array_equal(head[:, 1], np.full(S, E * (E - 1) / 2.0))
    assert np.array_equal(head[:, 2], np.full(S, (np.arange(E) ** 2.0).sum())) and np.array_equal(head[:, 5], np.zeros(S))
    assert np.array_equal(per[:, :, 2], base[:, None] + z) and np.array_equal(per[:, :, 3], base[:, None] + E - 1 + z)
    assert device_ctx.predictive_report()['instance'] == 'quantiles'


@pytest.mark.parametrize('S', ROWS)
@pytest.mark.parametrize('E', DRAWS)
def test_exact_over_rows_and_draws(device_ctx, S, E):
    check_exact(device_ctx, S, E, nc=5, Q=3, seed=S + E)


@pytest.mark.parametrize('nc', WIDTHS)
@pytest.mark.parametrize('S, E', [(17, 65), (1000, 64)])
def test_exact_over_widths(device_ctx, nc, S, E):
    check_exact(device_ctx, S, E, nc, Q=3, seed=nc)


@pytest.mark.parametrize('Q', QS)
@pytest.mark.parametrize('S, E, nc', [(17, 65, 5), (1000, 1003, 129)])
def test_exact_over_the_number_of_quantiles(device_ctx, Q, S, E, nc):
    check_exact(device_ctx, S, E, nc, Q, seed=Q)


def check_rounded(dev, X, betas, sig, y, p, S):
    """The device block against the statement, with the bounds of the module docstring -> the device's own unresolved."""
    Q = len(p)
    sd, rinv = pd.scales(sig)
    z = np.array([pd.normal_quantile(v) for v in p])
    E = betas.shape[0]
    host = pd.predictive_rows_host(X, betas, sd, rinv, y, p, z)
    first = split(pd.predictive_rows_host(X, betas, sd, rinv, y, p, z, max_passes=0), Q)[1]
    moved = rounding_sensitivity(X, betas, sig, y, p)
    moments = lambda blk: (blk[:, 0] + blk[:, 1] / E, (blk[:, 2] - blk[:, 1] ** 2 / E) / E)
    err_pit = np.abs(dev[:, 5] - host[:, 5]).max()
    err_mean = np.abs(moments(dev)[0] - moments(host)[0]).max()
    err_var = np.abs(moments(dev)[1] - moments(host)[1]).max()
    per = split(dev, Q)[1]
    mu = X @ betas.T
    F = np.stack([pd.mixture_cdf(mu, rinv, per[:, j, 0]) - p[j] for j in range(Q)], axis=1)
    print(f"S {S} E {E} nc {X.shape[1]} Q {Q}: pit {err_pit:.2e} mean {err_mean:.2e} var {err_var:.2e} |F_host(q_dev) - p| "
          f"{np.abs(F).max():.2e} |r_dev - that| {np.abs(per[:, :, 1] - F).max():.2e} against the sensitivity {moved} x 100; "
          f"passes {int(per[:, :, 4].max())} (host {int(split(host, Q)[1][:, :, 4].max())})")
    assert err_pit <= 100.0 * moved[0] and err_mean <= 100.0 * moved[1] and err_var <= 100.0 * moved[2]
    assert np.all(first[:, :, 2] <= per[:, :, 0]) and np.all(per[:, :, 0] <= first[:, :, 3])
    assert np.abs(F).max() <= pd.FTOL + 100.0 * moved[3]
    assert np.abs(per[:, :, 1] - F).max() <= pd.FTOL + 100.0 * moved[3]
    assert np.all(per[:, :, 2] <= per[:, :, 0]) and np.all(per[:, :, 0] <= per[:, :, 3]) and np.all(per[:, :, 4] >= 1)
    return int((np.abs(per[:, :, 1]) > pd.FTOL).sum())


@pytest.mark.parametrize('S, E, nc, p', [(500, 1000, 100, (0.025, 0.5, 0.975)), (1000, 64, 5, (0.025, 0.5, 0.975)),
                                         (17, 1003, 300, (0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999, 0.9)),
                                         (100, 65, 129, (0.1,)), (33, 15, 1, (0.025, 0.5, 0.975))])
def test_rounded_against_the_host_statement(device_ctx, S, E, nc, p):
    cols, betas, y, sig = continuous_case(S, E, nc, S + E + nc)
    slots, X = stage(device_ctx, cols, y)
    sd, rinv = pd.scales(sig)
    z = np.array([pd.normal_quantile(v) for v in p])
    dev = device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
    unresolved = check_rounded(dev, X, betas, sig, y, np.array(p), S)
    rep = device_ctx.predictive_report()
    assert rep['unresolved'] == unresolved and rep['quantiles'] == len(p) and rep['instance'] == 'pit_quantiles'
    assert rep['passes_max'] == int(split(dev, len(p))[1][:, :, 4].max()) and rep['passes_sum'] >= rep['passes_max']
    assert np.array_equal(device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z), dev)    # no atomics: the same bits
    only = device_ctx.predictive_rows(slots, betas, sd, rinv, True, [], [])                      # the PIT alone, from pass 0
    assert only.shape == (S, 6) and np.array_equal(only, dev[:, :6]) and device_ctx.predictive_report()['instance'] == 'pit'
    bare = device_ctx.predictive_rows(slots, betas, sd, rinv, False, p, z)                       # no data: pit is zero
    assert np.array_equal(bare[:, 5], np.zeros(S)) and np.array_equal(bare[:, 6:], dev[:, 6:])


def mixed_tile():
    """Sixteen rows mu[i][d] = c_d + a_i w_d, w_d = +-50: row 7 (a = 1) has two modes 100 apart with sd 0.05, the others
    (a = 0.0005) are unimodal."""
    rng = np.random.default_rng(12)
    E = 200
    a = np.full(16, 0.0005)
    a[7] = 1.0
    betas = np.stack([0.01 * rng.standard_normal(E), np.where(rng.random(E) < 0.3, -50.0, 50.0)], axis=1)
    return a, betas, np.full(E, 0.05 ** 2)


def test_a_hard_row_does_not_change_its_tile_mates(device_ctx):
    a, betas, sig = mixed_tile()
    sd, rinv = pd.scales(sig)
    p = (0.025, 0.5, 0.975)
    z = np.array([pd.normal_quantile(v) for v in p])
    slots, _ = stage(device_ctx, a[:, None], np.zeros(16))
    mixed = device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
    rep_mixed = device_ctx.predictive_report()
    easy = np.arange(16) != 7
    slots, _ = stage(device_ctx, a[easy][:, None], np.zeros(15))
    alone = device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
    rep_alone = device_ctx.predictive_report()
    assert np.array_equal(mixed[easy], alone)                        # bit for bit, in other lanes of another tile
    assert rep_mixed['passes_max'] > rep_alone['passes_max'] and rep_mixed['passes_max'] == split(mixed, 3)[1][7, :, 4].max()
    assert rep_mixed['unresolved'] == rep_alone['unresolved'] == 0


def test_rows_of_a_long_call_equal_a_short_call(device_ctx):
    cols, betas, y, sig = continuous_case(1000, 65, 9, 5)
    sd, rinv = pd.scales(sig)
    p = (0.05, 0.95)
    z = np.array([pd.normal_quantile(v) for v in p])
    slots, _ = stage(device_ctx, cols, y)
    long = device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
    slots, _ = stage(device_ctx, cols[:17], y[:17])
    short = device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
    assert np.array_equal(long[:17], short)
    assert np.array_equal(device_ctx.predictive_rows(slots, betas, sd, rinv, True, p, z), short)


def test_the_report_and_the_timing_slot(device_ctx):
    ctx = device_ctx
    S, E, nc = 100003, 40, 6
    cols, betas, y, sig = continuous_case(S, E, nc, 9)
    sd, rinv = pd.scales(sig)
    p = (0.1, 0.5, 0.9, 0.99, 0.01)
    z = np.array([pd.normal_quantile(v) for v in p])
    slots, _ = stage(ctx, cols, y)
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        dev = ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
        timed = ctx.timing_get(_capi.K_PREDICTIVE)
    finally:
        ctx.timing_enable(False)
    rep = ctx.predictive_report()
    passes = split(dev, 5)[1][:, :, 4]
    tiles = -(-S // 16)
    assert rep['instance'] == 'pit_quantiles' and rep['with_data'] and rep['with_quantiles'] and rep['quantiles'] == 5
    assert rep['row_tiles'] == tiles > rep['grid'] >= 1 and rep['lds_bytes'] == lds_bytes(nc)            # the tile loop went round
    assert rep['passes_max'] == passes.max() and tiles <= rep['passes_sum'] <= tiles * rep['passes_max']
    per_tile = np.pad(passes.max(axis=1), (0, tiles * 16 - S)).reshape(tiles, 16).max(axis=1)
    assert rep['passes_sum'] == per_tile.sum()
    assert rep['unresolved'] == int((np.abs(split(dev, 5)[1][:, :, 1]) > pd.FTOL).sum()) and rep['kernel_ms'] > 0.0
    assert timed['launches'] == 1 and timed['ms'] > 0.0
    assert timed['flops'] == 2.0 * 16 * 8 * E * (tiles + rep['passes_sum'])                              # of the passes that ran


def test_refusals_launch_nothing(device_ctx, monkeypatch):
    ctx = device_ctx
    cols, betas, y, sig = continuous_case(200, 30, 4, 3)
    sd, rinv = pd.scales(sig)
    p = np.array([0.025, 0.975])
    z = np.array([pd.normal_quantile(v) for v in p])
    slots, X = stage(ctx, cols, y)
    before = ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
    ctx.timing_enable(True)
    ctx.timing_reset()

    def refused(match, **kw):
        args = dict(slots=slots, betas=betas, sd=sd, rinv=rinv, with_data=True, p=p, z=z)
        args.update(kw)
        with pytest.raises(_capi.FoklNativeError, match=match) as exc:
            ctx.predictive_rows(**args)
        assert exc.value.code == -2
        assert ctx.predictive_report()['instance'] == 'none' and ctx.predictive_report()['grid'] == 0

    try:
        wide = 1284                                              # 1284 x 16 x 8 + 128 bytes: past the 160 KiB of a compute unit
        refused(f'{wide} columns want {lds_bytes(wide)} bytes of LDS per 16-row tile, a compute unit has 163840',
                slots=np.zeros(wide, dtype=np.int32), betas=np.zeros((30, wide)))
        monkeypatch.setenv('FOKL_PREDICTIVE_FREE_BYTES', str(64 << 20))
        refused(f'{200 * 16 * 8} of results = rows x \\(6 \\+ 5 Q\\) x 8.*the device has {64 << 20} free')
        monkeypatch.delenv('FOKL_PREDICTIVE_FREE_BYTES')
        refused('at most FOKL_PREDICTIVE_MAX_QUANTILES = 8', p=np.linspace(0.1, 0.9, 9), z=np.zeros(9))
        refused(r'strictly inside \(0, 1\)', p=np.array([0.5, 1.0]))
        refused('repeat', p=np.array([0.5, 0.5]))
        refused('max_passes must be >= 0', max_passes=-1)
        refused('ftol and xtol must be finite and >= 0', ftol=-1.0)
        refused('ftol and xtol must be finite and >= 0', xtol=float('nan'))
        refused('neither data nor quantiles', with_data=False, p=[], z=[])
        refused('positive and finite', sd=-sd)
        for bad in (np.nan, -np.inf):                            # draws of a flagged chain, or overflowed ones
            spoiled = betas.copy()
            spoiled[29, 3] = bad
            refused('fokl_predictive_rows: every coefficient must be finite', betas=spoiled)
            refused('fokl_predictive_rows: every coefficient must be finite', betas=spoiled, with_data=False)
        with pytest.raises(_capi.FoklNativeError, match='slot'):
            ctx.predictive_rows(np.array([0, 2, 3, 9999], dtype=np.int32), betas, sd, rinv, True, p, z)
        with pytest.raises(ValueError):
            ctx.predictive_rows(slots, betas[:, :2], sd, rinv, True, p, z)
        with pytest.raises(ValueError):
            ctx.predictive_rows(slots, betas, sd[:-1], rinv, True, p, z)
        assert ctx.timing_get(_capi.K_PREDICTIVE)['launches'] == 0   # nothing was launched
    finally:
        ctx.timing_enable(False)
    assert np.array_equal(ctx.read_slot(2), cols[:, 0]) and np.array_equal(ctx.read_slot(_capi.SLOT_Y), y)
    assert np.array_equal(ctx.predictive_rows(slots, betas, sd, rinv, True, p, z), before)


# ---------------------------------------------------------------------------------------------------------
# predictive on the device against predictive_host, after a fit
# ---------------------------------------------------------------------------------------------------------

def test_predictive_after_a_fit_and_a_resample():
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
            model.predictive()
        post = model.resample(chains=4, draws=64, burnin=20, seed=5)
        assert not post.flagged.any()
        p = (0.025, 0.25, 0.5, 0.75, 0.975)
        res = model.predictive(post, quantiles=p)
        assert model.setnos is None and np.array_equal(np.random.get_state()[1], state)
        host = pd.predictive_host(post.betas, post.sigsqd, model.mtx, model.phis, model.kernel, model.inputs, model.data,
                                  quantiles=p)
        assert sorted(res.keys()) == sorted(host.keys()) and res.rows == n and res.draws == 256
        # the same bounds as for the kernel alone, from the sensitivity of this very case
        X = basis_matrix(model.inputs, model.mtx, model.phis, model.kernel)
        data = np.asarray(model.data, dtype=np.float64).reshape(-1)
        moved = rounding_sensitivity(X, post.betas, post.sigsqd, data, p)
        sd, rinv = pd.scales(post.sigsqd)
        F = np.stack([pd.mixture_cdf(X @ post.betas.T, rinv, res.quantiles[:, j]) - p[j] for j in range(5)], axis=1)
        print(f"pit {np.abs(res.pit - host.pit).max():.2e} mean {np.abs(res.mean - host.mean).max():.2e} var "
              f"{np.abs(res.sd ** 2 - host.sd ** 2).max():.2e} F {np.abs(F).max():.2e} against {moved} x 100; coverage "
              f"{res.coverage}, pit_ks {res.pit_ks:.4f}")
        assert np.abs(res.pit - host.pit).max() <= 100.0 * moved[0] and np.abs(res.mean - host.mean).max() <= 100.0 * moved[1]
        assert np.abs(res.sd ** 2 - host.sd ** 2).max() <= 100.0 * moved[2] + 4.0 * np.finfo(float).eps * host.sd.max() ** 2
        assert np.abs(F).max() <= pd.FTOL + 100.0 * moved[3] and np.abs(res.residual - F).max() <= pd.FTOL + 100.0 * moved[3]
        assert res.unresolved == int((np.abs(res.residual) > pd.FTOL).sum()) == 0
        # the summaries follow from the returned per-row arrays
        assert [(c['lower'], c['upper']) for c in res.coverage] == [(0.025, 0.975), (0.25, 0.75)]
        for k, (lo, hi) in enumerate([(0, 4), (1, 3)]):
            inside = (res.quantiles[:, lo] <= data) & (data <= res.quantiles[:, hi])
            assert np.array_equal(res.inside[:, k], inside) and res.coverage[k]['observed'] == inside.mean()
        assert np.array_equal(np.round(res.pit_hist * n), np.histogram(res.pit, bins=20, range=(0.0, 1.0))[0])
        assert res.pit_ks == pd.pit_ks(res.pit)
        thin = model.predictive(post, draws=np.arange(0, 256, 2), quantiles=())
        assert thin.draws == 128 and thin.quantiles.shape == (n, 0) and 'pit' in thin
        x_new = 0.05 + 0.9 * rng.random((501, 3))
        new = model.predictive(post, inputs=x_new, clean=True)       # new inputs without data: intervals alone
        assert new.rows == 501 and 'pit' not in new and np.all(np.diff(new.quantiles, axis=1) > 0.0) and new.unresolved == 0

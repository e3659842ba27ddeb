"""fokl_infer_inputs (csrc/fokl_infer_device.inc) against infer.sample_host, the statement of the ensemble sampler over unknown
inputs: the target alone, whole chains by their accept flags, the bitwise invariances counter-based numbers give, the native
refusals, and FoKL.infer_inputs after a fit and a resample."""
import warnings

import numpy as np
import pytest

from test_infer_host import KERNEL, MINMAX6, MTX6, PHIS, UNKNOWN6, small_problem
from fokl_gpy_amd import _capi, FoKLRoutines, infer
from fokl_gpy_amd.embedded import basis_matrix
from fokl_gpy_amd.optimize import TermTable, start_points

pytestmark = pytest.mark.gpu

FIELDS = ('mtx_u', 'betas', 'h', 'table', 'lo', 'hi', 'prior_mean', 'prior_prec', 'y', 'P', 'starts')


def on_device(ctx, p, **over):
    q = dict(p, **over)
    return ctx.infer_inputs(*[q[k] for k in FIELDS], q['burnin'], q['draws'], q['thin'], q['jump_every'], q['seed'],
                            draw_ids=q.get('draw_ids'), rows=q.get('rows', True), term_cap=q.get('term_cap', 0))


def on_host(p, **over):
    q = dict(p, **over)
    return infer.sample_host(*[q[k] for k in FIELDS], q['burnin'], q['draws'], q['thin'], q['jump_every'], q['seed'],
                             draw_ids=q.get('draw_ids'), **{k: q[k] for k in ('rows', 'flags') if k in q})


def moved(x, starts):
    """The accept flags [E, iterations, 64] of chains kept at thin = 1 from burn-in 0: an accepted proposal is another point."""
    before = np.concatenate([np.broadcast_to(starts, x[:, :1].shape), x[:, :-1]], axis=1)
    return np.any(x != before, axis=-1)


def follows(dev_x, host_x, starts, at_least):
    """The flag rule: every accept flag of at least ``at_least`` ensembles equals the host's, and where they do the states
    agree to 1e-9.  Returns the ensembles compared."""
    fd, fh = moved(dev_x, starts), moved(host_x, starts)
    same = [e for e in range(dev_x.shape[0]) if np.array_equal(fd[e], fh[e])]
    print('ensembles with equal flags', len(same), 'of', dev_x.shape[0])
    assert len(same) >= at_least
    gap = np.max(np.abs(dev_x[same] - host_x[same]))
    print('largest state difference', gap)
    assert gap <= 1e-9
    return same


# ---------------------------------------------------------------------------------------------------------
# the target only: lp of the starts and of the first proposals
# ---------------------------------------------------------------------------------------------------------

def case_smallest():
    """d = 1, K = 1, T = 1, E = 1: the exponent d - 1 = 0."""
    return infer._prepare([[0.1, 1.0]], [0.01], [[1]], PHIS, [[0.0, 1.0]], KERNEL, [0], None, [0.2], burnin=0, draws=1, thin=1)


def case_mixed():
    """d = 4 of m = 6, K = 7, E = 3: knowns, a four-factor term, terms of knowns only, a prior, narrowed bounds, noise=."""
    rng = np.random.default_rng(5)
    betas = rng.standard_normal((3, MTX6.shape[0] + 1))
    return infer._prepare(betas, None, MTX6, PHIS, MINMAX6, KERNEL, UNKNOWN6, rng.random((7, 2)), rng.standard_normal(7),
                          noise=0.7, prior={'x1': (1.2, 0.5), 3: (14.0, 3.0)}, bounds={'x2': (-0.5, 0.8), 5: (-2.5, -0.5)},
                          burnin=0, draws=1, thin=1)


def case_widest():
    """d = 16 = m, 32 distinct factors, K = 2, E = 2: 160 of the 288 values a walker may keep, the most d = 16 can ask for
    with two orders per input.  The starts are a cloud about the centre: from starts all over a 16-dimensional box every
    jump proposal leaves it and none would be evaluated."""
    rng = np.random.default_rng(6)
    mtx = np.zeros((40, 16), dtype=int)
    for t in range(32):
        mtx[t, t % 16] = 1 + t // 16
    for t in range(32, 40):
        mtx[t, [t % 16, (3 * t + 1) % 16, (5 * t + 2) % 16]] = [1, 2, 1]
    mtx[39, 9] = 2                                                     # a four-factor term
    betas = 0.3 * rng.standard_normal((2, 41))
    cloud = 0.5 + 0.2 * (start_points(64, np.zeros(16), np.ones(16)) - 0.5)
    return infer._prepare(betas, [0.5, 0.8], mtx, PHIS, [[0.0, 1.0]] * 16, KERNEL, list(range(16)), None,
                          rng.standard_normal(2), starts=cloud, burnin=0, draws=1, thin=1)


@pytest.mark.parametrize('case, rows_wanted', [(case_smallest, 3 + 4), (case_mixed, None), (case_widest, 3 * 32 + 64)])
def test_target_against_the_statement(device_ctx, case, rows_wanted):
    p = case()
    for jump_every in (0, 1):                                          # the first proposals: stretch moves, jump moves
        x, lp, sums, accepted, evals = on_device(device_ctx, p, jump_every=jump_every)
        rep = device_ctx.infer_report()
        assert rep['mapping'] == 'walker_per_lane' and rep['launches'] == 1 and rep['grid'] == p['E']
        assert rep['iterations'] == 1 and rep['evaluations'] == evals.sum() and rep['lds_bytes'] == 512 * rep['lds_rows']
        if rows_wanted:
            assert rep['lds_rows'] == rows_wanted
        assert x.shape == (p['E'], 1, 64, p['d']) and np.all((x > p['lo']) & (x < p['hi']))
        w = p['betas'][:, None, :] * p['P'][None, :, :]
        ref, scale = infer.log_target(TermTable(p['mtx_u']), p['table'], x[:, 0], w, p['h'], p['y'], p['prior_mean'],
                                      p['prior_prec'], parts=True)
        err = np.abs(lp[:, 0] - ref) / scale
        print(case.__name__, 'jump_every', jump_every, 'largest |dlp| / scale', err.max(), 'accepted', accepted.sum(axis=(0, 1)))
        assert err.max() <= 1e-11
        hx, hlp, _, h_accepted, h_evals = on_host(p, jump_every=jump_every)
        same = np.any(x != p['starts'], axis=-1) == np.any(hx != p['starts'], axis=-1)       # walkers with the host's flag
        assert same.mean() >= 0.9 and np.max(np.abs(x - hx)[same]) <= 1e-9
        assert np.array_equal(evals, h_evals) and np.all((h_evals > 64) & (h_evals <= 128))  # first proposals were evaluated
        assert np.array_equal(accepted[same[:, 0]], h_accepted[same[:, 0]]) and h_accepted[:, :, 1 if jump_every else 0].sum() > 0


# ---------------------------------------------------------------------------------------------------------
# chains follow the statement; the bitwise invariances
# ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def chains():
    p = infer._prepare(*small_problem(), burnin=0, draws=40, thin=1, jump_every=2, seed=6)
    return p, on_host(p)


def test_chains_follow_the_statement(device_ctx, chains):
    p, host = chains
    x, lp, sums, accepted, evals = on_device(device_ctx, p)
    same = follows(x, host[0], p['starts'], at_least=4)
    assert np.all(accepted[same].sum(axis=1) > 0)                      # stretch and jump moves were both accepted
    assert np.array_equal(accepted[same], host[3][same]) and np.array_equal(evals[same], host[4][same])
    assert np.max(np.abs(lp[same] - host[1][same])) <= 1e-9 * np.max(np.abs(host[1]))
    assert np.allclose(sums[same], host[2][same], rtol=0, atol=1e-8)


def test_an_ensemble_alone_thinning_and_slicing_change_no_bit(device_ctx, chains):
    p, _ = chains
    ctx = device_ctx
    base = on_device(ctx, p)
    rep = ctx.infer_report()
    assert rep['launches'] == 1 and rep['grid'] == 5 and rep['draws_per_launch'] == 5 and rep['kernel_us'] > 0
    again = on_device(ctx, p)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    alone = on_device(ctx, p, betas=p['betas'][3:4], h=p['h'][3:4], draw_ids=p['draw_ids'][3:4])
    assert all(np.array_equal(a[0], b[3]) for a, b in zip(alone, base))
    third = on_device(ctx, p, thin=3)
    assert np.array_equal(third[0], base[0][:, ::3]) and np.array_equal(third[1], base[1][:, ::3])
    assert all(np.array_equal(a, b) for a, b in zip(third[2:], base[2:]))
    none = on_device(ctx, p, rows=False)
    assert none[0] is None and none[1] is None and all(np.array_equal(a, b) for a, b in zip(none[2:], base[2:]))
    per_draw = (2 * 40 + 1) * p['K'] * p['T']                          # term evaluations by a wavefront per draw
    for cap, launches, grid in ((per_draw, 5, 1), (2 * per_draw + 1, 3, 2)):
        sliced = on_device(ctx, p, term_cap=cap)
        rep = ctx.infer_report()
        assert rep['launches'] == launches and rep['grid'] == grid and rep['draws_per_launch'] == grid
        assert all(np.array_equal(a, b) for a, b in zip(sliced, base))


def test_native_refusals_launch_nothing(device_ctx, chains, monkeypatch):
    p, _ = chains
    ctx = device_ctx
    on_device(ctx, p)
    assert ctx.infer_report()['mapping'] == 'walker_per_lane'

    def refused(match, **over):
        with pytest.raises(_capi.FoklNativeError, match=match) as exc:
            on_device(ctx, p, **over)
        assert exc.value.code == -2
        rep = ctx.infer_report()
        assert rep['mapping'] == 'none' and not any(v for k, v in rep.items() if k != 'mapping')

    d17 = np.zeros((p['T'], 17), dtype=np.int32)
    refused('1 to 16', mtx_u=d17, lo=np.zeros(17), hi=np.ones(17), prior_mean=np.zeros(17), prior_prec=np.zeros(17),
            starts=np.full((64, 17), 0.5))
    refused('lo < hi', lo=p['hi'])
    refused('lo < hi', hi=np.array([1.0, np.inf]))
    edge = p['starts'].copy()
    edge[17, 1] = p['hi'][1]
    refused('start 17 is not strictly inside', starts=edge)
    refused('positive and finite', h=np.array([1.0, 1.0, 0.0, 1.0, 1.0]))
    refused('positive and finite', h=np.array([1.0, np.inf, 1.0, 1.0, 1.0]))
    refused('at least 1', y=np.zeros(0), P=np.zeros((0, p['T'] + 1)))
    high = p['mtx_u'].copy()
    high[0, 0] = p['n_basis'] + 1
    refused('outside the coefficient table', mtx_u=high)
    refused('thin >= 1', thin=0)
    refused('thin >= 1', draws=0)
    refused('thin >= 1', burnin=-1)
    refused('thin >= 1', jump_every=-1)
    nan = p['betas'].copy()
    nan[2, 1] = np.nan
    refused('NaN or infinity in betas', betas=nan)
    refused('precision', prior_prec=np.array([-1.0, 0.0]))
    wide = np.zeros((48, 16), dtype=np.int32)                          # 80 distinct factors: 304 values per walker
    for t in range(48):
        wide[t, t % 16] = 1 + t // 16
        wide[t, (t + 1) % 16] = 3 + t // 16
    refused('a wavefront.s LDS holds 288', mtx_u=wide, betas=np.ones((5, 49)), P=np.ones((p['K'], 49)), lo=np.zeros(16),
            hi=np.ones(16), prior_mean=np.zeros(16), prior_prec=np.zeros(16), starts=np.full((64, 16), 0.5))
    monkeypatch.setenv('FOKL_INFER_FREE_BYTES', str(65 << 20))         # 64 MiB are to stay spare: 1 MiB counts as free
    refused('bytes of kept rows', betas=np.tile(p['betas'], (40, 1)), h=np.tile(p['h'], 40), draw_ids=None, draws=400)
    monkeypatch.delenv('FOKL_INFER_FREE_BYTES')
    x = on_device(ctx, p)[0]
    assert ctx.infer_report()['mapping'] == 'walker_per_lane' and np.isfinite(x).all()


# ---------------------------------------------------------------------------------------------------------
# FoKL.infer_inputs after a fit and a resample
# ---------------------------------------------------------------------------------------------------------

def test_infer_inputs_after_a_fit_and_a_resample():
    rng = np.random.default_rng(11)
    n = 4000
    x = rng.random((n, 2))
    y = 2.0 * x[:, 1] + np.sin(3.0 * x[:, 0]) + 0.5 * x[:, 0] * x[:, 1] + 0.05 * rng.standard_normal(n)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = FoKLRoutines.FoKL(kernel=KERNEL, burnin=60, draws=60, UserWarnings=False, ConsoleOutput=False)
        np.random.seed(7)
        model.fit(x, y, clean=True)
        post = model.resample(chains=4, draws=50, burnin=20, seed=5)
        assert not post.flagged.any() and post.betas.shape[0] == 200
        truth, x1 = 0.63, np.array([0.2, 0.5, 0.8])
        low = np.array([float(mm[0]) for mm in model.minmax])
        span = np.array([float(mm[1]) for mm in model.minmax]) - low
        at_truth = (np.stack([x1, np.full(3, truth)], axis=1) - low) / span
        obs = basis_matrix(at_truth, model.mtx, model.phis, KERNEL) @ post.betas.mean(axis=0) + np.array([0.02, -0.03, 0.01])
        state = np.random.get_state()[1].copy()
        kept = {k: np.copy(v) for k, v in vars(model).items() if isinstance(v, np.ndarray)}
        names = sorted(vars(model))
        with pytest.raises(ValueError, match='resample.*noise='):
            model.infer_inputs(unknown=['x2'], known=x1, data=obs, clean=True)
        res = model.infer_inputs(post, unknown=['x2'], known=x1, data=obs, clean=True, burnin=100, draws=100, thin=5, seed=3)
        assert model.setnos is None and np.array_equal(np.random.get_state()[1], state) and sorted(vars(model)) == names
        assert all(np.array_equal(getattr(model, k), v) for k, v in kept.items())
        assert res.x.shape == (200 * 20 * 64, 1) and res.draws == 200 and res.accept.shape == (200, 2)
        print('pooled mean', res.mean, 'interval', res.quantiles, 'acceptance', res.accept.mean(axis=0), 'rhat', res.rhat_max)
        assert res.quantiles[0, 0] < truth < res.quantiles[0, 1] and res.quantiles[0, 1] - res.quantiles[0, 0] < 0.2
        assert np.all(res.accept[:, 0] > 0.2) and np.all(res.evals > 64) and np.isfinite(res.rhat).all()
        pick = np.array([0, 50, 100, 150, 199])
        args = (post.betas, post.sigsqd, model.mtx, model.phis, model.minmax, KERNEL, [1], x1, obs)
        kw = dict(clean=True, burnin=0, draws=40, thin=1, jump_every=4, seed=3, posterior=pick)
        dev = model.infer_inputs(post, unknown=[1], known=x1, data=obs, **kw)
        host = infer.infer_inputs_host(*args, **kw)
        starts = low[1] + span[1] * infer._prepare(*args, **kw)['starts']
        same = follows(dev.x.reshape(5, 40, 64, 1), host.x.reshape(5, 40, 64, 1), starts, at_least=4)
        assert np.array_equal(dev.draw, host.draw) and np.array_equal(dev.evals[same], host.evals[same])
        sub = model.infer_inputs(post, unknown=['x2'], known=x1, data=obs, clean=True, burnin=100, draws=100, thin=5, seed=3,
                                 posterior=pick)
        full = res.x.reshape(200, -1)
        assert np.array_equal(sub.x.reshape(5, -1), full[pick])        # a draw's stream belongs to its row

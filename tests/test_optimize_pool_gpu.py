"""FoKL.optimize_pool / pooloptimum.optimize_pool on the device against from-scratch arithmetic on the host.

Models are built as test_acquire_gpu builds them (``mtx`` directly, Bernoulli kernel, seeded draws around one coefficient
vector).  The device's sums run in another order than numpy's, so a row may differ from the host's where two values tie to
rounding: the device's row must hold a value within tol_d of the host's at that rank, tol_d the forward error bound of two
dot products (test_drawbest_rows_gpu.tolerance), and a Thompson batch is followed along the device's OWN picks.
"""
import numpy as np
import pytest

from test_design_gpu import KERNEL, PHIS, columns, pool_of
from test_acquire_gpu import fitted, NC, DRAWS
from test_drawbest_rows_gpu import tolerance
from fokl_gpy_amd import pooloptimum as po

pytestmark = pytest.mark.gpu


def products(model, pool, betas=None, sense='max'):
    """(F [S, E] in the sense 'max', tol [E])"""
    X = columns(pool, model.mtx)
    betas = model.betas if betas is None else betas
    return (1.0 if sense == 'max' else -1.0) * (X @ betas.T), tolerance(X, betas)


def check_ranks(res, host, F, tol, sign=1.0):
    cols = np.arange(F.shape[1])
    for r in range(res.top):
        rows = res.ranked[r]
        assert np.all(rows >= 0)
        at = F[rows, cols]
        assert np.all(np.abs(sign * res.ranked_value[r] - at) <= tol), r
        assert np.all(at >= sign * host.ranked_value[r] - tol), r
    assert np.array_equal(res.best, res.ranked[0]) and np.array_equal(res.value, res.ranked_value[0])
    for d in cols:
        assert len(set(res.ranked[:, d].tolist())) == res.top


def check_shares(res):
    rows, share, entropy = po.shares(res.best, res.draws)
    assert np.array_equal(res.rows, rows) and np.array_equal(res.share, share) and res.entropy == entropy
    counts = np.bincount(res.best, minlength=res.rows_in_pool)
    assert np.array_equal(res.share, counts[res.rows] / res.draws) and abs(res.share.sum() - 1.0) <= 1e-12
    assert np.all(np.diff(res.share) <= 0) and res.entropy == pytest.approx(-np.sum(share * np.log(share)))
    assert res.no_candidate == 0
    top_rows, top_share, _ = po.shares(res.ranked, res.draws)
    assert np.array_equal(res.rows_top, top_rows) and np.array_equal(res.share_top, top_share) and top_share.max() <= 1.0


def follow_the_batch(res, F, tol, seed):
    """Each pick is within tol of its draw's best row not taken before; the draws are the rule's; the batch is distinct."""
    q = res.picks
    assert np.array_equal(res.draw, po.thompson_draws(res.draws, q, seed))
    for j in range(q):
        d = int(res.draw[j])
        f = F[:, d].copy()
        f[res.index[:j]] = -np.inf
        assert f[res.index[j]] >= f.max() - tol[d], j
        assert res.rank[j] <= j
    assert len(set(res.index.tolist())) == q


@pytest.mark.parametrize('sense', po.SENSES)
@pytest.mark.parametrize('S', (17, 1029))
def test_ranks_and_shares_against_the_host_twin(device_ctx, S, sense):
    model, pool = fitted(device_ctx), pool_of(S, S + 2)
    res = model.optimize_pool(pool=pool, top=3, sense=sense)
    host = po.optimize_pool_host(model.betas, model.mtx, PHIS, KERNEL, pool, top=3, sense=sense)
    F, tol = products(model, pool, sense=sense)
    sign = 1.0 if sense == 'max' else -1.0
    check_ranks(res, host, F, tol, sign)
    check_shares(res)
    assert res.draws == DRAWS and res.rows_in_pool == S and res.ranked.shape == (3, DRAWS) and 'index' not in res
    assert np.array_equal(res.x_best, pool[res.best])
    print(f"S {S} {sense}: {len(res.rows)} rows share the draws, entropy {res.entropy:.4f} nats, rows that differ from the "
          f"host's {int(np.sum(res.ranked != host.ranked))} of {3 * DRAWS}")
    rep = device_ctx.drawbest_report()
    assert rep['instance'] == 'ran' and rep['ranks'] == 3 and rep['launches'] == 6 and rep['lds_bytes'] == 8 * 16 * 32


def test_clean_returns_the_rows_as_passed_and_a_resample_serves_as_post(device_ctx):
    model = fitted(device_ctx)
    model.minmax = [[-1.0, 3.0]] * 4
    raw = -1.0 + 4.0 * pool_of(100, 13)
    res = model.optimize_pool(pool=raw, clean=True, picks=3, seed=2)
    same = model.optimize_pool(pool=pool_of(100, 13), picks=3, seed=2)
    assert np.array_equal(res.best, same.best) and np.array_equal(res.x_best, raw[res.best])
    assert np.array_equal(res.index, same.index) and np.array_equal(res.x, raw[res.index])
    assert np.allclose(res.x_normalised, same.x_best, rtol=0.0, atol=1e-15)
    assert np.allclose(res.x_batch_normalised, same.x, rtol=0.0, atol=1e-15)
    post = dict(betas=np.concatenate([model.betas[:10], np.full((1, NC), np.nan)]), sigsqd=None)
    with pytest.raises(ValueError, match=r"1 of the 11 draws are NaN or infinite \(the rows of a resample's flagged chains"):
        model.optimize_pool(post, pool=pool_of(100, 13))
    kept = model.optimize_pool(post, pool=pool_of(100, 13), draws=np.arange(10))
    assert kept.draws == 10 and np.array_equal(kept.best, same.best[:10])
    last = model.optimize_pool(pool=pool_of(100, 13), draws=40)
    assert last.draws == 40 and np.array_equal(last.best, same.best[-40:])


def test_thompson_batch_with_and_without_the_second_call(device_ctx):
    model, pool = fitted(device_ctx), pool_of(1029, 21)
    F, tol = products(model, pool)
    plain = model.optimize_pool(pool=pool)
    seed = next(s for s in range(50) if len(set(plain.best[po.thompson_draws(DRAWS, 5, s)].tolist())) == 5)
    res = model.optimize_pool(pool=pool, picks=5, seed=seed)
    assert not res.second_call and res.rank.tolist() == [0] * 5 and np.array_equal(res.index, plain.best[res.draw])
    assert np.array_equal(res.x, pool[res.index]) and np.array_equal(res.best, plain.best)
    follow_the_batch(res, F, tol, seed)

    same = np.repeat(model.betas[:1], 40, axis=0)                 # every draw agrees: the ranks in turn
    res = po.optimize_pool(same, model.mtx, PHIS, KERNEL, pool, picks=5, seed=1, device=model._backend())
    F, tol = products(model, pool, same)
    assert res.second_call and res.rank.tolist() == [0, 1, 2, 3, 4] and res.entropy == 0.0
    follow_the_batch(res, F, tol, 1)
    rep = device_ctx.drawbest_report()                           # the second call: the batch's distinct draws, 5 deep
    assert rep['ranks'] == 5 and rep['launches'] == 10
    host = po.optimize_pool_host(same, model.mtx, PHIS, KERNEL, pool, picks=5, seed=1)
    assert host.second_call and np.array_equal(host.draw, res.draw)
    assert np.all(F[res.index, res.draw] >= F[host.index, host.draw] - tol[res.draw])


def test_excluding_the_winners_changes_every_best(device_ctx):
    model, pool = fitted(device_ctx), pool_of(200, 31)
    first = model.optimize_pool(pool=pool)
    second = model.optimize_pool(pool=pool, exclude=first.rows)
    assert not set(second.best.tolist()) & set(first.rows.tolist()) and np.all(second.best != first.best)
    assert np.all(second.value <= first.value) and second.open_rows == 200 - len(first.rows)
    F, tol = products(model, pool)
    F[first.rows] = -np.inf
    assert np.all(F[second.best, np.arange(DRAWS)] >= F.max(axis=0) - tol)
    check_shares(second)

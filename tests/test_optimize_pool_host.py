"""pooloptimum.ranks_host / thompson_host / optimize_pool_host, the numpy statement of "every draw's best rows of a pool",
against independent arithmetic (no device).

References are formed from scratch: the whole f matrix sorted per draw by np.lexsort, the closed form of the probability
of being optimal between two rows under Gaussian draws, and a from-scratch walk of the Thompson rule.
"""
import itertools
import math

import numpy as np
import pytest

from test_acquire_host import KERNEL, PHIS, MTX, continuous_case, integer_case, model_case, columns
from fokl_gpy_amd import FoKLRoutines
from fokl_gpy_amd import pooloptimum as po


def brute_ranks(X, betas, ranks, mask=None):
    """(index [ranks, E], value [ranks, E]) from the whole f = X betas': per draw np.lexsort((arange, -f)) over the
    candidates (unmasked, not NaN).  f is stored whole, its products formed 16 rows at a time as the statement forms them
    (BLAS rounds a product of another shape differently; what is under test is the order)."""
    BT = np.ascontiguousarray(betas.T)
    with np.errstate(invalid='ignore', over='ignore'):
        F = np.concatenate([X[t:t + 16] @ BT for t in range(0, X.shape[0], 16)])
    S, E = F.shape
    index = np.full((ranks, E), -1, dtype=np.int64)
    value = np.full((ranks, E), -np.inf)
    for d in range(E):
        ok = ~np.isnan(F[:, d])
        if mask is not None:
            ok &= np.asarray(mask) == 0
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, -F[cand, d]))][:ranks]
        index[:order.shape[0], d], value[:order.shape[0], d] = order, F[order, d]
    return index, value


def inf_case(seed=3, S=37, nc=5, E=24):
    """``integer_case`` with +inf in a few rows of column 2; the draws' coefficient of that column is 0 in some draws (the
    rows' f is NaN and never ranks), positive in some (+inf: ranks first) and negative in others (-inf: ranks last).
    (Shared with the GPU tests.)"""
    X, betas, _ = integer_case(seed, S, nc, E)
    X[[1, 8, 20], 2] = np.inf
    betas[:, 2] = np.resize([0.0, 1.0, -2.0], E)
    return X, betas


def host(betas, pool, **kw):
    return po.optimize_pool_host(betas, MTX, PHIS, KERNEL, pool, **kw)


@pytest.mark.parametrize('case', (integer_case, continuous_case), ids=('integer', 'continuous'))
@pytest.mark.parametrize('S', (1, 15, 16, 17, 1029))
@pytest.mark.parametrize('ranks', (1, 6))
def test_ranks_against_a_full_sort_per_draw(case, S, ranks):
    X, betas, _ = case(S + ranks, S, 7, 40)
    got = po.ranks_host(X, betas, ranks)
    index, value = brute_ranks(X, betas, ranks)
    assert got['index'].dtype == np.int64 and np.array_equal(got['index'], index)
    assert got['value'].tobytes() == value.tobytes()
    if case is integer_case and S > 16:                          # the data is full of ties: the lowest index carries it
        assert np.any(np.sum(X @ betas.T == value[0], axis=0) > 1)


def test_one_row_and_three_ranks_runs_out_after_the_first():
    X, betas, _ = integer_case(0, 1, 4, 9)
    got = po.ranks_host(X, betas, 3)
    assert np.array_equal(got['index'], [[0] * 9, [-1] * 9, [-1] * 9])
    assert np.array_equal(got['value'][0], (X @ betas.T)[0]) and np.all(got['value'][1:] == -np.inf)


def test_a_mask_that_removes_a_draws_best_promotes_the_next():
    X, betas, _ = integer_case(5, 33, 6, 20)
    free = po.ranks_host(X, betas, 2)
    mask = np.zeros(33, dtype=np.uint8)
    mask[np.unique(free['index'][0, :5])] = 1                    # the best rows of the first five draws
    got = po.ranks_host(X, betas, 6, mask)
    index, value = brute_ranks(X, betas, 6, mask)
    assert np.array_equal(got['index'], index) and got['value'].tobytes() == value.tobytes()
    assert not np.any(mask[got['index']]) and np.all(got['index'][0, :5] != free['index'][0, :5])


def test_nan_never_ranks_and_infinities_compare_as_numbers():
    X, betas = inf_case()
    got = po.ranks_host(X, betas, 37)
    index, value = brute_ranks(X, betas, 37)
    assert np.array_equal(got['index'], index) and got['value'].tobytes() == value.tobytes()
    zero, plus, minus = got['index'][:, 0], got['index'][:, 1], got['index'][:, 2]
    assert np.all(zero[34:] == -1) and not set(zero.tolist()) & {1, 8, 20}         # NaN: three candidates fewer
    assert plus[:3].tolist() == [1, 8, 20] and np.all(got['value'][:3, 1] == np.inf)
    assert minus[34:].tolist() == [1, 8, 20] and np.all(got['value'][34:, 2] == -np.inf)


def test_sense_min_is_max_on_negated_betas_with_the_values_flipped():
    _, pool, betas = model_case(2)
    a, b = host(betas, pool, sense='min', top=3, picks=4, seed=5), host(-betas, pool, sense='max', top=3, picks=4, seed=5)
    assert np.array_equal(a.ranked, b.ranked) and a.ranked_value.tobytes() == (-b.ranked_value).tobytes()
    assert a.value.tobytes() == (-b.value).tobytes() and np.array_equal(a.index, b.index)
    F = columns(pool) @ betas.T
    assert np.array_equal(a.best, F.argmin(axis=0)) and np.array_equal(a.value, F.min(axis=0))


@pytest.mark.parametrize('mu', (0.0, 0.5, 2.0))
def test_share_of_two_rows_under_gaussian_draws_is_the_normal_cdf(mu):
    E = 4000
    X = np.array([[1.0, -1.0], [1.0, 1.0]])
    betas = np.random.default_rng([7, int(10 * mu)]).standard_normal((E, 2)) + np.array([0.0, mu])
    best = po.ranks_host(X, betas)['index'][0]                   # row 1 wins where beta_1 > 0: probability Phi(mu)
    rows, share, entropy = po.shares(best, E)
    p = 0.5 * (1.0 + math.erf(mu / math.sqrt(2.0)))
    got = float(share[rows == 1][0])
    assert abs(got - p) <= 4.0 * math.sqrt(p * (1.0 - p) / E)
    assert share.sum() == pytest.approx(1.0, abs=1e-15) and np.all(np.diff(share) <= 0)
    assert entropy == pytest.approx(-sum(s * math.log(s) for s in share), abs=1e-15)


def test_result_fields_follow_from_the_ranks():
    _, pool, betas = model_case(3)
    res = host(betas, pool, top=4)
    index, value = brute_ranks(columns(pool), betas, 4)
    assert np.array_equal(res.ranked, index) and np.array_equal(res.ranked_value, value)
    assert np.array_equal(res.best, index[0]) and np.array_equal(res.value, value[0])
    assert np.array_equal(res.x_best, pool[index[0]]) and res.no_candidate == 0 and 'index' not in res
    counts = np.bincount(index[0], minlength=40)
    assert np.array_equal(res.rows, np.lexsort((np.arange(40), -counts))[:np.count_nonzero(counts)])
    assert np.array_equal(res.share, counts[res.rows] / 30.0) and res.share.sum() == pytest.approx(1.0)
    assert res.entropy == pytest.approx(-np.sum(res.share * np.log(res.share)))
    counts = np.bincount(index.reshape(-1), minlength=40)
    assert np.array_equal(res.share_top, counts[res.rows_top] / 30.0) and res.share_top.max() <= 1.0
    assert res.share_top.sum() == pytest.approx(4.0)
    one = host(betas[0], pool)                                   # one coefficient vector: one draw
    assert one.draws == 1 and one.share.tolist() == [1.0] and one.entropy == 0.0
    cut = host(betas, pool, exclude=res.rows)
    assert not set(cut.best.tolist()) & set(res.rows.tolist()) and cut.open_rows == 40 - len(res.rows)


def walk_thompson(F, mask, picks, seed):
    """The rule from scratch on the whole f: (index, draw, rank) with rank counted among the draw's candidates."""
    E = F.shape[1]
    perm = np.random.default_rng(seed).permutation(E)
    index, draw, rank, taken = [], [], [], []
    for j in range(picks):
        d = int(perm[j % E])
        cand = np.flatnonzero((mask == 0) & ~np.isnan(F[:, d]))
        order = cand[np.lexsort((cand, -F[cand, d]))]
        s = next(int(s) for s in order if s not in taken)
        index.append(s), draw.append(d), rank.append(int(np.flatnonzero(order == s)[0])), taken.append(s)
    return np.array(index), np.array(draw), np.array(rank)


@pytest.mark.parametrize('picks, E', ((5, 30), (12, 5)), ids=('fewer_than_draws', 'wraps'))
def test_thompson_batch_is_each_draws_best_untaken_row(picks, E):
    _, pool, betas = model_case(6, E=E)
    np.random.seed(11)
    state = np.random.get_state()[1].copy()
    res = host(betas, pool, picks=picks, seed=3, exclude=[0, 4])
    assert np.array_equal(np.random.get_state()[1], state)
    mask = np.zeros(40, dtype=np.uint8)
    mask[[0, 4]] = 1
    index, draw, rank = walk_thompson(columns(pool) @ betas.T, mask, picks, 3)
    assert np.array_equal(res.index, index) and np.array_equal(res.draw, draw) and np.array_equal(res.rank, rank)
    assert len(set(res.index.tolist())) == picks and np.array_equal(res.x, pool[res.index])
    assert res.second_call == bool(np.any(rank > 0)) or picks > E
    if picks > E:
        assert res.second_call and np.array_equal(res.draw[E:2 * E], res.draw[:E])
    again, other = host(betas, pool, picks=picks, seed=3, exclude=[0, 4]), host(betas, pool, picks=picks, seed=4, exclude=[0, 4])
    assert np.array_equal(again.index, res.index) and np.array_equal(again.draw, res.draw)
    assert not np.array_equal(other.draw, res.draw)


def test_thompson_over_draws_that_agree_takes_the_ranks_in_turn():
    _, pool, betas = model_case(8)
    same = np.repeat(betas[:1], 30, axis=0)
    res = host(same, pool, picks=6)
    order = np.lexsort((np.arange(40), -(columns(pool) @ betas[0])))
    assert res.second_call and res.rank.tolist() == [0, 1, 2, 3, 4, 5] and np.array_equal(res.index, order[:6])
    assert res.entropy == 0.0 and res.share.tolist() == [1.0]
    apart = host(betas, pool, picks=2, seed=1)                    # two draws with different best rows: no second call
    if apart.best[apart.draw[0]] != apart.best[apart.draw[1]]:
        assert not apart.second_call and apart.rank.tolist() == [0, 0]


def test_thompson_host_takes_an_array_of_ranked_rows():
    ranked = np.array([[3, 3, 5], [1, 2, 3], [-1, 0, 4]])
    got = po.thompson_host(ranked, 3, 5, seed=0)
    draw = np.random.default_rng(0).permutation(3)[np.arange(5) % 3]
    assert np.array_equal(got['draw'], draw)
    taken = []
    for j, d in enumerate(draw):
        have = [int(s) for s in ranked[:, d] if s >= 0]           # a draw's rows end at its first -1
        left = [(r, s) for r, s in enumerate(have) if s not in taken]
        assert (got['rank'][j], got['index'][j]) == (left[0] if left else (-1, -1))
        taken += [left[0][1]] if left else []


def test_refusals_name_their_limit(monkeypatch):
    _, pool, betas = model_case(5)
    with pytest.raises(ValueError, match='call fit first'):
        po.optimize_pool_host(betas, None, PHIS, KERNEL, pool)
    with pytest.raises(ValueError, match=r'optimize_pool needs betas \[draws, terms \+ 1\]'):
        host(None, pool)
    with pytest.raises(ValueError, match=r'pool \[S, M\] is needed'):
        host(betas, None)
    with pytest.raises(ValueError, match='the pool has 3 columns, the interaction matrix has 2'):
        host(betas, np.zeros((5, 3)))
    with pytest.raises(ValueError, match='betas have 5 columns, the interaction matrix wants 6'):
        host(betas[:, :5], pool)
    rows = pool.copy()
    rows[7, 1] = np.nan
    with pytest.raises(ValueError, match=r'1 of the 40 pool rows are NaN or infinite \(the first is row 7\)'):
        host(betas, rows)
    with pytest.raises(ValueError, match=r'they must lie in \[0, 1\]'):
        po.optimize_pool_host(np.zeros((2, 1)), np.zeros((0, 2), dtype=int), PHIS, 'Cubic Splines', pool + 0.5)
    for top in (0, 65, 1.5):
        with pytest.raises(ValueError, match=r'top must be an integer in 1..64'):
            host(betas, pool, top=top)
    for picks in (-1, 65):
        with pytest.raises(ValueError, match=r'picks must be an integer in 0..64'):
            host(betas, pool, picks=picks)
    with pytest.raises(ValueError, match=r'39 picks from 38 open rows \(a pool of 40, 2 excluded\): at most 38'):
        host(betas, pool, picks=39, exclude=[3, 3, 9])
    for exclude in ([40], [-1], [0.5]):
        with pytest.raises(ValueError, match=r'exclude must hold integer rows of the pool, 0..39'):
            host(betas, pool, exclude=exclude)
    with pytest.raises(ValueError, match='exclude names every one of the 40 pool rows'):
        host(betas, pool, exclude=np.arange(40))
    with pytest.raises(ValueError, match=r"sense must be one of \('max', 'min'\)"):
        host(betas, pool, sense='up')
    holed = betas.copy()
    holed[[2, 9]] = np.nan
    with pytest.raises(ValueError, match=r"2 of the 30 draws are NaN or infinite \(the rows of a resample's flagged chains"):
        host(holed, pool)
    assert host(holed, pool, draws=np.flatnonzero(np.isfinite(holed).all(axis=1))).draws == 28
    with pytest.raises(ValueError, match=r'draws must be None \(all\), an integer in 1..30'):
        host(betas, pool, draws=31)
    with pytest.raises(ValueError, match='draws as an array must hold at least one integer index into the 30 rows'):
        host(betas, pool, draws=np.array([30]))
    wide = np.array([r for r in itertools.product(range(11), repeat=3) if any(r)][:po.MAX_COLUMNS])
    with pytest.raises(ValueError, match=r'1281 columns \(terms \+ 1\), optimize_pool takes at most 1280 .*160 KiB'):
        po.optimize_pool_host(np.zeros((2, 1281)), wide, PHIS, KERNEL, np.zeros((3, 3)))
    monkeypatch.setenv('FOKL_ACQUIRE_FREE_BYTES', str(64 << 20))
    with pytest.raises(ValueError, match='64 MiB to spare, FOKL_ACQUIRE_FREE_BYTES counts 67108864 as free'):
        host(betas, pool)
    monkeypatch.delenv('FOKL_ACQUIRE_FREE_BYTES')
    model = FoKLRoutines.FoKL(kernel=KERNEL, UserWarnings=False, ConsoleOutput=False)
    with pytest.raises(ValueError, match='optimize_pool needs a fitted model: call fit first'):
        model.optimize_pool(pool=pool)
    model.mtx, model.betas = MTX, betas
    with pytest.raises(ValueError, match="optimize_pool takes a resample's result OR betas=, not both"):
        model.optimize_pool(dict(betas=betas), pool=pool, betas=betas)
    with pytest.raises(ValueError, match='this resample kept no rows'):
        model.optimize_pool(dict(betas=None), pool=pool)
    with pytest.raises(ValueError, match='needs what resample returned'):
        model.optimize_pool(3.0, pool=pool)

"""design.design_host, the numpy statement of the greedy optimal design, against independent arithmetic (no device).

Every reference here is formed from scratch (``slogdet`` / ``inv`` of A0 + X_D' X_D, exhaustive enumeration), never by the
downdates the statement itself uses.  The 1e-10 bounds are those of a 6-column model whose A0 has a condition number of a
few hundred: rounding (1e-16) times the condition number times the 30 picks stays below 1e-12.
"""
import itertools
import math

import numpy as np
import pytest

from fokl_gpy_amd import FoKLRoutines, getKernels
from fokl_gpy_amd import design as dg
from fokl_gpy_amd.embedded import basis_matrix

KERNEL = 'Bernoulli Polynomials'
PHIS = getKernels.bernoulli()
MTX = np.array([[1, 0], [0, 1], [2, 0], [1, 1], [0, 2]])             # 6 columns with the intercept
INV_TAU = 0.5


def case(S=40, n=60, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((n, 2)), rng.random((S, 2))


def columns(x, mtx=MTX):
    return basis_matrix(np.asarray(x, dtype=np.float64), mtx, PHIS, KERNEL)


def a0_of(train, mtx=MTX, inv_tau=INV_TAU):
    X = columns(train, mtx)
    return X.T @ X + inv_tau * np.eye(X.shape[1])


def host(train, pool, **kw):
    kw.setdefault('inv_tausqd', INV_TAU)
    return dg.design_host(MTX, PHIS, KERNEL, train, pool, **kw)


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_logdet_gain_is_the_growth_of_log_det(criterion):
    train, pool = case()
    res = host(train, pool, picks=12, criterion=criterion)
    A0, X = a0_of(train), columns(pool)
    base = np.linalg.slogdet(A0)[1]
    for k in range(12):
        XD = X[res.index[:k + 1]]
        assert abs(np.linalg.slogdet(A0 + XD.T @ XD)[1] - base - res.logdet_gain[k]) <= 1e-10, k
    assert np.array_equal(res.x, pool[res.index]) and np.array_equal(res.x_basis, X[res.index])


def test_ivr_target_variance_from_scratch_and_its_differences():
    train, pool = case(seed=1)
    target = np.random.default_rng(5).random((33, 2))
    for tgt, Xt in ((None, columns(train)), (target, columns(target))):
        res = host(train, pool, picks=10, criterion='ivr', target=tgt, sigsqd_mean=0.37)
        A0, X = a0_of(train), columns(pool)
        assert res.target_var.shape == (11,) and res.sigsqd_mean == 0.37
        for k in range(11):
            XD = X[res.index[:k]]
            Ck = np.linalg.inv(A0 + XD.T @ XD)
            scratch = 0.37 * np.mean(np.einsum('si,ij,sj->s', Xt, Ck, Xt))
            assert abs(res.target_var[k] - scratch) <= 1e-10 * scratch, k
        assert np.allclose(res.target_var[:-1] - res.target_var[1:], 0.37 * res.gain, rtol=0, atol=1e-12 * res.target_var[0])
        assert np.all(res.gain > 0.0)
    assert host(train, pool, picks=3).target_var is None


def test_first_pick_is_the_exhaustive_best_and_greedy_meets_the_submodularity_bound():
    train, pool = case(S=10, seed=2)
    res = host(train, pool, picks=3)
    A0, X = a0_of(train), columns(pool)
    base = np.linalg.slogdet(A0)[1]
    single = [np.linalg.slogdet(A0 + np.outer(x, x))[1] - base for x in X]
    assert res.index[0] == int(np.argmax(single))
    subsets = list(itertools.combinations(range(10), 3))
    assert len(subsets) == 120
    best = max(np.linalg.slogdet(A0 + X[list(s)].T @ X[list(s)])[1] - base for s in subsets)
    assert res.logdet_gain[2] >= (1.0 - 1.0 / math.e) * best
    assert res.logdet_gain[2] <= best + 1e-12
    # 'ivr': the first pick is the row whose measurement lowers the target's mean variance most, found from scratch
    ivr = host(train, pool, picks=1, criterion='ivr')
    Xt = columns(train)
    after = [np.mean(np.einsum('si,ij,sj->s', Xt, np.linalg.inv(A0 + np.outer(x, x)), Xt)) for x in X]
    assert ivr.index[0] == int(np.argmin(after))


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_refresh_every_pick_and_never_agree(criterion):
    train, pool = case()
    a = host(train, pool, picks=30, criterion=criterion, refresh_every=1)
    b = host(train, pool, picks=30, criterion=criterion, refresh_every=0)
    assert np.array_equal(a.index, b.index)
    assert np.allclose(a.gain, b.gain, rtol=1e-10, atol=0.0)
    assert np.allclose(a.logdet_gain, b.logdet_gain, rtol=0.0, atol=1e-10)


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_ties_go_to_the_lowest_index(criterion):
    train, pool = case(seed=3)
    first = int(host(train, pool, picks=1, criterion=criterion).index[0])
    pool = np.concatenate([pool, pool[first:first + 1]])             # row 40 = row `first`, exactly
    res = host(train, pool, picks=41, criterion=criterion)
    assert res.index[0] == first and 40 in res.index[1:]             # the copy stays available and is taken later
    assert sorted(res.index.tolist()) == list(range(41))
    rep = host(train, pool, picks=60, criterion=criterion, replicates=True)
    assert rep.index[0] == first
    assert len(set(rep.index.tolist())) < 60                         # rows come more than once
    # a prior so weak that repeating the best row beats every other row
    twice = dg.design_host(np.zeros((0, 2), dtype=int), PHIS, KERNEL, train[:1], pool, picks=3, replicates=True, inv_tausqd=1e-3)
    assert np.array_equal(twice.index, [0, 0, 0])                    # an intercept alone: every row ties, row 0 every time


def test_nothing_random_is_touched_and_the_same_call_gives_the_same_bits():
    train, pool = case()
    np.random.seed(11)
    state = np.random.get_state()[1].copy()
    a = host(train, pool, picks=9, criterion='ivr', keep='variance')
    b = host(train, pool, picks=9, criterion='ivr', keep='variance')
    assert np.array_equal(np.random.get_state()[1], state)
    for name in ('index', 'gain', 'logdet_gain', 'target_var', 'variance'):
        assert a[name].tobytes() == b[name].tobytes()
    XD = columns(pool)[a.index]
    Ck = np.linalg.inv(a0_of(train) + XD.T @ XD)
    assert np.allclose(a.variance, np.einsum('si,ij,sj->s', columns(pool), Ck, columns(pool)), rtol=1e-10, atol=0.0)


def integer_case(S, nc, seed=0):
    """(X [S, nc], C0, CMC0 [nc, nc]) as int64: X = [1 | integers in -3..3], C0 = B'B + I with B 3 x nc from {-1, 0, 1},
    CMC0 = D'D + 2 I with D 2 x nc from {-1, 0, 1}.  Symmetric positive definite, and every sum that ``select_host`` or the
    kernels form before the first division is an integer below 2^53: exact in float64 whatever its order.  (Shared with
    tests/test_design_select_gpu.py.)"""
    rng = np.random.default_rng([S, nc, seed])
    X = np.concatenate([np.ones((S, 1), dtype=np.int64), rng.integers(-3, 4, size=(S, nc - 1))], axis=1)
    B, D = rng.integers(-1, 2, size=(3, nc)), rng.integers(-1, 2, size=(2, nc))
    eye = np.eye(nc, dtype=np.int64)
    return X, B.T @ B + eye, D.T @ D + 2 * eye


def exact_first_pick(X, C0, CMC0):
    """The first pick and the first downdate in int64 up to the one division each value needs:
    -> (index, gain, v*, v [S], w [S] or None), float64."""
    ivr = CMC0 is not None
    f = lambda a: np.asarray(a, dtype=np.int64).astype(np.float64)
    v0 = np.einsum('sj,sj->s', X @ C0, X)
    w0 = np.einsum('sj,sj->s', X @ CMC0, X) if ivr else None
    crit = f(w0) / (1.0 + f(v0)) if ivr else f(v0)             # one correctly rounded division
    i = int(np.argmax(crit))                                     # the first of the largest
    x = X[i]
    u = C0 @ x
    vstar = int(x @ u)
    p = X @ u
    assert int(np.max(np.abs(p))) ** 2 < 2 ** 53 and int(v0.max()) < 2 ** 53
    d = float(1 + vstar)
    v = f(v0) - f(p * p) / d
    w = None
    if ivr:
        a = CMC0 @ x
        wstar, q = int(x @ a), X @ a
        assert max(int(w0.max()), 2 * int(np.max(np.abs(p * q))), wstar) < 2 ** 53
        w = f(w0) - 2.0 * f(p) * f(q) / d + f(p) * f(p) * float(wstar) / (d * d)
    return i, crit[i], float(vstar), v, w


EXACT_SHAPES = [(17, 1), (1029, 17), (33, 513), (1029, 768)]


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('S, nc', EXACT_SHAPES)
def test_select_host_first_pick_and_downdate_are_the_integer_arithmetic_bit_for_bit(S, nc, criterion):
    """On integer data the statement's first pick and first downdate are one rounding away from int64 arithmetic, and that
    rounding is a division both sides do alike: equal as bits, not to a tolerance."""
    X, C0, CMC0 = integer_case(S, nc)
    if criterion == 'variance':
        CMC0 = None
    i, gain, vstar, v, w = exact_first_pick(X, C0, CMC0)
    Xf = X.astype(np.float64)
    res = dg.select_host(Xf, C0, CMC0, picks=1, keep=True)
    assert res['index'][0] == i
    assert res['gain'].tobytes() == np.array([gain]).tobytes() and res['vstar'].tobytes() == np.array([vstar]).tobytes()
    assert np.array_equal(res['x'][0], Xf[i])
    assert res['v'].tobytes() == v.tobytes()
    assert (res['w'] is None) if w is None else (res['w'].tobytes() == w.tobytes())
    # the second pick is the first argmax of the criterion formed from those bit-exact v and w, the first pick masked
    crit = w / (1.0 + v) if criterion == 'ivr' else v.copy()
    crit[i] = -np.inf
    two = dg.select_host(Xf, C0, CMC0, picks=2)
    assert two['index'][0] == i and two['index'][1] == int(np.argmax(crit))
    assert two['gain'].tobytes() == np.array([gain, crit.max()]).tobytes()


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('refresh_every', (0, 5))
def test_select_host_nan_rows_never_win_and_the_empty_pick_is_minus_one(criterion, refresh_every):
    X, C0, CMC0 = integer_case(40, 17)
    Xf = X.astype(np.float64)
    Xf[[3, 20, 35], 5] = np.nan
    res = dg.select_host(Xf, C0, CMC0 if criterion == 'ivr' else None, picks=40, refresh_every=refresh_every, keep=True)
    finite = sorted(set(range(40)) - {3, 20, 35})
    assert sorted(res['index'][:37].tolist()) == finite
    assert np.all(res['index'][37:] == -1) and np.all(res['gain'][37:] == -np.inf)
    assert np.array_equal(res['vstar'][37:], np.zeros(3)) and not res['x'][37:].any()
    assert np.all(np.isfinite(res['gain'][:37])) and np.array_equal(np.flatnonzero(np.isnan(res['v'])), [3, 20, 35])
    # a NaN in one row changes no other row's exact arithmetic: the first pick is the finite rows' own
    i, gain, vstar, _, _ = exact_first_pick(X[finite], C0, CMC0 if criterion == 'ivr' else None)
    assert res['index'][0] == finite[i] and res['gain'][0] == gain and res['vstar'][0] == vstar


def wide_mtx(terms):
    rows = [r for r in itertools.product(range(10), repeat=3) if any(r)]
    return np.array(rows[:terms])


def test_refusals(monkeypatch):
    train, pool = case()
    with pytest.raises(ValueError, match='picks must be an integer >= 1'):
        host(train, pool, picks=0)
    with pytest.raises(ValueError, match='41 picks from a pool of 40 rows.*replicates'):
        host(train, pool, picks=41)
    assert host(train, pool, picks=41, replicates=True).index.shape == (41,)
    bad = pool.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match='1 of the 40 pool rows are NaN or infinite.*row 7'):
        host(train, bad, picks=2)
    train3 = np.random.default_rng(0).random((5, 3))
    with pytest.raises(ValueError, match='769 columns.*at most 768'):
        dg.design_host(wide_mtx(768), PHIS, KERNEL, train3, train3, picks=1, inv_tausqd=1.0)
    monkeypatch.setenv('FOKL_DESIGN_FREE_BYTES', str(1 << 20))
    with pytest.raises(ValueError, match='FOKL_DESIGN_FREE_BYTES'):
        host(train, pool, picks=2)
    monkeypatch.delenv('FOKL_DESIGN_FREE_BYTES')
    with pytest.raises(ValueError, match="'ivr' needs a target population with at least one row"):
        host(train, pool, picks=2, criterion='ivr', target=np.zeros((0, 2)))
    with pytest.raises(ValueError, match='resample.*tausqd='):
        dg.design_host(MTX, PHIS, KERNEL, train, pool, picks=2)
    with pytest.raises(ValueError, match='criterion must be one of'):
        host(train, pool, picks=2, criterion='entropy')
    with pytest.raises(ValueError, match='refresh_every'):
        host(train, pool, picks=2, refresh_every=-1)


def test_the_class_method_refuses_before_it_touches_a_device():
    train, pool = case()
    model = FoKLRoutines.FoKL(kernel=KERNEL, UserWarnings=False, ConsoleOutput=False)
    with pytest.raises(ValueError, match='fitted model: call fit first'):
        model.design(pool=pool, tausqd=2.0)
    model.betas, model.mtx, model.inputs = np.zeros((10, 6)), MTX, train
    with pytest.raises(ValueError, match='resample.*tausqd='):
        model.design(pool=pool)
    with pytest.raises(ValueError, match='resample'):
        model.design(dict(betas=np.zeros((10, 6))), pool=pool)
    with pytest.raises(ValueError, match='positive number'):
        model.design(pool=pool, tausqd=-1.0)

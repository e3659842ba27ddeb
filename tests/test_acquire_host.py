"""acquire.acquire_host / acquire.select_host, the numpy statement of the batch acquisition, against independent arithmetic
(no device).

References are formed from scratch: the joint value of a batch from the whole f matrix, exhaustive enumeration of every
batch, the closed forms of EI and PI under a Gaussian f.  The lazy path is held to the bits of the full one.
"""
import itertools
import math

import numpy as np
import pytest

from fokl_gpy_amd import FoKLRoutines, getKernels, population
from fokl_gpy_amd import acquire as aq
from fokl_gpy_amd.embedded import basis_matrix

KERNEL = 'Bernoulli Polynomials'
PHIS = getKernels.bernoulli()
MTX = np.array([[1, 0], [0, 1], [2, 0], [1, 1], [0, 2]])             # 6 columns with the intercept


def continuous_case(seed, S=1029, nc=17, E=200):
    """(X [S, nc], betas [E, nc], b0 [E]): uniform columns behind an intercept, draws around one mean, and as the incumbent
    of a draw its best value over 50 other rows (what incumbent='training' is to a model).  (Shared with the GPU tests.)"""
    rng = np.random.default_rng([seed, S, nc, E])
    X = np.concatenate([np.ones((S, 1)), rng.uniform(-1.0, 1.0, size=(S, nc - 1))], axis=1)
    betas = rng.standard_normal(nc) + 0.3 * rng.standard_normal((E, nc))
    train = np.concatenate([np.ones((50, 1)), rng.uniform(-1.0, 1.0, size=(50, nc - 1))], axis=1)
    return X, betas, (train @ betas.T).max(axis=0)


def integer_case(seed, S, nc, E):
    """(X, betas, b0) of small integers: X = [1 | -3..3], betas in -2..2, b0 in -4..4.  Every f is an integer below
    9 (3 nc + 1), every difference and every sum of them an exact integer in any order, and b stays integer after every
    pick.  (Shared with the GPU tests.)"""
    rng = np.random.default_rng([seed, S, nc, E])
    X = np.concatenate([np.ones((S, 1)), rng.integers(-3, 4, size=(S, nc - 1))], axis=1).astype(np.float64)
    betas = rng.integers(-2, 3, size=(E, nc)).astype(np.float64)
    return X, betas, rng.integers(-4, 5, size=E).astype(np.float64)


def model_case(seed=0, n=60, S=40, E=30):
    rng = np.random.default_rng(seed)
    betas = np.array([0.3, 1.0, -0.8, 0.5, 1.5, -0.7]) + 0.2 * rng.standard_normal((E, 6))
    return rng.random((n, 2)), rng.random((S, 2)), betas


def columns(x):
    return basis_matrix(np.asarray(x, dtype=np.float64), MTX, PHIS, KERNEL)


def host(betas, train, pool, **kw):
    return aq.acquire_host(betas, MTX, PHIS, KERNEL, train, pool, **kw)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_cumsum_of_the_gains_is_the_joint_value_of_the_batch(criterion):
    """Continuous data: to 1e-12 relative (sums of a few hundred terms of one sign in two orders differ by rounding times
    their number).  Integer data with 64 draws (the division is exact): equal."""
    X, betas, b0 = continuous_case(3, S=200, nc=9)
    F = X @ betas.T
    res = aq.select_host(X, betas, b0, picks=10, criterion=criterion)
    joint = np.cumsum(res['gain'])
    assert res['gain'][0] > 0.0 and np.all(res['gain'] >= 0.0)
    for k in range(10):
        scratch = aq.joint_value(F, b0, res['index'][:k + 1], criterion)
        assert abs(joint[k] - scratch) <= 1e-12 * scratch, k
    X, betas, b0 = integer_case(1, 100, 5, 64)
    F = X @ betas.T
    res = aq.select_host(X, betas, b0, picks=8, criterion=criterion)
    assert res['gain'][0] > 0.0
    assert np.array_equal(np.cumsum(res['gain']), [aq.joint_value(F, b0, res['index'][:k + 1], criterion) for k in range(8)])


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_greedy_meets_the_submodularity_bound_against_exhaustive_search(criterion):
    """12-row pools, picks=3, 40 seeds: greedy >= (1 - 1 / e) x the best of all 220 batches.  A condition."""
    worst = 1.0
    for seed in range(40):
        X = continuous_case(seed, S=12, nc=5, E=60)[0]
        betas = np.random.default_rng(seed).standard_normal((60, 5))             # draws that disagree about the best row
        F = X @ betas.T
        b0 = np.quantile(F, 0.75, axis=0)                        # a quarter of the pool improves on a draw: batches differ
        res = aq.select_host(X, betas, b0, picks=3, criterion=criterion)
        greedy = aq.joint_value(F, b0, res['index'], criterion)
        best = max(aq.joint_value(F, b0, batch, criterion) for batch in itertools.combinations(range(12), 3))
        assert greedy <= best + 1e-12
        assert greedy >= (1.0 - 1.0 / math.e) * best, seed
        assert res['index'][0] == int(np.argmax([aq.joint_value(F, b0, [s], criterion) for s in range(12)]))
        if best > 0.0:
            worst = min(worst, greedy / best)
    print(f"{criterion}: the worst greedy / exhaustive ratio over 40 pools is {worst:.3f}")


def test_closed_forms_under_gaussian_draws():
    """betas ~ N(m, V) and a scalar incumbent: f_s ~ N(x.m, x'Vx), EI = s (z Phi(z) + phi(z)), PI = Phi(z).  200 000 draws;
    every row within 4 standard errors, the error taken from the sample's own spread."""
    rng = np.random.default_rng(11)
    nc, E, b = 4, 200_000, 0.7
    m = np.array([0.2, 0.6, -0.4, 0.3])
    L = np.tril(0.3 * rng.standard_normal((nc, nc))) + 0.2 * np.eye(nc)
    betas = m + rng.standard_normal((E, nc)) @ L.T
    X = np.concatenate([np.ones((8, 1)), rng.uniform(-1.0, 1.0, size=(8, nc - 1))], axis=1)
    F = X @ betas.T
    s = np.sqrt(np.einsum('si,ij,sj->s', X, L @ L.T, X))
    z = (X @ m - b) / s
    Phi = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in z])
    phi = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    closed = {'ei': s * (z * Phi + phi), 'pi': Phi}
    terms = {'ei': np.maximum(F - b, 0.0), 'pi': (F > b).astype(np.float64)}
    for criterion in aq.CRITERIA:
        got = aq.select_host(X, betas, np.full(E, b), picks=1, criterion=criterion, trace_pick=0)['trace_g']
        se = terms[criterion].std(axis=1, ddof=1) / math.sqrt(E)
        dev = np.abs(got - closed[criterion]) / se
        print(f"{criterion}: worst deviation from the closed form {dev.max():.2f} standard errors")
        assert np.all(se > 0.0) and np.all(dev <= 4.0), dev


def test_lazy_returns_the_bits_of_evaluating_everything_and_skips():
    fewest = None
    for seed in range(5):
        X, betas, b0 = continuous_case(seed)
        tiles = -(-X.shape[0] // 16)
        for criterion in aq.CRITERIA:
            full = aq.select_host(X, betas, b0, picks=12, criterion=criterion, lazy=False)
            lazy = aq.select_host(X, betas, b0, picks=12, criterion=criterion, lazy=True)
            assert np.array_equal(lazy['index'], full['index']) and lazy['index'].min() >= 0, (seed, criterion)
            assert lazy['gain'].tobytes() == full['gain'].tobytes(), (seed, criterion)
            assert lazy['incumbent_after'].tobytes() == full['incumbent_after'].tobytes(), (seed, criterion)
            assert np.all(full['tiles_evaluated'] == tiles) and lazy['tiles_evaluated'][0] == tiles
            assert np.all(lazy['tiles_evaluated'] >= 1) and np.all(lazy['tiles_evaluated'] <= tiles)
            later = int(lazy['tiles_evaluated'][1:].min())
            fewest = later if fewest is None else min(fewest, later)
    print(f"the cheapest later pick evaluated {fewest} of 65 tiles")
    assert fewest < 65                                           # a lazy path that evaluates everything fails here


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_lazy_trace_is_the_full_trace_where_a_tile_was_evaluated(criterion):
    """At the later pick that evaluated fewest tiles: fresh rows hold the full run's bits, and a skipped un-picked row holds a
    stale gain that bounds its gain now and is below the pick's."""
    X, betas, b0 = continuous_case(2)
    k = 1 + int(np.argmin(aq.select_host(X, betas, b0, picks=6, criterion=criterion)['tiles_evaluated'][1:]))
    full = aq.select_host(X, betas, b0, picks=6, criterion=criterion, lazy=False, trace_pick=k)
    lazy = aq.select_host(X, betas, b0, picks=6, criterion=criterion, lazy=True, trace_pick=k)
    rows = np.repeat(lazy['trace_eval'].astype(bool), 16)[:X.shape[0]]
    assert lazy['trace_eval'].sum() == lazy['tiles_evaluated'][k] < 65
    assert np.array_equal(lazy['trace_g'][rows], full['trace_g'][rows])
    stale = ~rows
    stale[lazy['index'][:k]] = False                             # a picked row is behind the mask: its gain is not read
    assert stale.any()
    assert np.all(lazy['trace_g'][stale] >= full['trace_g'][stale])              # a stale gain is an upper bound
    assert np.all(lazy['trace_g'][stale] < lazy['gain'][k])
    if criterion == 'ei':
        assert np.all(full['trace_g'][full['index'][:k]] == 0.0)                 # a picked row improves on nothing


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_sense_min_is_max_on_negated_betas_and_incumbent(criterion):
    train, pool, betas = model_case()
    b0 = np.random.default_rng(4).normal(0.4, 0.2, size=betas.shape[0])
    lo = host(betas, train, pool, picks=6, criterion=criterion, sense='min', incumbent=b0, keep='first')
    hi = host(-betas, train, pool, picks=6, criterion=criterion, sense='max', incumbent=-b0, keep='first')
    assert np.array_equal(lo.index, hi.index)
    for name in ('gain', 'joint', 'first'):
        assert lo[name].tobytes() == hi[name].tobytes(), name
    assert np.array_equal(lo.incumbent, b0) and np.array_equal(lo.incumbent_after, -hi.incumbent_after)
    assert np.array_equal(lo.x, pool[lo.index]) and lo.sense == 'min' and lo.first.shape == (40,)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_an_incumbent_above_everything_gains_nothing_and_picks_in_pool_order(criterion):
    train, pool, betas = model_case(1)
    top = float((columns(pool) @ betas.T).max())
    res = host(betas, train, pool, picks=5, criterion=criterion, incumbent=top + 1.0)
    assert res.index.tolist() == [0, 1, 2, 3, 4] and np.array_equal(res.gain, np.zeros(5)) and np.array_equal(res.joint, np.zeros(5))
    assert np.array_equal(res.incumbent_after, res.incumbent) and np.all(res.incumbent == top + 1.0)
    low = host(betas, train, pool, picks=5, criterion=criterion, sense='min', incumbent=-top - 100.0)
    assert low.index.tolist() == [0, 1, 2, 3, 4] and np.array_equal(low.gain, np.zeros(5))


def test_pi_without_an_incumbent_picks_by_coverage_and_ei_is_refused():
    train, pool, betas = model_case(2)
    res = host(betas, train, pool, picks=3, criterion='pi', incumbent='none')
    assert res.index.tolist() == [0, 1, 2] and res.gain.tolist() == [1.0, 0.0, 0.0]    # the first row covers every draw
    assert np.all(res.incumbent == -np.inf) and np.all(res.incumbent_after == np.inf)
    part = np.where(np.arange(betas.shape[0]) % 2 == 0, -np.inf, 1e9)           # only the even draws can be covered
    res = host(betas, train, pool, picks=2, criterion='pi', incumbent=part)
    assert res.gain.tolist() == [0.5, 0.0] and np.array_equal(np.isinf(res.incumbent_after), part < 0.0)
    with pytest.raises(ValueError, match="criterion='ei' needs a finite incumbent.*infinite"):
        host(betas, train, pool, criterion='ei', incumbent='none')
    with pytest.raises(ValueError, match="criterion='ei' needs a finite incumbent"):
        host(betas, train, pool, criterion='ei', incumbent=part)


def test_training_incumbent_is_propagates_per_draw_extreme():
    train, pool, betas = model_case(3)
    pop = population.propagate_host(betas, MTX, PHIS, KERNEL, train)
    assert np.array_equal(host(betas, train, pool, picks=2).incumbent, pop.max)
    assert np.array_equal(host(betas, train, pool, picks=2, sense='min').incumbent, pop.min)
    last = host(betas, train, pool, picks=2, draws=7)
    assert np.array_equal(last.incumbent, pop.max[-7:]) and last.draws == 7
    some = host(betas, train, pool, picks=2, draws=np.array([3, 0, 11]), incumbent=np.arange(30.0))
    assert np.array_equal(some.incumbent, [3.0, 0.0, 11.0])


def test_a_fit_alone_is_enough_and_nothing_is_drawn_at_random():
    train, pool, betas = model_case(4)
    np.random.seed(9)
    state = np.random.get_state()[1].copy()
    a, b = host(betas, train, pool, picks=4), host(betas, train, pool, picks=4, lazy=False)
    assert np.array_equal(np.random.get_state()[1], state)
    assert np.array_equal(a.index, b.index) and a.gain.tobytes() == b.gain.tobytes()
    assert len(set(a.index.tolist())) == 4 and np.all(np.diff(a.joint) >= 0.0) and a.first is None
    one = host(betas[0], train, pool, picks=1)                    # one coefficient vector: one draw
    assert one.draws == 1 and one.incumbent.shape == (1,)


def test_refusals_name_their_limit(monkeypatch):
    train, pool, betas = model_case(5)
    with pytest.raises(ValueError, match='call fit first'):
        aq.acquire_host(betas, None, PHIS, KERNEL, train, pool)
    with pytest.raises(ValueError, match='training inputs'):
        aq.acquire_host(betas, MTX, PHIS, KERNEL, None, pool)
    with pytest.raises(ValueError, match=r'pool \[S, M\] is needed'):
        host(betas, train, None)
    with pytest.raises(ValueError, match=r'pool must be \[S, 2\]'):
        host(betas, train, np.zeros((5, 3)))
    with pytest.raises(ValueError, match='the interaction matrix has 3'):
        aq.acquire_host(betas, np.ones((5, 3), dtype=int), PHIS, KERNEL, train, pool)
    with pytest.raises(ValueError, match='picks must be an integer >= 1'):
        host(betas, train, pool, picks=0)
    with pytest.raises(ValueError, match='41 picks from a pool of 40 rows: at most 40'):
        host(betas, train, pool, picks=41)
    with pytest.raises(ValueError, match=r"criterion must be one of \('ei', 'pi'\)"):
        host(betas, train, pool, criterion='ucb')
    with pytest.raises(ValueError, match=r"sense must be one of \('max', 'min'\)"):
        host(betas, train, pool, sense='up')
    with pytest.raises(ValueError, match="keep must be None or 'first'"):
        host(betas, train, pool, keep='all')
    with pytest.raises(ValueError, match='betas have 5 columns, the interaction matrix wants 6'):
        host(betas[:, :5], train, pool)
    holed = betas.copy()
    holed[[2, 9]] = np.nan
    with pytest.raises(ValueError, match=r"2 of the 30 draws are NaN or infinite \(the rows of a resample's flagged chains"):
        host(holed, train, pool)
    assert host(holed, train, pool, picks=2, draws=np.flatnonzero(np.isfinite(holed).all(axis=1))).draws == 28
    with pytest.raises(ValueError, match=r'draws must be None \(all\), an integer in 1..30'):
        host(betas, train, pool, draws=31)
    with pytest.raises(ValueError, match='draws as an array must hold at least one integer index into the 30 rows'):
        host(betas, train, pool, draws=np.array([30]))
    with pytest.raises(ValueError, match="incumbent must be 'training', 'none', a number or an array"):
        host(betas, train, pool, incumbent='best')
    with pytest.raises(ValueError, match=r'one value per draw \(30\)'):
        host(betas, train, pool, incumbent=np.zeros(29))
    with pytest.raises(ValueError, match='every incumbent must be finite, or -inf'):
        host(betas, train, pool, criterion='pi', incumbent=np.nan)
    with pytest.raises(ValueError, match='every incumbent must be finite, or -inf'):
        host(betas, train, pool, criterion='pi', incumbent=np.inf)
    with pytest.raises(ValueError, match='every incumbent must be finite, or inf'):
        host(betas, train, pool, criterion='pi', sense='min', incumbent=-np.inf)
    rows = pool.copy()
    rows[7, 1] = np.nan
    with pytest.raises(ValueError, match=r'1 of the 40 pool rows are NaN or infinite \(the first is row 7\)'):
        host(betas, train, rows)
    with pytest.raises(ValueError, match='the training inputs must be finite'):
        host(betas, np.where(np.arange(120).reshape(60, 2) == 5, np.inf, train), pool)
    wide = np.array([r for r in itertools.product(range(11), repeat=3) if any(r)][:aq.MAX_COLUMNS])
    with pytest.raises(ValueError, match=r'1281 columns \(terms \+ 1\), acquire takes at most 1280 .*160 KiB'):
        aq.acquire_host(np.zeros((2, 1281)), wide, PHIS, KERNEL, np.zeros((3, 3)), np.zeros((3, 3)))
    monkeypatch.setenv('FOKL_ACQUIRE_FREE_BYTES', str(64 << 20))
    with pytest.raises(ValueError, match='64 MiB to spare, FOKL_ACQUIRE_FREE_BYTES counts 67108864 as free'):
        host(betas, train, pool)
    monkeypatch.delenv('FOKL_ACQUIRE_FREE_BYTES')
    model = FoKLRoutines.FoKL(kernel=KERNEL, UserWarnings=False, ConsoleOutput=False)
    with pytest.raises(ValueError, match='acquire needs a fitted model: call fit first'):
        model.acquire(pool=pool)
    model.mtx, model.betas, model.inputs = MTX, betas, train
    with pytest.raises(ValueError, match="acquire takes a resample's result OR betas=, not both"):
        model.acquire(dict(betas=betas), pool=pool, betas=betas)
    with pytest.raises(ValueError, match='this resample kept no rows'):
        model.acquire(dict(betas=None), pool=pool)
    with pytest.raises(ValueError, match='needs what resample returned'):
        model.acquire(3.0, pool=pool)

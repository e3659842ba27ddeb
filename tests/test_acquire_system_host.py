"""acquire.acquire_system_host / acquire.select_system_host, the numpy statement of the batch acquisition under limits on
other models' outputs, against independent arithmetic (no device).

References are formed from scratch: ``select_host`` for infinite limits, the joint value of a batch from the whole f and
feasibility matrices, exhaustive enumeration of every batch, the closed form of EI x P(feasible) under independent Gaussian
draws.  The lazy path is held to the bits of the full one.
"""
import itertools
import math

import numpy as np
import pytest

from test_acquire_host import KERNEL, MTX, PHIS, columns, continuous_case, integer_case, model_case
from fokl_gpy_amd import acquire as aq
from fokl_gpy_amd.embedded import basis_matrix

LIMITS = (-0.5, 0.8)
INF = (np.array([-np.inf]), np.array([np.inf]))


def constraint_case(seed, S=1029, E=200):
    """(Xc [S, 5], betas_c [E, 5]) of the constraint model: an intercept and four uniform(-1, 1) columns, draws
    [0.2, 1, -1, 0.5, 0.3] + 0.3 N(0, 1); with LIMITS about half of the (row, draw) pairs are feasible.  (Shared with the GPU
    tests.)"""
    rng = np.random.default_rng([77, seed, S, E])
    Xc = np.concatenate([np.ones((S, 1)), rng.uniform(-1.0, 1.0, size=(S, 4))], axis=1)
    return Xc, np.array([0.2, 1.0, -1.0, 0.5, 0.3]) + 0.3 * rng.standard_normal((E, 5))


def feasibility(Xc, betas_c, limits=LIMITS):
    G = Xc @ betas_c.T
    return (G >= limits[0]) & (G <= limits[1])


def system(X, betas, Xc, betas_c, b0, limits=LIMITS, **kw):
    return aq.select_system_host([X, Xc], [betas, betas_c], b0, [limits[0]], [limits[1]], **kw)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('lazy', (False, True))
def test_infinite_limits_return_the_bytes_of_the_unconstrained_statement(criterion, lazy):
    for seed in range(3):
        X, betas, b0 = continuous_case(seed)
        Xc, betas_c = constraint_case(seed)
        free = aq.select_host(X, betas, b0, picks=8, criterion=criterion, lazy=lazy, trace_pick=7)
        res = system(X, betas, Xc, betas_c, b0, limits=(-np.inf, np.inf), picks=8, criterion=criterion, lazy=lazy, trace_pick=7)
        for name in ('index', 'gain', 'incumbent_after', 'tiles_evaluated', 'trace_g', 'trace_eval'):
            assert res[name].tobytes() == free[name].tobytes(), (name, seed)
        assert np.all(res['feasible'] == 200)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_lazy_is_full_and_cumsum_is_the_joint_value_under_real_limits(criterion):
    fewest, differ = 65, False
    for seed in range(3):
        X, betas, b0 = continuous_case(seed)
        Xc, betas_c = constraint_case(seed)
        F, ok = X @ betas.T, feasibility(Xc, betas_c)
        share = ok.mean()
        print(f"seed {seed}: the feasible share is {share:.3f}")
        assert 0.2 <= share <= 0.8
        full = system(X, betas, Xc, betas_c, b0, picks=10, criterion=criterion, lazy=False)
        lazy = system(X, betas, Xc, betas_c, b0, picks=10, criterion=criterion, lazy=True)
        assert np.array_equal(lazy['index'], full['index']) and lazy['index'].min() >= 0
        for name in ('gain', 'incumbent_after', 'feasible'):
            assert lazy[name].tobytes() == full[name].tobytes(), (name, seed)
        assert np.array_equal(full['feasible'], ok[full['index']].sum(axis=1))
        joint = np.cumsum(full['gain'])
        assert full['gain'][0] > 0.0 and np.all(full['gain'] >= 0.0)
        for k in range(10):
            scratch = aq.joint_value_system(F, ok, b0, full['index'][:k + 1], criterion)
            assert abs(joint[k] - scratch) <= 1e-12 * scratch, (seed, k)
        free = aq.select_host(X, betas, b0, picks=10, criterion=criterion)
        differ = differ or not np.array_equal(free['index'], full['index'])
        assert np.all(full['tiles_evaluated'] == 65) and lazy['tiles_evaluated'][0] == 65
        fewest = min(fewest, int(lazy['tiles_evaluated'][1:].min()))
    print(f"{criterion}: the cheapest later pick evaluated {fewest} of 65 tiles")
    assert differ and fewest < 65


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_cumsum_equals_the_joint_value_on_integer_data(criterion):
    """64 draws: the division is exact, every sum an integer: equal, not close."""
    X, betas, b0 = integer_case(1, 100, 5, 64)
    Xc, betas_c, _ = integer_case(2, 100, 3, 64)
    limits = (-4.0, 5.0)
    F, ok = X @ betas.T, feasibility(Xc, betas_c, limits)
    assert 0.2 <= ok.mean() <= 0.8
    res = system(X, betas, Xc, betas_c, b0, limits=limits, picks=8, criterion=criterion)
    assert res['gain'][0] > 0.0
    assert np.array_equal(np.cumsum(res['gain']),
                          [aq.joint_value_system(F, ok, b0, res['index'][:k + 1], criterion) for k in range(8)])


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_greedy_meets_the_submodularity_bound_against_exhaustive_search(criterion):
    """12-row pools, 40 seeds: greedy with three picks >= (1 - 1 / e) x the best of all 220 batches; with one pick it is the
    best row."""
    for seed in range(40):
        X = continuous_case(seed, S=12, nc=5, E=60)[0]
        betas = np.random.default_rng(seed).standard_normal((60, 5))
        Xc, betas_c = constraint_case(seed, S=12, E=60)
        F, ok = X @ betas.T, feasibility(Xc, betas_c)
        b0 = np.quantile(F, 0.75, axis=0)
        res = system(X, betas, Xc, betas_c, b0, picks=3, criterion=criterion)
        greedy = aq.joint_value_system(F, ok, b0, res['index'], criterion)
        best = max(aq.joint_value_system(F, ok, b0, batch, criterion) for batch in itertools.combinations(range(12), 3))
        assert greedy <= best + 1e-12
        assert greedy >= (1.0 - 1.0 / math.e) * best, seed
        singles = [aq.joint_value_system(F, ok, b0, [s], criterion) for s in range(12)]
        one = system(X, betas, Xc, betas_c, b0, picks=1, criterion=criterion)
        assert one['index'][0] == int(np.argmax(singles)) == res['index'][0]


def test_the_first_gain_is_the_closed_form_times_the_probability_of_feasibility():
    """One row, f ~ N(mu, s^2) and g ~ N(m, r^2) independent, a scalar incumbent b: the gain is the mean of
    t = [lo <= g <= hi] max(f - b, 0), whose expectation is EI(mu, s, b) P and whose variance is P E[(f - b)+^2] - (EI P)^2 with
    E[(f - b)+^2] = s^2 ((z^2 + 1) Phi(z) + z phi(z)); for 'pi' a Bernoulli variable with p = Phi(z) P.  The standard error
    follows from E; 4 of them are allowed."""
    rng = np.random.default_rng(21)
    E, b, mu, s, m, r = 200_000, 0.7, 0.5, 0.4, 0.1, 0.5
    one = np.ones((1, 1))
    betas = mu + s * rng.standard_normal((E, 1))
    betas_c = m + r * rng.standard_normal((E, 1))
    Phi = lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0)))
    P = Phi((LIMITS[1] - m) / r) - Phi((LIMITS[0] - m) / r)
    z = (mu - b) / s
    phi = math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    ei = s * (z * Phi(z) + phi)
    second = s * s * ((z * z + 1.0) * Phi(z) + z * phi)
    closed = {'ei': ei * P, 'pi': Phi(z) * P}
    se = {'ei': math.sqrt((P * second - (ei * P) ** 2) / E), 'pi': math.sqrt(Phi(z) * P * (1.0 - Phi(z) * P) / E)}
    for criterion in aq.CRITERIA:
        got = system(one, betas, one, betas_c, np.full(E, b), picks=1, criterion=criterion)['gain'][0]
        dev = abs(got - closed[criterion]) / se[criterion]
        print(f"{criterion}: {got:.6f} against {closed[criterion]:.6f}, {dev:.2f} standard errors")
        assert dev <= 4.0


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('lazy', (False, True))
def test_a_pool_with_no_feasible_row_gains_nothing_and_is_taken_in_order(criterion, lazy):
    X, betas, b0 = continuous_case(0, S=40, nc=5, E=30)
    Xc, betas_c = constraint_case(0, S=40, E=30)
    res = system(X, betas, Xc, betas_c, b0 - 10.0, limits=(50.0, 60.0), picks=5, criterion=criterion, lazy=lazy, trace_pick=0)
    assert res['index'].tolist() == [0, 1, 2, 3, 4] and res['gain'].tobytes() == np.zeros(5).tobytes()
    assert res['incumbent_after'].tobytes() == (b0 - 10.0).tobytes() and np.all(res['feasible'] == 0)
    assert res['trace_g'].tobytes() == np.zeros(40).tobytes()


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_nan_in_a_constraint_column_is_infeasible_and_nan_in_the_objective_needs_a_feasible_draw(criterion):
    X, betas, b0 = integer_case(7, 40, 9, 24)
    Xc, betas_c, _ = integer_case(8, 40, 3, 24)
    limits = (-4.0, 5.0)
    ok = feasibility(Xc, betas_c, limits)
    assert ok[3].any() and ok[20].any()
    Xn = Xc.copy()
    Xn[3, 1] = np.nan                                            # row 3 becomes infeasible in every draw
    res = system(X, betas, Xn, betas_c, b0, limits=limits, picks=40, criterion=criterion, trace_pick=0)
    assert res['trace_g'][3] == 0.0 and not np.isnan(res['trace_g']).any() and np.all(res['index'] >= 0)
    assert res['feasible'][res['index'].tolist().index(3)] == 0
    Xo = X.copy()
    Xo[[3, 20], 5] = np.nan                                      # the objective is NaN at rows 3 and 20
    res = system(Xo, betas, Xn, betas_c, b0, limits=limits, picks=40, criterion=criterion, trace_pick=0)
    assert res['trace_g'][3] == 0.0 and np.isnan(res['trace_g'][20])
    assert np.array_equal(np.flatnonzero(np.isnan(res['trace_g'])), [20])
    assert sorted(res['index'][:39].tolist()) == sorted(set(range(40)) - {20}) and res['index'][39] == -1
    assert res['gain'][39] == -np.inf and res['feasible'][39] == 0


# ---- acquire_system_host: two fitted models -------------------------------------------------------------------------

MTX_C = np.array([[1], [2]])                                     # the constraint model reads one input: 3 columns
MINMAX = [[0.0, 2.0], [-1.0, 1.0]]
MINMAX_C = [[-2.0, 2.0]]


def models_case(seed=0, n=60, S=40, E=30):
    """Objective 'yield' over (a, b), constraint 'impurity' over b alone with another minmax; pool and measured rows in true
    scale.  (Shared with the GPU tests.)"""
    train, pool, betas = model_case(seed, n, S, E)
    rng = np.random.default_rng([seed, 5])
    betas_c = np.array([0.1, 0.8, -0.5]) + 0.2 * rng.standard_normal((E, 3))
    low, span = np.array([0.0, -1.0]), np.array([2.0, 2.0])
    models = [dict(betas=betas, mtx=MTX, phis=PHIS, minmax=MINMAX, kernel=KERNEL, inputs=train),
              dict(betas=betas_c, mtx=MTX_C, phis=PHIS, minmax=MINMAX_C, kernel=KERNEL)]
    return models, low + pool * span, low + train * span


XVARS, YVARS = [['a', 'b'], ['b']], ['yield', 'impurity']
LIMIT = {'impurity': (None, 0.25)}


def scratch(models, x, sign=1.0):
    """(F, ok) [rows, E] of true-scale rows x from basis_matrix per model."""
    xa = (x - np.array([0.0, -1.0])) / np.array([2.0, 2.0])
    xc = (x[:, 1:] - (-2.0)) / 4.0
    F = basis_matrix(xa, MTX, PHIS, KERNEL) @ (sign * models[0]['betas']).T
    G = basis_matrix(xc, MTX_C, PHIS, KERNEL) @ models[1]['betas'].T
    return F, G <= 0.25


def host(models, pool, **kw):
    kw.setdefault('constraints', LIMIT)
    kw.setdefault('no_feasible', 0.3)                            # some seeds leave a draw without a feasible measured row
    return aq.acquire_system_host(models, XVARS, YVARS, 'yield', pool, **kw)


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('sense', aq.SENSES)
def test_measured_incumbent_counts_and_the_result_fields(criterion, sense):
    models, pool, measured = models_case(1)
    sign = 1.0 if sense == 'max' else -1.0
    Fm, okm = scratch(models, measured, sign)
    F, ok = scratch(models, pool, sign)
    assert 0.1 < ok.mean() < 0.9 and okm.any(axis=0).all()
    res = host(models, pool, picks=5, criterion=criterion, sense=sense, keep='first')
    best = np.where(okm, Fm, -np.inf).max(axis=0)
    assert np.array_equal(res.measured_feasible, okm.sum(axis=0)) and res.measured_feasible.dtype == np.int64
    assert np.allclose(res.incumbent, sign * best, rtol=1e-12, atol=0)
    again = host(models, pool, picks=5, criterion=criterion, sense=sense, measured=measured)
    assert np.allclose(again.incumbent, res.incumbent, rtol=1e-12, atol=0) and np.array_equal(again.index, res.index)
    assert np.array_equal(res.feasible_draws, ok[res.index].sum(axis=1)) and np.array_equal(res.p_feasible, res.feasible_draws / 30)
    assert np.array_equal(res.x, pool[res.index]) and res.first.shape == (40,) and res.row_tiles == 3
    assert np.allclose(res.first, aq.gain_rows_system(F, ok, sign * res.incumbent, criterion), rtol=1e-9, atol=1e-12)
    assert np.array_equal(res.joint, np.cumsum(res.gain)) and res.variables == ['a', 'b']
    swapped = aq.acquire_system_host(models, XVARS, YVARS, 'yield', pool[:, ::-1], variables=['b', 'a'], constraints=LIMIT,
                                     picks=5, criterion=criterion, sense=sense, measured=measured[:, ::-1])
    assert np.array_equal(swapped.index, res.index) and np.array_equal(swapped.x, pool[res.index][:, ::-1])


def test_draws_without_a_feasible_measured_row():
    models, pool, measured = models_case(2)
    tight = {'impurity': (None, -0.35)}
    okm = basis_matrix((measured[:, 1:] + 2.0) / 4.0, MTX_C, PHIS, KERNEL) @ models[1]['betas'].T <= -0.35
    empty = ~okm.any(axis=0)
    assert 0 < empty.sum() < 30
    with pytest.raises(ValueError, match=f"{int(empty.sum())} of the 30 draws have no feasible measured row.*no_feasible="):
        host(models, pool, constraints=tight, picks=2, no_feasible=None)
    res = host(models, pool, constraints=tight, picks=2, no_feasible=0.25)
    assert np.all(res.incumbent[empty] == 0.25) and np.all(np.isfinite(res.incumbent))
    assert np.array_equal(res.measured_feasible == 0, empty)
    res = host(models, pool, constraints=tight, picks=2, criterion='pi', no_feasible=None)
    assert np.all(res.incumbent[empty] == -np.inf) and np.all(np.isfinite(res.incumbent[~empty]))
    low = host(models, pool, constraints=tight, picks=2, criterion='pi', sense='min', no_feasible=None)
    assert np.all(low.incumbent[empty] == np.inf)
    given = host(models, pool, picks=2, incumbent=0.4)
    assert np.all(given.incumbent == 0.4) and given.measured_feasible is None
    none = host(models, pool, picks=2, criterion='pi', incumbent='none')
    assert np.all(none.incumbent == -np.inf) and none.gain[0] > 0.0
    last = host(models, pool, picks=2, draws=7, incumbent=np.arange(30.0))
    assert np.array_equal(last.incumbent, np.arange(23.0, 30.0)) and last.draws == 7


def test_measured_none_needs_the_constraints_to_read_the_objectives_variables():
    models, pool, measured = models_case(3)
    wide = np.concatenate([pool, np.zeros((40, 1))], axis=1)
    with pytest.raises(ValueError, match=r"the constraint model 'impurity' reads \['c'\], which the objective does not: pass "
                                         r"measured="):
        aq.acquire_system_host(models, [['a', 'b'], ['c']], YVARS, 'yield', wide, constraints=LIMIT)
    res = aq.acquire_system_host(models, [['a', 'b'], ['c']], YVARS, 'yield', wide, constraints=LIMIT, picks=2, no_feasible=0.3,
                                 measured=np.concatenate([measured, np.zeros((60, 1))], axis=1))
    assert res.variables == ['a', 'b', 'c'] and res.x.shape == (2, 3)
    bare = [dict(models[0]), models[1]]
    del bare[0]['inputs']
    with pytest.raises(ValueError, match='it has none: pass measured='):
        host(bare, pool)


def test_refusals_name_their_limit(monkeypatch):
    models, pool, measured = models_case(4)
    third = dict(models[1])
    with pytest.raises(ValueError, match="without one use acquire"):
        host(models, pool, constraints={})
    with pytest.raises(ValueError, match="constraints: 'yield' is the objective"):
        host(models, pool, constraints={'yield': (0.0, 1.0)})
    with pytest.raises(ValueError, match="constraints: 'purity' is not a model output"):
        host(models, pool, constraints={'purity': (0.0, 1.0)})
    with pytest.raises(ValueError, match="model 'colour' is neither the objective nor constrained"):
        aq.acquire_system_host(models + [third], XVARS + [['b']], YVARS + ['colour'], 'yield', pool, constraints=LIMIT)
    with pytest.raises(ValueError, match=r"constraints\['impurity'\]: the lower limit 1.0 is above the upper limit 0.5"):
        host(models, pool, constraints={'impurity': (1.0, 0.5)})
    with pytest.raises(ValueError, match=r"constraints\['impurity'\] must be numbers or None, not NaN"):
        host(models, pool, constraints={'impurity': (np.nan, 0.5)})
    with pytest.raises(ValueError, match="at most 8 models.*not 9"):
        aq.acquire_system_host([models[0]] + [third] * 8, [['a', 'b']] + [['b']] * 8, ['yield'] + [f'c{k}' for k in range(8)],
                               'yield', pool, constraints={f'c{k}': (None, 1.0) for k in range(8)})
    with pytest.raises(ValueError, match="output 'impurity' is also a model's input.*optimize_system"):
        aq.acquire_system_host(models, [['a', 'impurity'], ['b']], YVARS, 'yield', pool, constraints=LIMIT)
    with pytest.raises(ValueError, match="objective 'a' is not a model output"):
        aq.acquire_system_host(models, XVARS, YVARS, 'a', pool, constraints=LIMIT)
    with pytest.raises(ValueError, match="xvars and yvars need one entry per model"):
        aq.acquire_system_host(models, XVARS[:1], YVARS, 'yield', pool, constraints=LIMIT)
    with pytest.raises(ValueError, match=r"models\[1\]: its coefficient table \(phis\) differs from the other models'"):
        host([models[0], dict(models[1], phis=PHIS[:3])], pool)
    with pytest.raises(ValueError, match=r"models\[1\]: its coefficient table \(phis\) differs from the other models'"):
        host([models[0], dict(models[1], kernel='Cubic Splines')], pool)
    with pytest.raises(ValueError, match=r"models\[1\] lacks \['minmax'\]"):
        host([models[0], {key: value for key, value in models[1].items() if key != 'minmax'}], pool)
    with pytest.raises(ValueError, match=r"models\[1\]: betas have 2 columns, the interaction matrix wants 3"):
        host([models[0], dict(models[1], betas=models[1]['betas'][:, :2])], pool)
    with pytest.raises(ValueError, match="the draws are paired.*the models have \\[30, 29\\]"):
        host([models[0], dict(models[1], betas=models[1]['betas'][:29])], pool)
    shared = host([models[0], dict(models[1], betas=models[1]['betas'][0])], pool, picks=2)       # one row is shared
    assert shared.draws == 30
    with pytest.raises(ValueError, match=r"variables must name every input the models read, once each: \['a', 'b'\]"):
        host(models, pool, variables=['a'])
    with pytest.raises(ValueError, match=r'pool must be \[S, 2\]'):
        host(models, np.zeros((5, 3)))
    with pytest.raises(ValueError, match=r'pool \[S, 2\] is needed'):
        host(models, None)
    with pytest.raises(ValueError, match='picks must be an integer >= 1'):
        host(models, pool, picks=0)
    with pytest.raises(ValueError, match='41 picks from a pool of 40 rows: at most 40'):
        host(models, pool, picks=41)
    with pytest.raises(ValueError, match=r"criterion must be one of \('ei', 'pi'\)"):
        host(models, pool, criterion='ucb')
    with pytest.raises(ValueError, match=r"sense must be one of \('max', 'min'\)"):
        host(models, pool, sense='up')
    with pytest.raises(ValueError, match="keep must be None or 'first'"):
        host(models, pool, keep='all')
    rows = pool.copy()
    rows[7, 1] = np.nan
    with pytest.raises(ValueError, match=r'1 of the 40 pool rows are NaN or infinite \(the first is row 7\)'):
        host(models, rows)
    holed = models[1]['betas'].copy()
    holed[[2, 9]] = np.nan
    with pytest.raises(ValueError, match=r"models\[1\]: 2 of the 30 draws are NaN or infinite"):
        host([models[0], dict(models[1], betas=holed)], pool)
    assert host([models[0], dict(models[1], betas=holed)], pool, picks=2,
                draws=np.flatnonzero(np.isfinite(holed).all(axis=1))).draws == 28
    with pytest.raises(ValueError, match=r'draws must be None \(all\), an integer in 1..30'):
        host(models, pool, draws=31)
    with pytest.raises(ValueError, match="incumbent must be 'measured', 'none', a number or an array"):
        host(models, pool, incumbent='training')
    with pytest.raises(ValueError, match=r'one value per draw \(30\)'):
        host(models, pool, incumbent=np.zeros(29))
    with pytest.raises(ValueError, match='every incumbent must be finite, or -inf'):
        host(models, pool, criterion='pi', incumbent=np.inf)
    with pytest.raises(ValueError, match="criterion='ei' needs a finite incumbent"):
        host(models, pool, incumbent='none')
    with pytest.raises(ValueError, match=r'measured= must be \[n, 2\]'):
        host(models, pool, measured=np.zeros((4, 3)))
    with pytest.raises(ValueError, match='measured= must be finite'):
        host(models, pool, measured=np.full((4, 2), np.nan))
    with pytest.raises(ValueError, match='no_feasible must be None or a finite number'):
        host(models, pool, no_feasible=np.inf)
    wide = np.array([r for r in itertools.product(range(11), repeat=2) if any(r)])            # 120 terms
    wide3 = np.array([r for r in itertools.product(range(11), repeat=3) if any(r)][:1275])    # 1 276 columns
    big = dict(betas=np.zeros((2, 1276)), mtx=wide3, phis=PHIS, minmax=[[0.0, 1.0]] * 3, kernel=KERNEL)
    small = dict(betas=np.zeros((2, 5)), mtx=wide[:4, :1], phis=PHIS, minmax=[[0.0, 1.0]], kernel=KERNEL)
    with pytest.raises(ValueError, match=r'add up to 1284 \(\[1276, 8\]\); acquire_system takes at most 1280 .*160 KiB'):
        aq.acquire_system_host([big, small], [['a', 'b', 'c'], ['a']], YVARS, 'yield', np.zeros((3, 3)), constraints=LIMIT,
                               incumbent=0.0, picks=1)
    monkeypatch.setenv('FOKL_ACQUIRE_FREE_BYTES', str(64 << 20))
    with pytest.raises(ValueError, match='64 MiB to spare, FOKL_ACQUIRE_FREE_BYTES counts 67108864 as free'):
        host(models, pool)

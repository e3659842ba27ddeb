"""One iteration of the multistart optimiser on the MI355X, as the product kernel itself traces it (model_optimize(...,
trace_iteration=k)): values against an exact and a rational reference, every decision against the host statement's own
operations on the traced values, bit for bit.  tests/optimize_step_cases.py has the references and their derivation,
tests/test_optimize_step_host.py shows them right on the CPU."""
import numpy as np
import pytest

import optimize_step_cases as C
from test_optimize_gpu import draws_of, family
from fokl_gpy_amd import _capi
from fokl_gpy_amd import optimize as opt

pytestmark = pytest.mark.gpu
MAX_ITER, TOL = 60, 1e-10


def traced(ctx, mtx, betas, table, lo, hi, starts, sign, k, max_iter=MAX_ITER, tol=TOL):
    """(results, flat trace of iteration k, report)"""
    out = ctx.model_optimize(np.ascontiguousarray(mtx, dtype=np.int32), betas, table, lo, hi, starts, sign, max_iter, tol,
                             trace_iteration=k)
    report = ctx.optimize_report()
    assert report['traced'] == 1 and report['solves'] == betas.shape[0] * starts.shape[0] and report['launches'] == 1
    assert report['instance'] == ('uniform' if starts.shape[0] % 64 == 0 else 'per_lane')
    assert report['grid'] == -(-report['solves'] // 64) and report['lds_raised'] == int(report['lds_bytes'] > 65536)
    return out[:4], C.flat(out[4]), report


@pytest.mark.parametrize('name', ['one', 'six', 'sixteen'])
def test_the_first_pass_is_exact(device_ctx, name):
    """F, noise, g and H of iteration 0 equal ``optimize._model_parts`` by np.array_equal on integer data, for sign +1 and
    -1, over sizes with idle lanes in the last wavefront and a draw boundary inside a wavefront; every decision of the
    iteration from those values; each rule of the active set occurs at coordinate 0 and at coordinate m - 1."""
    seen = set()
    for E, S in C.SIZES:
        mtx, betas, starts, lo, hi = C.exact_problem(name, E, S)
        m = mtx.shape[1]
        x0, coef = C.first_points(betas, starts, lo, hi)
        tt = opt.TermTable(mtx)
        for sign in (1.0, -1.0):
            _, tr, report = traced(device_ctx, mtx, betas, C.INT_TABLE, lo, hi, starts, sign, 0)
            F, noise, g, H = opt._model_parts(tt, C.INT_TABLE, x0, coef, 2, scale=sign, weight=sign)
            label = f"{name} {E} x {S} sign {sign:+.0f}"
            assert tr['running'].all(), label
            assert np.array_equal(tr['x_in'], x0) and np.array_equal(tr['F'], F) and np.array_equal(tr['noise'], noise), label
            assert np.array_equal(tr['g'], g.T), label
            assert np.array_equal(tr['H'], H.T), (label, np.argwhere(tr['H'] != H.T)[:5])
            C.check_decisions(tr, lo, hi, TOL, 0, MAX_ITER, np.zeros(E * S, dtype=bool), label)
            seen |= C.rules_seen(tr['x_in'], tr['g'], tr['active'], lo, hi)
            wide = (mtx > 0).sum(axis=1)
            assert report['slots'] == tt.n_slots and report['side_list'] == int(wide[wide > 3].sum()), report
    assert seen == C.all_rules(m, fixed=m > 2), C.all_rules(m, m > 2) - seen
    if name == 'sixteen':
        assert report['lds_bytes'] > 65536 and report['lds_raised'] == 1


def rational_models():
    for name in ('two', 'eight', 'sixteen'):
        yield (name,) + family(name)
    yield 'twenty', C.TWENTY, C.TWENTY_MEAN


@pytest.mark.parametrize('k', [0, 3])
@pytest.mark.parametrize('name, mtx, mean', list(rational_models()), ids=lambda v: v if isinstance(v, str) else '')
def test_a_pass_stays_within_the_rational_bound_and_decides_as_the_statement(device_ctx, name, mtx, mean, k):
    """The real Bernoulli table (orders up to 20 in 'twenty'): F, noise, g, H and every traced Ft of sampled solves against
    exact rational arithmetic at the device's own traced points, within gamma_N M; every decision of every solve."""
    mtx = np.ascontiguousarray(mtx, dtype=np.int32)
    m = mtx.shape[1]
    lo, hi = np.zeros(m), np.ones(m)
    E, S = 2, 32
    betas, starts = draws_of(mean, E, 5), opt.start_points(S, lo, hi)
    _, tr, report = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, k)
    carried = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, k - 1)[1]['steepest'] if k else np.zeros(E * S, dtype=bool)
    counts = C.check_decisions(tr, lo, hi, TOL, k, MAX_ITER, carried, f"{name} k = {k}")
    assert counts['stepping'] >= E * S // 2, counts
    assert report['lds_raised'] == int(name in ('eight', 'sixteen'))   # 132 and 280 rows of 512 bytes
    coef = np.repeat(betas, S, axis=0)
    worst = dict(F=0.0, noise=0.0, g=0.0, H=0.0, Ft=0.0)
    picked = np.flatnonzero(tr['stepping'])[::7][:6]
    for b in picked:
        ratios = C.rational_ratios(mtx, C.TABLE, tr['x_in'][b], coef[b], -1.0, tr['F'][b], tr['noise'][b], tr['g'][b], tr['H'][b])
        points = C.trial_points(tr['x_in'][b], tr['d'][b], lo, hi, int(tr['trials'][b]))
        ratios['Ft'] = max(C.rational_value_ratio(mtx, C.TABLE, point, coef[b], -1.0, tr['Ft'][b, h])
                           for h, point in enumerate(points))
        worst = {key: max(worst[key], ratios[key]) for key in worst}
    print(f"\n{name} k = {k}: N = {C.roundings(mtx)}, {len(picked)} solves, largest error / bound on the device: "
          + ', '.join(f"{key} {value:.3f}" for key, value in worst.items()) + f"; {counts}")
    assert len(picked) >= 3 and max(worst.values()) <= 1.0, worst


def test_the_factorisation_at_its_edges(device_ctx):
    """Designed Hessians: positive definite, a negative pivot, a pivot of exactly 0, a pivot equal to the floor, a huge
    diagonal on an ACTIVE coordinate (the floor must not see it), reach below, equal to and above 1, and an overflowing
    entry that makes the Newton direction non-finite.  The traced H is the designed one, the factor and the direction are
    ``optimize._direction``'s on the traced H, g and active set, bit for bit."""
    for name, (betas, start, lo, hi, want) in C.factor_cases().items():
        lo, hi = np.array(lo), np.array(hi)
        _, tr, _ = traced(device_ctx, C.POWER_MTX, np.array([betas]), C.POWERS, lo, hi, np.array([start]), 1.0, 0)
        assert tr['H'][0].tolist() == want and tr['stepping'][0], name
        C.check_decisions(tr, lo, hi, TOL, 0, MAX_ITER, np.zeros(1, dtype=bool), name)
        assert not tr['use_steepest'][0], name
        if name == 'negative pivot':
            assert tr['factor'][0, 0] == np.sqrt(2.0)
        if name == 'zero pivot':
            assert tr['factor'][0, 2] == np.sqrt(opt.PIVOT_FLOOR * 4.0)
        if name == 'pivot on the floor':
            assert tr['factor'][0, 2] == np.sqrt(1e-8) and tr['H'][0, 2] == opt.PIVOT_FLOOR * 1.0
        if name == 'huge diagonal on an active coordinate':
            assert tr['active'][0].tolist() == [False, True] and tr['factor'][0, 0] == np.sqrt(1e-3)
            assert abs(tr['d'][0, 0] - 0.1) < 1e-12 and tr['d'][0, 1] == 0.0
        if name.startswith('reach'):
            assert np.max(np.abs(tr['d'][0])) == {'reach below 1': 0.5, 'reach equal to 1': 1.0, 'reach above 1': 1.0}[name]
            assert tr['d'][0].tolist() == {'reach below 1': [-0.5, -0.25], 'reach equal to 1': [-1.0, -0.5],
                                           'reach above 1': [-1.0, -1.0 / 3.0]}[name]
    o = C.OVERFLOW
    _, tr, _ = traced(device_ctx, o['mtx'], o['betas'], C.OVERFLOW_TABLE, o['lo'], o['hi'], o['starts'], 1.0, 0, tol=0.0)
    assert tr['status_tests'][0] == -1 and tr['H'][0].tolist() == [2.0, np.inf, 2.0] and np.isfinite(tr['g'][0]).all()
    C.check_decisions(tr, o['lo'], o['hi'], 0.0, 0, MAX_ITER, np.zeros(1, dtype=bool), 'overflow')
    assert tr['use_steepest'][0] and tr['d'][0].tolist() == [-1.0, -1.0] and not tr['failed'][0]


def test_the_search_at_its_edges(device_ctx):
    """The designed searches (their outcomes are asserted on the CPU from the host statement): accepted at the first, the
    twelfth and the thirty-first trial point; none accepted, then steepest descent; none twice: stalled; trial points that
    do not move; a trial point clipped in one coordinate and free in the other.  The traces of k = 0 and k = 1 decide as
    the host walk's records, and their values equal them bit for bit at the start, where every number of these cases is exact."""
    names, betas, starts, lo, hi = C.search_problem()
    S = len(names)
    walk = C.host_walk(C.POWER_MTX, C.POWERS, betas, starts, lo, hi, 1.0, MAX_ITER, 0.0)
    own = np.arange(S) * S + np.arange(S)                              # the solve of case i: draw i, start i
    carried = np.zeros(S * S, dtype=bool)
    for k in (0, 1):
        results, tr, _ = traced(device_ctx, C.POWER_MTX, betas, C.POWERS, lo, hi, starts, 1.0, k, tol=0.0)
        counts = C.check_decisions(tr, lo, hi, 0.0, k, MAX_ITER, carried, f"search k = {k}")
        carried = tr['steepest']
        rec = walk[k]
        for key in ('running', 'stepping', 'trials', 'failed', 'use_steepest', 'status'):
            assert np.array_equal(tr[key][own], rec[key][own]), (k, key, tr[key][own], rec[key][own])
        if k == 0:
            for key in ('x_in', 'x_out', 'd', 'F', 'g'):               # exact data at the start
                assert C.same(tr[key][own], rec[key][own]), (k, key)
            assert C.same(tr['Ft'][own[1:5]], rec['Ft'][own[1:5]])     # the cubics: powers of two throughout
            assert tr['trials'][own].tolist() == [1, 12, 31, 31, 31, 31, 1] and tr['failed'][own].tolist() == \
                [False, False, False, True, True, True, False]
            assert counts['first'] >= 1 and counts['middle'] >= 1 and counts['last'] >= 1 and counts['failed'] >= 3
        else:
            assert tr['use_steepest'][own].tolist() == [False, False, False, True, True, True, False]
            assert tr['status'][own[4]] == opt.STALLED and not tr['failed'][own[3]] and 5 <= tr['trials'][own[3]] <= 29
            assert not tr['failed'][own[5]] and tr['x_out'][own[5], 0] > 1.0
    status = results[3].ravel()
    assert status[own[4]] == opt.STALLED and results[2].ravel()[own[4]] == 1


def test_the_walk_of_one_small_case(device_ctx):
    """Every k from 0 to the last iteration, one launch each: x_out of k is x_in of k + 1, `steepest` is carried, a
    solve that stopped keeps its point while its neighbours go on, the returned iterations and status are the trace's,
    and a traced call returns what the plain call returns."""
    mtx, mean = family('two')
    lo, hi = np.zeros(2), np.ones(2)
    betas, starts = draws_of(mean, 2, 3), opt.start_points(12, lo, hi)
    args = (np.ascontiguousarray(mtx, dtype=np.int32), betas, C.TABLE, lo, hi, starts, -1.0, MAX_ITER, TOL)
    plain = device_ctx.model_optimize(*args)
    assert device_ctx.optimize_report()['traced'] == 0
    x, f, iterations, status = (a.reshape((24,) + a.shape[2:]) for a in plain)
    last = int(iterations.max())
    assert 2 <= last <= MAX_ITER and len(set(iterations.tolist())) >= 2   # the solves stop at different iterations
    before, stopped_at = None, np.full(24, -1)
    for k in range(last + 1):
        results, tr, _ = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, k)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(results, plain)), k   # trace on equals trace off
        assert np.array_equal(tr['running'], iterations >= k), k
        carried = before['steepest'] if before else np.zeros(24, dtype=bool)
        C.check_decisions(tr, lo, hi, TOL, k, MAX_ITER, carried, f"walk k = {k}")
        if before:
            assert np.array_equal(tr['x_in'], before['x_out']), k
        ends = tr['running'] & (tr['status'] >= 0)
        assert np.array_equal(ends, iterations == k) and np.array_equal(tr['status'][ends], status[ends]), k
        assert np.array_equal(tr['x_out'][iterations <= k], x[iterations <= k]), k   # stopped: the result, and it stays
        before = tr
    beyond = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, last + 1)[1]
    assert not beyond['running'].any() and np.all(beyond['status'] == -9)


def test_invariances_bit_for_bit(device_ctx):
    """A solve alone equals the same solve inside a full wavefront of other solves; 64 starts in one call (uniform) equal
    two calls of 32 (per lane); the report names the instantiation each time."""
    mtx, mean = family('eight')
    mtx = np.ascontiguousarray(mtx, dtype=np.int32)
    lo, hi = np.zeros(8), np.ones(8)
    betas, starts = draws_of(mean, 3, 8), opt.start_points(64, lo, hi)
    whole, tr, report = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, 2)
    assert report['instance'] == 'uniform' and report['grid'] == 3
    for e, s in ((1, 37), (2, 63), (0, 0)):
        alone, tr1, report = traced(device_ctx, mtx, betas[e:e + 1], C.TABLE, lo, hi, starts[s:s + 1], -1.0, 2)
        assert report['instance'] == 'per_lane' and report['grid'] == 1
        assert all(np.array_equal(a[0, 0], b[e, s], equal_nan=True) for a, b in zip(alone, whole)), (e, s)
        assert all(C.same(tr1[key][0], tr[key][e * 64 + s]) for key in tr), (e, s)
    halves = [traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts[h:h + 32], -1.0, 2) for h in (0, 32)]
    assert all(half[2]['instance'] == 'per_lane' and half[2]['grid'] == 2 for half in halves)
    for i in range(4):
        assert np.array_equal(np.concatenate([halves[0][0][i], halves[1][0][i]], axis=1), whole[i], equal_nan=True)
    for key in tr:
        both = np.concatenate([half[1][key].reshape((3, 32) + half[1][key].shape[1:]) for half in halves], axis=1)
        assert C.same(both.reshape(tr[key].shape), tr[key]), key


def test_the_edges_of_the_loop(device_ctx):
    mtx, mean = family('two')
    mtx = np.ascontiguousarray(mtx, dtype=np.int32)
    lo, hi = np.zeros(2), np.ones(2)
    betas, starts = draws_of(mean, 2, 3), opt.start_points(5, lo, hi)
    # max_iter = 0: the tests of iteration 0, no step
    (x, f, it, st), tr, _ = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, 0, max_iter=0)
    assert np.all(it == 0) and np.all(st == opt.ITERATION_LIMIT) and np.array_equal(x, np.broadcast_to(starts, x.shape))
    assert np.all(tr['status_tests'] == opt.ITERATION_LIMIT) and np.isnan(tr['alpha']).all() and C.same(f.ravel(), -tr['F'])
    # tol = 0: no solve converges unless its projected gradient is exactly 0; the decisions hold as ever
    (x, f, it, st), tr, _ = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, 4, tol=0.0)
    carried = traced(device_ctx, mtx, betas, C.TABLE, lo, hi, starts, -1.0, 3, tol=0.0)[1]['steepest']
    C.check_decisions(tr, lo, hi, 0.0, 4, MAX_ITER, carried, 'tol = 0')
    assert np.all(np.isin(st, (opt.CONVERGED, opt.STALLED, opt.ITERATION_LIMIT)))
    assert np.all(tr['pg'][tr['status_tests'] == opt.CONVERGED] == 0.0)
    # a model that is only its constant: solved, converged at iteration 0 with f = beta_0
    none = np.zeros((0, 2), dtype=np.int32)
    (x, f, it, st), tr, report = traced(device_ctx, none, np.array([[1.5], [-2.0]]), C.TABLE, lo, hi, starts, -1.0, 0)
    assert np.all(st == opt.CONVERGED) and np.all(it == 0) and f.tolist() == [[1.5] * 5, [-2.0] * 5]
    assert np.array_equal(x, np.broadcast_to(starts, x.shape)) and report['slots'] == 0
    assert np.all(tr['g'] == 0.0) and np.all(tr['H'] == 0.0) and np.all(tr['pg'] == 0.0)
    # an infinite coefficient: non-finite at iteration 0, and that draw alone
    broken = np.concatenate([betas, betas[:1]])
    broken[1, 4] = np.inf
    (x, f, it, st), tr, _ = traced(device_ctx, mtx, broken, C.TABLE, lo, hi, starts, -1.0, 0)
    assert np.all(st[1] == opt.NON_FINITE) and np.all(it[1] == 0) and np.array_equal(x[1], starts)
    assert np.all(tr['status_tests'].reshape(3, 5)[1] == opt.NON_FINITE)
    clean = device_ctx.model_optimize(mtx, betas, C.TABLE, lo, hi, starts, -1.0, MAX_ITER, TOL)
    for a, b in zip((x, f, it, st), clean):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[0])
    assert np.all(st[[0, 2]] != opt.NON_FINITE)


def test_a_refusal_zeroes_the_report(device_ctx):
    mtx, mean = family('two')
    mtx = np.ascontiguousarray(mtx, dtype=np.int32)
    lo, hi = np.zeros(2), np.ones(2)
    betas, starts = draws_of(mean, 2, 3), opt.start_points(5, lo, hi)
    device_ctx.model_optimize(mtx, betas, C.TABLE, lo, hi, starts, -1.0, MAX_ITER, TOL)
    assert device_ctx.optimize_report()['instance'] == 'per_lane'
    for k, sign in ((None, 0.5), (0, 0.5), (-1, -1.0)):
        with pytest.raises(_capi.FoklNativeError):
            device_ctx.model_optimize(mtx, betas, C.TABLE, lo, hi, starts, sign, MAX_ITER, TOL, trace_iteration=k)
        report = device_ctx.optimize_report()
        assert report.pop('instance') == 'none' and set(report.values()) == {0}

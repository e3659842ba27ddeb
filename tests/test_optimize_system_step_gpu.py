"""One iteration of the constrained system optimiser on the MI355X, as the product kernel itself traces it
(system_optimize(p, trace_iteration=k)): the first pass of exact systems bit for bit, a later pass against the rational
reference, every decision -- the Newton step's and the multiplier / penalty update's -- recomputed from the traced values
bit for bit, and the launches beyond one.  tests/optimize_step_cases.py has the references,
tests/test_optimize_step_host.py shows them right on the CPU."""
import numpy as np
import pytest

import optimize_step_cases as C
from test_optimize_system_gpu import prepared
from fokl_gpy_amd import _capi
from fokl_gpy_amd import optimize as opt

pytestmark = pytest.mark.gpu


def traced(ctx, p, k):
    """(results, flat trace of iteration k, report)"""
    out = ctx.system_optimize(p, trace_iteration=k)
    report = ctx.system_optimize_report()
    E, S = p['coef'].shape[0], p['starts'].shape[0]
    assert report['traced'] == 1 and report['solves'] == E * S
    assert report['instance'] == ('uniform' if S % 64 == 0 else 'per_lane')
    assert report['lds_raised'] == int(report['lds_bytes'] > 65536)
    assert report['lds_bytes'] == 512 * opt.system_lds_rows(report['slots'], p['n'], p['K'], len(p['cons']))
    return out[:7], C.flat(out[7]), report


@pytest.mark.parametrize('name', C.EXACT_SYSTEMS)
def test_the_first_pass_is_exact(device_ctx, name):
    """ev, nz, L, its allowance, viol, measure, g and H of iteration 0 equal the host statement's by np.array_equal on
    exact data (lam = 0, rho = 10): an equality with a variable as the objective, ranges with the upper side, the lower
    side and no side active, a tie alone, a range and a tie on one model, a second reader through a map with b != 1."""
    for E, S in ((3, 64), (5, 32), (1, 1)):
        p = C.exact_system(name, E, S)
        system = opt._System(p)
        x0, coef = C.system_first_points(p)
        B, Cn = x0.shape[0], len(p['cons'])
        host = C.host_system_pass(system, x0, coef, np.zeros((2 * Cn, B)), np.full(B, opt.RHO_START))
        _, tr, report = traced(device_ctx, p, 0)
        label = f"{name} {E} x {S}"
        assert tr['running'].all() and np.all(tr['lam'] == 0.0) and np.all(tr['rho'] == opt.RHO_START), label
        assert np.all(tr['inner'] == opt.INNER_START) and np.all(tr['target'] == opt.FEASIBLE_START), label
        for key in ('ev', 'nz', 'F', 'noise', 'viol', 'measure', 'g'):
            assert np.array_equal(tr[key], host[key]), (label, key)
        assert np.array_equal(tr['x_in'], x0), label
        assert np.array_equal(tr['H'], host['H']), (label, np.argwhere(tr['H'] != host['H'])[:5])
        C.check_system_decisions(tr, p, system, 0, np.zeros(B, dtype=bool), label)
        assert report['launches'] == 1 and report['grid'] == -(-B // 64)


def test_the_walk_of_one_small_system(device_ctx):
    """Every k from 0 to the last iteration of the 'eight' system (2 models, a two-sided range), one launch each: the
    decisions of every iteration; x, `steepest`, the multipliers, the penalty, the inner tolerance and the target are
    carried from the exit of k to the entry of k + 1; updates of both kinds occur -- the multipliers move and the
    tolerances shrink, or rho grows -- and the iterate stays in them; at an iteration with lam != 0 and rho > 10 the
    values stay within the rational bound; the returned iterations and status are the trace's."""
    p = prepared('eight', 2, 8)
    system = opt._System(p)
    B = 16
    coef = np.repeat(p['coef'], 8, axis=0)
    plain = device_ctx.system_optimize(p)
    assert device_ctx.system_optimize_report()['traced'] == 0
    x, f, viol, y, mu, iterations, status = (a.reshape((B,) + a.shape[2:]) for a in plain)
    last = int(iterations.max())
    assert 10 <= last <= p['max_iter']
    before, totals, worst, checked = None, dict(good_update=0, penalty_update=0, stepping=0), {}, 0
    for k in range(last + 1):
        results, tr, _ = traced(device_ctx, p, k)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(results, plain)), k   # trace on equals trace off
        assert np.array_equal(tr['running'], iterations >= k), k
        carried = before['steepest'] if before else np.zeros(B, dtype=bool)
        counts = C.check_system_decisions(tr, p, system, k, carried, f"walk k = {k}")
        totals = {key: totals[key] + counts.get(key, 0) for key in totals}
        if before:
            on = tr['running']
            assert np.array_equal(tr['x_in'], before['x_out']), k
            for entry, exit_ in (('lam', 'lam_out'), ('rho', 'rho_out'), ('inner', 'inner_out'), ('target', 'target_out')):
                assert C.same(tr[entry][on], before[exit_][on]), (k, entry)
        ends = tr['running'] & (tr['status'] >= 0)
        assert np.array_equal(ends, iterations == k), k
        # (the kernel turns a limit or a stall with a violation into 'infeasible' after the loop)
        assert np.all((tr['status'][ends] == status[ends]) | (status[ends] == opt.INFEASIBLE)), k
        assert np.array_equal(tr['x_out'][iterations <= k], x[iterations <= k]), k
        later = tr['stepping'] & (tr['rho'] > opt.RHO_START) & np.any(tr['lam'] != 0.0, axis=1)
        if later.any() and checked < 6:
            for b in np.flatnonzero(later)[:3]:
                ratios = C.system_ratios(p, tr['x_in'][b], coef[b], tr['lam'][b], tr['rho'][b],
                                         {key: tr[key][b] for key in ('ev', 'F', 'g', 'H')})
                if ratios is None:
                    continue
                points = C.trial_points(tr['x_in'][b], tr['d'][b], p['lo'], p['hi'], int(tr['trials'][b]))
                refs = [C.fraction_system(p, point, coef[b], tr['lam'][b], tr['rho'][b]) for point in points]
                ratios['Ft'] = max(C.worst_ratio(tr['Ft'][b, h], ref['L'], ref['ML'], C.system_roundings(p))
                                   for h, ref in enumerate(refs))
                worst = {key: max(worst.get(key, 0.0), value) for key, value in ratios.items()}
                checked += 1
        before = tr
    print(f"\n'eight' system, {last + 1} iterations walked: {totals}; N = {C.system_roundings(p)}, {checked} solves with "
          f"lam != 0 and rho > 10, largest error / bound on the device: {worst}")
    assert totals['good_update'] >= 1 and totals['penalty_update'] >= 1 and totals['stepping'] >= last
    assert checked >= 3 and max(worst.values()) <= 1.0, worst


def test_more_than_one_launch(device_ctx):
    """max_iter = 65536 makes a launch 64 solves: three launches for 3 x 64 and for 5 x 32 solves, and -- every solve
    ends before iteration 60 -- the results of the one launch of max_iter = 60, bit for bit."""
    for E, S in ((3, 64), (5, 32)):
        p = prepared('eight', E, S)
        sliced = device_ctx.system_optimize(dict(p, max_iter=65536))
        report = device_ctx.system_optimize_report()
        assert report['launches'] == 3 and report['grid'] == 1 and report['solves'] == E * S, report
        assert report['instance'] == ('uniform' if S == 64 else 'per_lane')
        whole = device_ctx.system_optimize(dict(p, max_iter=60))
        report = device_ctx.system_optimize_report()
        assert report['launches'] == 1 and report['grid'] == -(-E * S // 64), report
        assert whole[5].max() < 60
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(sliced, whole)), (E, S)
        # ... and a trace reaches the later launches' solves as well
        tr = C.flat(device_ctx.system_optimize(dict(p, max_iter=65536), trace_iteration=1)[7])
        one = C.flat(device_ctx.system_optimize(dict(p, max_iter=60), trace_iteration=1)[7])
        assert tr['running'].all() and all(C.same(tr[key], one[key]) for key in tr), (E, S)


def test_invariances_bit_for_bit(device_ctx):
    """A solve alone equals the same solve inside a full wavefront; 64 starts in one call (uniform) equal two calls of 32
    (per lane); the 'sixteen' system's LDS is above 64 KB and the report says that the attribute was set."""
    p = prepared('eight', 3, 64)
    whole, tr, report = traced(device_ctx, p, 2)
    assert report['instance'] == 'uniform' and report['grid'] == 3 and report['lds_raised'] == 0
    for e, s in ((1, 37), (2, 63)):
        alone, tr1, report = traced(device_ctx, dict(p, coef=p['coef'][e:e + 1], starts=p['starts'][s:s + 1]), 2)
        assert report['instance'] == 'per_lane' and report['grid'] == 1
        assert all(np.array_equal(a[0, 0], b[e, s], equal_nan=True) for a, b in zip(alone, whole)), (e, s)
        assert all(C.same(tr1[key][0], tr[key][e * 64 + s]) for key in tr), (e, s)
    halves = [traced(device_ctx, dict(p, starts=p['starts'][h:h + 32]), 2) for h in (0, 32)]
    assert all(half[2]['instance'] == 'per_lane' and half[2]['grid'] == 2 for half in halves)
    for i in range(7):
        assert np.array_equal(np.concatenate([halves[0][0][i], halves[1][0][i]], axis=1), whole[i], equal_nan=True), i
    big = prepared('sixteen', 1, 4)
    device_ctx.system_optimize(big)
    report = device_ctx.system_optimize_report()
    assert report['lds_bytes'] > 65536 and report['lds_raised'] == 1 and report['instance'] == 'per_lane'


def test_a_refusal_zeroes_the_report(device_ctx):
    p = prepared('two', 2, 4)
    device_ctx.system_optimize(p)
    assert device_ctx.system_optimize_report()['instance'] == 'per_lane'
    for k, change in ((None, dict(sign=0.5)), (0, dict(ctol=-1.0)), (-1, {})):
        with pytest.raises(_capi.FoklNativeError):
            device_ctx.system_optimize(dict(p, **change), trace_iteration=k)
        report = device_ctx.system_optimize_report()
        assert report.pop('instance') == 'none' and set(report.values()) == {0}

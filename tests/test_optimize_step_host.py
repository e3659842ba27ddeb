"""The references of tests/test_optimize_step_gpu.py and tests/test_optimize_system_step_gpu.py, shown on the CPU before
anything runs on a device: the exact cases are exact (``optimize._model_parts`` equals ``fractions.Fraction`` arithmetic),
the host statement -- a second double evaluation, in another order of the sums -- stays within the derived rounding bound
of the rational reference, the designed cases of the factorisation and the search end as they are named, and the trace's
fields are where the header says."""
from fractions import Fraction

import numpy as np
import pytest

import optimize_step_cases as C
from test_optimize_gpu import draws_of, family
from fokl_gpy_amd import _capi
from fokl_gpy_amd import optimize as opt


@pytest.mark.parametrize('name', ['one', 'six', 'sixteen'])
def test_the_exact_cases_are_exact_and_meet_every_rule_of_the_active_set(name):
    seen = set()
    for E, S in C.SIZES:
        mtx, betas, starts, lo, hi = C.exact_problem(name, E, S)
        assert np.array_equal(betas, np.round(betas)) and np.abs(betas).max() <= 3
        assert np.array_equal(starts * 8, np.round(starts * 8)) and starts.min() >= 0 and starts.max() <= 1
        if E > 1:
            assert not np.array_equal(betas[0], betas[1])
        if S > 1:
            assert np.all(np.any(starts[1:] != starts[:-1], axis=1))       # a lane off by one reads another start
        x, coef = C.first_points(betas, starts, lo, hi)
        tt = opt.TermTable(mtx)
        assert 3 * tt.n_slots + tt.n_hess + 3 * tt.m <= opt.LDS_ROWS       # the kernel takes it
        for sign in (1.0, -1.0):
            F, noise, g, H = opt._model_parts(tt, C.INT_TABLE, x, coef, 2, scale=sign, weight=sign)
            stride = {'one': 1, 'six': 5, 'sixteen': 7}[name]
            for i in range((E + S) % stride, x.shape[0], stride):
                ref = C.fraction_parts(mtx, C.INT_TABLE, x[i], coef[i], sign)
                assert C.is_exact(F[i], ref['e']) and C.is_exact(noise[i], ref['noise']), (name, E, S, i)
                assert C.is_exact(g[:, i], ref['g']) and C.is_exact(H[:, i], ref['H']), (name, E, S, i)
            active = opt._active_set(x.T, g, lo[:, None], hi[:, None]).T
            seen |= C.rules_seen(x, g.T, active, lo, hi)
    assert seen == C.all_rules(mtx.shape[1], fixed=mtx.shape[1] > 2), C.all_rules(mtx.shape[1], mtx.shape[1] > 2) - seen


def rational_models():
    for name in ('two', 'eight', 'sixteen'):
        yield (name,) + family(name)
    yield 'twenty', C.TWENTY, C.TWENTY_MEAN


@pytest.mark.parametrize('name, mtx, mean', list(rational_models()), ids=lambda v: v if isinstance(v, str) else '')
def test_the_host_statement_stays_within_the_rational_bound(name, mtx, mean):
    """At the host walk's own iterates of k = 0 and k = 3 and at their trial points: the same check the device gets."""
    mtx = np.ascontiguousarray(mtx, dtype=np.int32)
    m = mtx.shape[1]
    lo, hi = np.zeros(m), np.ones(m)
    betas, starts = draws_of(mean, 2, 5), opt.start_points(8, lo, hi)
    walk = C.host_walk(mtx, C.TABLE, betas, starts, lo, hi, -1.0, 60, 1e-10)
    _, coef = C.first_points(betas, starts, lo, hi)
    worst = dict(F=0.0, noise=0.0, g=0.0, H=0.0, Ft=0.0)
    for k in (0, 3):
        rec = walk[k]
        for b in np.flatnonzero(rec['running'])[::5][:3]:
            ratios = C.rational_ratios(mtx, C.TABLE, rec['x_in'][b], coef[b], -1.0, rec['F'][b], rec['noise'][b], rec['g'][b],
                                       rec['H'][b])
            if 'Ft' in rec and rec['stepping'][b]:
                points = C.trial_points(rec['x_in'][b], rec['d'][b], lo, hi, int(rec['trials'][b]))
                ratios['Ft'] = max(C.rational_value_ratio(mtx, C.TABLE, point, coef[b], -1.0, rec['Ft'][b, h])
                                   for h, point in enumerate(points))
            worst = {key: max(worst[key], ratios.get(key, 0.0)) for key in worst}
    print(f"\n{name}: N = {C.roundings(mtx)}, largest error / bound of the host statement: "
          + ', '.join(f"{key} {value:.3f}" for key, value in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_the_designed_hessians_are_what_they_are_named():
    tt = opt.TermTable(C.POWER_MTX)
    for name, (betas, start, lo, hi, want) in C.factor_cases().items():
        lo, hi = np.array(lo), np.array(hi)
        x = np.clip(np.array([start]), lo, hi)
        F, noise, g, H = opt._model_parts(tt, C.POWERS, x, np.array([betas]), 2, weight=1.0)
        assert H.ravel().tolist() == want, name
        factor = H.copy()
        active, d, use = opt._step_direction(x, g, factor, lo, hi, np.zeros(1, dtype=bool))
        floor = opt.PIVOT_FLOOR * max(1.0, max(abs(want[0]), abs(want[2])))
        if name == 'negative pivot':
            assert factor[0, 0] == np.sqrt(2.0) and d[0, 0] * g[0, 0] + d[1, 0] * g[1, 0] < 0
        if name == 'zero pivot':
            assert factor[2, 0] == np.sqrt(opt.PIVOT_FLOOR * 4.0)
        if name == 'pivot on the floor':
            assert want[2] == floor and factor[2, 0] == np.sqrt(floor)
        if name == 'huge diagonal on an active coordinate':
            assert active.ravel().tolist() == [False, True] and factor[0, 0] == np.sqrt(1e-3) and abs(d[0, 0] - 0.1) < 1e-12
        if name.startswith('reach'):
            reach = np.max(np.abs(g.ravel() / 4.0))                # the factor of diag(4, 4) is exact
            assert {'reach below 1': reach < 1, 'reach equal to 1': reach == 1, 'reach above 1': reach > 1}[name]
            assert np.max(np.abs(d)) == min(reach, 1.0)
        assert not use[0]
    # the overflowing cross entry: value and gradient finite, the Newton direction not: steepest descent is selected
    o = C.OVERFLOW
    H = np.array([[2.0], [np.inf], [2.0]])                            # what the kernel forms (the statement's 0 / 1 matrix
    g = np.array([[1e200], [1e200]])                                  # products turn the other entries into NaN)
    active, d, use = opt._step_direction(o['starts'].copy(), g, H, o['lo'], o['hi'], np.zeros(1, dtype=bool))
    assert use[0] and d.ravel().tolist() == [-1.0, -1.0]


def test_the_designed_searches_end_as_they_are_named():
    names, betas, starts, lo, hi = C.search_problem()
    walk = C.host_walk(C.POWER_MTX, C.POWERS, betas, starts, lo, hi, 1.0, 60, 0.0)
    S = len(names)
    at = {name: i * S + i for i, name in enumerate(names)}
    first, second = walk[0], walk[1]
    trials = lambda rec, name: int(rec['trials'][at[name]])
    assert first['stepping'][list(at.values())].all()
    assert trials(first, 'first') == 1 and not first['failed'][at['first']]
    assert trials(first, 'twelfth') == 12 and first['x_out'][at['twelfth'], 0] == 2.0 ** -11
    assert trials(first, 'thirty-first') == 31 and not first['failed'][at['thirty-first']]
    assert first['x_out'][at['thirty-first'], 0] == 2.0 ** -30
    b = at['none, then steepest descent']
    assert first['failed'][b] and not first['use_steepest'][b] and np.array_equal(first['x_out'][b], first['x_in'][b])
    assert second['use_steepest'][b] and not second['failed'][b] and 5 <= trials(second, 'none, then steepest descent') <= 29
    b = at['none twice: stalled']
    assert first['failed'][b] and second['failed'][b] and second['use_steepest'][b] and second['status'][b] == opt.STALLED
    b = at['not moved']
    assert first['failed'][b] and trials(first, 'not moved') == 31 and first['pg'][b] == 2.0 ** -51
    assert np.all(first['Ft'][b] <= first['F'][b])                    # every trial point passes the decrease test ...
    assert np.all(np.array(C.trial_points(first['x_in'][b], first['d'][b], lo, hi, 31)) == first['x_in'][b])   # ... unmoved
    assert second['use_steepest'][b] and not second['failed'][b] and second['x_out'][b, 0] > 1.0
    b = at['clipped in one coordinate']
    assert trials(first, 'clipped in one coordinate') == 1 and first['x_out'][b, 0] == hi[0]
    assert first['x_in'][b, 0] + first['d'][b, 0] > hi[0] and lo[1] < first['x_out'][b, 1] < hi[1]
    assert first['x_out'][b, 1] == first['x_in'][b, 1] + first['d'][b, 1]


def test_a_model_that_is_only_its_constant_converges_at_once():
    mtx = np.zeros((0, 2), dtype=np.int32)
    x, f, it, st = opt.solve_host(mtx, np.array([[1.5], [-2.0]]), C.TABLE, np.zeros(2), np.ones(2),
                                  opt.start_points(3, np.zeros(2), np.ones(2)), -1.0, 60, 1e-10)
    assert np.all(st == opt.CONVERGED) and np.all(it == 0) and f.tolist() == [[1.5] * 3, [-2.0] * 3]


def test_the_trace_fields_are_where_the_header_says():
    m, K, Cn = 3, 2, 1
    h = m * (m + 1) // 2
    stride = 13 + 4 * m + 2 * h + 31 + 2 * K + 4 * Cn + 10
    rows = np.arange(2 * stride, dtype=np.float64).reshape(1, 2, stride)
    rows[0, 1, 4] = 5.0                                                # the active mask: coordinates 0 and 2
    tr = _capi.DeviceContext._step_trace(rows, m, K, Cn)
    assert tr['F'][0, 0] == 1 and tr['pg'][0, 0] == 3 and tr['status_tests'][0, 0] == 5 and tr['trials'][0, 0] == 8
    assert tr['alpha'][0, 0] == 9 and tr['status'][0, 0] == 12 and tr['active'][0, 1].tolist() == [True, False, True]
    at = 13
    for name, width in (('x_in', m), ('g', m), ('H', h), ('factor', h), ('d', m), ('Ft', 31), ('x_out', m), ('ev', K),
                        ('nz', K), ('lam', 2 * Cn)):
        assert tr[name][0, 0].tolist() == list(range(at, at + width)), name
        at += width
    assert [tr[name][0, 0] for name in ('rho', 'inner', 'target', 'viol', 'measure')] == list(range(at, at + 5))
    assert tr['lam_out'][0, 0].tolist() == [at + 7, at + 8] and tr['target_out'][0, 0] == at + 11 == stride - 1
    plain = _capi.DeviceContext._step_trace(rows[..., :13 + 4 * m + 2 * h + 31], m)
    assert 'ev' not in plain and plain['x_out'].shape == (1, 2, m)
    nothing = _capi.DeviceContext._step_trace(np.full((1, 1, 13 + 4 * m + 2 * h + 31), np.nan), m)
    assert not nothing['running'][0, 0] and nothing['status'][0, 0] == -9


# ---------------------------------------------------------------------------------------------------------
# systems
# ---------------------------------------------------------------------------------------------------------

from test_optimize_system_gpu import prepared


@pytest.mark.parametrize('name', C.EXACT_SYSTEMS)
def test_the_exact_systems_are_exact(name):
    """Dyadic maps and power-of-two scales; at lam = 0, rho = 10 ``_System.values``, ``.merit`` and ``.derivatives`` equal
    Fraction arithmetic by the docstring's formulas exactly; the constraint sides are active where the case says."""
    signs = [set() for _ in range(3)]
    for E, S in ((3, 64), (5, 32)):
        p = C.exact_system(name, E, S)
        assert all(C.is_dyadic(a) for a in p['shift'] + p['slope']) and C.is_dyadic(p['starts'])
        assert all(np.log2(c['scale']) == np.round(np.log2(c['scale'])) and C.is_dyadic([c['offset'], c['span']]) for c in p['cons'])
        x, coef = C.system_first_points(p)
        B, Cn = x.shape[0], len(p['cons'])
        lam, rho = np.zeros((2 * Cn, B)), np.full(B, opt.RHO_START)
        host = C.host_system_pass(opt._System(p), x, coef, lam, rho)
        for b in range((E + S) % 3, B, 3):
            ref = C.fraction_system(p, x[b], coef[b], lam[:, b], opt.RHO_START)
            assert C.is_exact(host['ev'][b], ref['ev']) and C.is_exact(host['F'][b], ref['L']), (name, b)
            assert C.is_exact(host['g'][b], ref['g']) and C.is_exact(host['H'][b], ref['H']), (name, b)
            assert C.is_exact(host['viol'][b], ref['viol']) and C.is_exact(host['measure'][b], ref['measure']), (name, b)
        for i, each in enumerate(host['each']):
            signs[i] |= set(np.sign(each[0]).tolist())
    if name == 'ranges':                                              # upper side active, lower side active, inactive
        assert signs == [{1.0}, {-1.0}, {0.0}]
    if name == 'mapped':
        assert any(b != 1.0 for b in p['slope'][1]) and signs[0] == {0.0, 1.0}
    if name in ('tie', 'both'):
        assert p['cons'][-1]['var'] >= 0 and len(p['cons']) == (2 if name == 'both' else 1)
        assert p['cons'][0]['model'] == p['cons'][-1]['model']
    if name == 'equality':
        assert p['obj_var'] == 0 and p['cons'][0]['lo'] == p['cons'][0]['hi']


def test_the_system_statement_stays_within_the_rational_bound():
    """Any (z, lam, rho) is an input of the merit function's formulas: non-dyadic points of the 'eight' system with
    multipliers away from 0 and rho = 1000."""
    p = prepared('eight', 2, 8)
    system = opt._System(p)
    x, coef = C.system_first_points(p)
    B, Cn = x.shape[0], len(p['cons'])
    lam = np.abs(np.random.default_rng(3).standard_normal((2 * Cn, B)))
    rho = np.full(B, 1000.0)
    host = C.host_system_pass(system, x, coef, lam, rho)
    worst, checked = {}, 0
    for b in range(0, B, 3):
        ratios = C.system_ratios(p, x[b], coef[b], lam[:, b], 1000.0, {key: host[key][b] for key in ('ev', 'F', 'g', 'H')})
        if ratios:
            worst = {key: max(worst.get(key, 0.0), value) for key, value in ratios.items()}
            checked += 1
    print(f"\n'eight' system: N = {C.system_roundings(p)}, {checked} points, largest error / bound of the host statement: {worst}")
    assert checked >= 4 and max(worst.values()) <= 1.0


def test_the_walked_system_meets_both_updates_and_the_sliced_one_ends_early():
    out, calls = C.host_system_walk(prepared('eight', 2, 8))
    lam = np.array([call[0] for call in calls[:-1]])                   # [k, 2 C, B]
    rho = np.array([call[1] for call in calls[:-1]])
    assert np.any(np.diff(rho, axis=0) > 0) and np.any((np.diff(lam, axis=0) != 0).any(axis=1))
    assert rho.max() > opt.RHO_START and 10 <= out[5].max() <= 60
    for E, S in ((3, 64), (5, 32)):                                   # every solve ends before iteration 60
        out, _ = C.host_system_walk(prepared('eight', E, S))
        assert out[5].max() < 60 and np.all(out[6] == opt.CONVERGED)

"""dynamics.control_pooled and dynamics.control_cvar on the MI355X past their first pass, device against statement
(dynamics._control_pooled_solve_host, dynamics._control_cvar_solve_host; pinned without a device by the two *_host.py files).

The statement fixes every order of operations, so every comparison of a traced quantity here is bit for bit (``==``, NaN
matching NaN): the first tangent pass as in tests/test_control_pooled_gpu.py and tests/test_control_cvar_gpu.py, and the
TRIAL half of iteration 0, which ``first_trial=True`` brings out of the device after that iteration's last launch -- in
pipeline order the pooled F, noise and g the decision reads, the trial points, slope and moved, every live draw's own cost at
every trial point, the chunk sums of those (pooled) or phi and a of every trial point (CVaR: the risk kernel in its second
form, grid starts x 64), the lane taken and z, status and the descent count after iteration 0.  No quantity needed a
tolerance.  The decision is also recomputed from the device's own traced values with ``dynamics._armijo``.  Lanes 31 and 63 of
the wavefront are no trials: the 62 valid lanes are compared and ``moved`` must be 0 in those two.

Whole solves keep the gates of tests/test_control_pooled_gpu.py (equal status, iterations, descent steps and best start, u
within 1e-9 of the box width, costs within 1e-9 relative) and print max |u - u_host| / width.

1. the trial half at the chunk seams of the pooled sum (1, 63, 64, 65, 130 draws), a search that backtracks, a
   steepest-descent lane, non-finite lanes
2. risk workgroups of 64, 128 and 192 threads, LDS below and above 64 KB, up to the 9 024 draws the kernel takes
3. 1, 10, 11 and 32 decision values (1, 1, 2 and 9 blocks of the CVaR chunk kernel), eight states, one state
4. the regimes of the risk: no band draw, every draw in the band, identical draws, a thin tail, a whole chunk of weight 0"""
import numpy as np
import pytest

import test_control_cvar_gpu as cvar_suite
from assimilate_cases import model
from control_cases import BERN, chain, linear, mixed, product
from fokl_gpy_amd import dynamics, optimize

pytestmark = pytest.mark.gpu

ORDER = ('models', 'states', 'inputs', 'controls', 'forcing', 'y0', 't', 'draws', 'bounds', 'segments', 'control_bounds', 'targets',
         'weights', 'terminal', 'limits', 'limit_weight', 'move_weight', 'previous', 'init', 'starts', 'max_iter', 'tol',
         'draw_weights', 'keep')
DEFAULTS = dict(controls=None, forcing=None, y0=None, t=None, draws=None, bounds=None, segments=8, control_bounds=None, targets=None,
                weights=None, terminal=None, limits=None, limit_weight=1e3, move_weight=None, previous=None, init=None, starts=1,
                max_iter=60, tol=1e-10, draw_weights=None, keep=None)          # control_pooled's own defaults
PRODUCT, MIXED = cvar_suite.PRODUCT, cvar_suite.MIXED
_weights = cvar_suite._weights
FIRST_PASS = ('F_draws', 'g_draws', 'H_draws', 'a', 'phi', 'F', 'q', 'c', 'g', 'H')
# pipeline order: what the decision reads, the trial points, the draws' own trial costs, the sums or the risk, the decision
FIRST_TRIAL = ('reached', 'F', 'noise', 'g', 'trial', 'slope', 'moved', 'idle_moved', 'Ft_draws', 'Ft', 'phi_t', 'a_t', 'lane', 'z',
               'status', 'descent_steps')


def _prepared(args, kw):
    """The prepared problem of ``control_pooled(**args, **kw)``, or of ``control_cvar`` where kw holds alpha."""
    call = {**DEFAULTS, **args, **kw}
    risk = {key: call.pop(key) for key in ('alpha', 'smoothing', 'epsilon') if key in call}
    p = dynamics._prepare_control_pooled(*(call[key] for key in ORDER))
    if risk:
        p.update(zip(('alpha', 'smoothing', 'epsilon'),
                     dynamics._check_cvar(risk['alpha'], risk.get('smoothing', 0.01), risk.get('epsilon'))))
    return p


def _solve(ctx, args, kw, first_trial=False):
    """The native solve and the statement's of one prepared problem -> (device's ``solved``, the statement's, the report)."""
    p = _prepared(args, kw)
    if 'alpha' in p:
        dev, rep = ctx.control_cvar_solve(p, first_trial=first_trial)[0], ctx.control_cvar_report()
        return dev, dynamics._control_cvar_solve_host(p), rep
    dev, rep = ctx.control_pooled_solve(p, first_trial=first_trial)[0], ctx.control_pooled_report()
    return dev, dynamics._control_pooled_solve_host(p), rep


def _same(dev, host, keys, what):
    """Bit for bit in the order of ``keys``: the first key that differs is the finding."""
    for key in keys:
        if key not in host:                                            # F or phi, Ft or phi_t and a_t: by the solver
            assert key not in dev, key
            continue
        a, b = np.asarray(dev[key]), np.asarray(host[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        differ = ~((a == b) | ((a != a) & (b != b)))
        if differ.any():
            at = tuple(np.argwhere(differ)[0])
            print(f"\n{what} {key}: {int(differ.sum())} of {differ.size} values differ, first at {at}: device {a[at]!r} host {b[at]!r}")
        assert not differ.any(), (what, key)


def _first_pass(ctx, args, kw):
    dev, host, rep = _solve(ctx, args, {**kw, 'max_iter': 0})
    assert set(dev['first_pass']) == set(host['first_pass'])
    _same(dev['first_pass'], host['first_pass'], FIRST_PASS, 'first pass')
    for key in ('z', 'cost', 'cost_start', 'status', 'iterations'):
        assert np.array_equal(dev[key], host[key]), key
    assert rep['iterations_queued'] == 1
    return dev, host, rep


def _trial_half(ctx, args, kw):
    """Iteration 0's trial half and what max_iter = 1 returns -> (device's first_trial, the statement's, the report)."""
    dev, host, rep = _solve(ctx, args, {**kw, 'max_iter': 1}, first_trial=True)
    got, want = dev['first_trial'], host['first_trial']
    assert set(got) - {'Ft_chunks'} == set(want)
    if 'Ft_chunks' in got:                                            # what the accept launch adds, in chunk order from the first
        chunks = got['Ft_chunks']
        assert chunks.shape[1] == rep['chunks']
        total = chunks[:, 0]
        with np.errstate(all='ignore'):
            for k in range(1, chunks.shape[1]):
                total = total + chunks[:, k]
        got = {**got, 'Ft': total}
    _same(got, want, FIRST_TRIAL, 'trial half')
    assert want['reached'].any() and not got['idle_moved'].any()
    # the decision from the device's own traced values, and the returned z as that column of the traced trial points
    risk = got['Ft'] if 'Ft' in got else got['phi_t']
    for s in np.flatnonzero(got['reached']):
        lanes = lambda x: x[s][..., np.newaxis]
        chosen, any_ok = dynamics._armijo(lanes(risk), got['F'][s:s + 1], got['noise'][s:s + 1], lanes(got['slope']), lanes(got['moved']))
        lane = int(chosen[0] + (chosen[0] >= 31)) if any_ok[0] else -1
        assert lane == got['lane'][s], (s, lane, got['lane'][s])
        if lane >= 0:
            assert np.array_equal(got['z'][s], got['trial'][s, :, lane // 32, lane % 32]) and got['status'][s] == -1
            assert got['descent_steps'][s] == (lane >= 32)
        else:
            assert got['status'][s] == optimize.STALLED
    for key in ('z', 'status', 'iterations', 'descent_steps'):
        assert np.array_equal(dev[key], host[key]), key
    assert rep['iterations_queued'] == 2
    return got, want, rep


def _whole_cvar(ctx, args, width, **kw):
    return cvar_suite._compare(ctx, args, width, **kw)


# ---------------------------------------------------------------------------------------------------------
# 1. the trial half at the chunk seams
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('case', ['product', 'mixed'])
@pytest.mark.parametrize('solver', ['pooled', 'cvar'])
def test_trial_half_bit_for_bit_across_the_chunk_seams(device_ctx, solver, case, E):
    args, kw = cvar_suite._case(case, E)
    kw.update(starts=2, draw_weights=_weights(E))
    if solver == 'cvar':
        kw.update(alpha=0.8, epsilon=2e-3 if case == 'product' else 5e-4)
    got, want, rep = _trial_half(device_ctx, args, kw)
    assert want['reached'].all() and np.all(want['lane'] >= 0) and rep['chunks'] == -(-E // 64) and rep['draws'] == E
    assert np.isnan(got['Ft_draws']).sum() == (2 * 62 if E > 1 else 0)          # the draw of weight 0 was never evaluated
    assert want['moved'].sum() > 62                                    # trials that move z in both starts


@pytest.mark.parametrize('E', [65, 130])
@pytest.mark.parametrize('solver', ['pooled', 'cvar'])
def test_trial_half_where_the_search_backtracks(device_ctx, solver, E):
    """Binding soft limits make the full Newton step overshoot from most of eight starts: the first passing lane is one of
    1 .. 5, so the decision depends on the risk of lanes that fail -- and on every chunk of the sum the accept launch forms
    itself, which no traced quantity shows (without chunk 0 the trial cost is too small and lane 0 passes)."""
    args, kw = cvar_suite._case('product', E)
    kw.update(starts=8, draw_weights=_weights(E), limits={'x0': (None, 0.42), 'x1': (-0.28, None)}, limit_weight=1e3)
    if solver == 'cvar':
        kw.update(alpha=0.8, epsilon=2e-3)
    _, want, _ = _trial_half(device_ctx, args, kw)
    assert want['reached'].all() and (want['lane'] > 0).sum() >= 5 and want['lane'].max() >= 3 and np.all(want['lane'] < 31)


def test_trial_half_with_a_step_in_a_steepest_descent_lane(device_ctx):
    """tests/test_control_host.py's 1e300-weight system as two identical draws: H overflows, no Newton trial moves z and
    lane 32 is taken.  (Under the CVaR solve this system ends non-finite in iteration 0, in the statement as well: pooled
    only.)"""
    c0, c1 = (float(v) for v in BERN[0])
    one = dict(betas=np.array([[-1e5 / c1 * c0, 1e5 / c1]] * 2), mtx=np.array([[1]]), phis=BERN, minmax=[[0.0, 1.0]],
               kernel='Bernoulli Polynomials')
    args = dict(models=[one], states=['x'], inputs=[['u']], controls=['u'], y0=[0.0], t=(0.0, 0.5, 1.0))
    with np.errstate(over='ignore'):
        got, want, _ = _trial_half(device_ctx, args, dict(bounds=[[-1e9, 1e9]], segments=1, targets={'x': 1e5 + 1.0},
                                                          weights={'x': 1e300}, init=[[0.9999]]))
    assert want['lane'].tolist() == [32] and got['z'].tolist() == [[1.0]] and not want['moved'][0, 0].any()


@pytest.mark.parametrize('solver', ['pooled', 'cvar'])
def test_trial_half_with_lanes_whose_cost_is_not_finite(device_ctx, solver):
    """Draw 1 (weight 1e-300) is 1e158 x a cubic in u that is flat at the start u = 0.5: its cost is finite there and
    overflows in the far steepest-descent lanes, so the pooled trial cost is inf and phi_t NaN in those lanes and they fail;
    the nearer lanes are finite and fail the Armijo test; the start stalls, on the device as in the statement."""
    k, s1, s3 = 1e158, float(BERN[0][1]), float(BERN[2][3])
    two = dict(betas=np.array([[0.3, 1.0, 0.0], [0.0, 0.25 * k * s3 / s1, k]]), mtx=np.array([[1], [3]]), phis=BERN, minmax=[[0.0, 1.0]],
               kernel='Bernoulli Polynomials')
    args = dict(models=[two], states=['x'], inputs=[['u']], controls=['u'], y0=[0.0], t=(0.0, 0.5, 1.0))
    kw = dict(bounds=[[-1e200, 1e200]], segments=1, targets={'x': 0.0}, init=[[0.5]], draw_weights=[1.0, 1e-300])
    if solver == 'cvar':
        kw.update(alpha=0.5, epsilon=1e-3)
    with np.errstate(all='ignore'):
        got, want, _ = _trial_half(device_ctx, args, kw)
    risk = want['Ft'] if solver == 'pooled' else want['phi_t']
    bad = ~np.isfinite(risk[0, 1])
    assert 0 < bad.sum() < 31 and want['moved'][0, 1].all() and want['lane'].tolist() == [-1]
    assert np.isfinite(want['Ft_draws'][0, 0]).all() and np.array_equal(~np.isfinite(want['Ft_draws'][0, 1, 1]), bad)
    assert got['status'].tolist() == [optimize.STALLED]


# ---------------------------------------------------------------------------------------------------------
# 2. wide risk workgroups
# ---------------------------------------------------------------------------------------------------------

WIDE = dict(segments=2, targets={'x0': 0.6, 'x1': -0.2}, move_weight={'u': 1e-3}, init=np.array([[1.0, 2.5]]), starts=2, alpha=0.9,
            epsilon=5e-4)
#        E: (chunks, risk_threads, risk_lds_bytes)
WIDE_PLAN = {4032: (63, 64, 65536), 4033: (64, 64, 66560), 4096: (64, 64, 66560), 4097: (65, 128, 68608), 8193: (129, 192, 135168),
             9024: (141, 192, 147456)}


def _wide(E):
    return product(E, 4, spread=0.3), dict(WIDE, draw_weights=_weights(E))


def _assert_plan(rep, E):
    chunks, threads, lds = WIDE_PLAN[E]
    assert lds == (2 * 64 * chunks + 2 * threads) * 8
    assert (rep['draws'], rep['chunks'], rep['risk_threads'], rep['risk_lds_bytes']) == (E, chunks, threads, lds)
    assert rep['starts'] == 2 and rep['D'] == 2 and rep['NS'] == 2


@pytest.mark.parametrize('E', sorted(WIDE_PLAN))
def test_wide_risk_workgroups_first_pass(device_ctx, E):
    """64, 128 and 192 threads; 65 536 bytes of LDS is the last launch without the attribute, 66 560 the first with it."""
    args, kw = _wide(E)
    _, host, rep = _first_pass(device_ctx, args, kw)
    _assert_plan(rep, E)
    first, live = host['first_pass'], kw['draw_weights'] != 0
    for s in range(2):
        q, c = first['q'][s], first['c'][s]
        below, band, full = int(((q == 0) & live).sum()), int((c != 0).sum()), int(((q != 0) & (c == 0)).sum())
        print(f"\n{E} draws, start {s}: {below} live draws with q = 0, {band} in the band, {full} with r = 1")
        assert below > 0 and band > 0 and full > 0
    assert len(set((np.flatnonzero(first['c'][0] != 0) // 64).tolist())) > 60           # band draws in (nearly) every chunk


@pytest.mark.parametrize('E', [4097, 9024])
def test_wide_risk_workgroups_trial_half(device_ctx, E):
    args, kw = _wide(E)
    got, want, rep = _trial_half(device_ctx, args, kw)
    _assert_plan(rep, E)
    assert want['reached'].all() and np.all(want['lane'] >= 0) and np.isfinite(want['phi_t']).all()


def test_wide_risk_workgroups_whole_solve(device_ctx):
    args, kw = _wide(4097)
    dev, _ = _whole_cvar(device_ctx, args, [4.0], **{**kw, 'starts': 1})
    rep = device_ctx.control_cvar_report()
    assert rep['risk_threads'] == 128 and rep['chunks'] == 65 and dev.iterations > 1 and dev.status == optimize.CONVERGED


def test_one_draw_more_than_the_risk_kernel_holds_is_refused(device_ctx):
    from fokl_gpy_amd._capi import FoklNativeError
    args, kw = _wide(9025)
    p = _prepared(args, {**kw, 'max_iter': 0})
    want = (2 * 64 * 142 + 2 * 192) * 8
    with pytest.raises(FoklNativeError, match=rf"\(2 x 64 x ceil\(draws / 64\) \+ 2 x threads\) x 8 = {want} bytes for 9025 draws, "
                                              r"the limit is 147456"):
        device_ctx.control_cvar_solve(p)
    assert set(device_ctx.control_cvar_report().values()) == {0}


# ---------------------------------------------------------------------------------------------------------
# 3. decision values and states under CVaR
# ---------------------------------------------------------------------------------------------------------

#   D: (controls, segments, steps, blocks of the chunk kernel)
DECISIONS = {1: (1, 1, 6, 1), 10: (2, 5, 10, 1), 11: (1, 11, 11, 2), 32: (2, 16, 16, 9)}


def _decisions(D):
    nc, segments, steps, blocks = DECISIONS[D]
    assert nc * segments == D and -(-(3 + 2 * D + 2 * D * D) // 256) == blocks
    args = linear(65, steps, nc, spread=0.05)
    kw = dict(segments=segments, targets={'x0': 0.5, 'x1': -0.2}, move_weight={name: 0.01 for name in args['controls']},
              previous=[0.0, 0.1][:nc], starts=2, draw_weights=_weights(65), alpha=0.8, smoothing=0.05)
    return args, kw, [2.0] * nc


@pytest.mark.parametrize('D', sorted(DECISIONS))
def test_decision_values_first_pass_and_trial_half(device_ctx, D):
    args, kw, _ = _decisions(D)
    _, host, rep = _first_pass(device_ctx, args, kw)
    assert rep['D'] == D and rep['chunks'] == 2 and rep['step_lds_bytes'] == (4 + D) * 64 * 8
    band = np.flatnonzero(host['first_pass']['c'][0] != 0)
    assert band.size > 0
    if D <= 11:
        assert set((band // 64).tolist()) == {0, 1}                    # band draws in both chunks
    got, want, _ = _trial_half(device_ctx, args, kw)
    assert want['reached'].all() and got['trial'].shape == (2, D, 2, 31)


@pytest.mark.parametrize('D', sorted(DECISIONS))
def test_decision_values_whole_solve(device_ctx, D):
    args, kw, width = _decisions(D)
    dev, _ = _whole_cvar(device_ctx, args, width, **kw)
    assert dev.status == optimize.CONVERGED and 1 < dev.iterations < 10 and device_ctx.control_cvar_report()['D'] == D


def test_eight_states_one_decision_value(device_ctx):
    args = chain(8, 65, 6)
    kw = dict(segments=1, targets={'x0': 0.1, 'x7': 0.0}, starts=2, draw_weights=_weights(65), alpha=0.8, smoothing=0.05)
    _, _, rep = _first_pass(device_ctx, args, kw)
    assert rep['NS'] == 8 and rep['D'] == 1
    _trial_half(device_ctx, args, kw)
    dev, _ = _whole_cvar(device_ctx, args, [10.0], **kw)
    assert dev.status == optimize.CONVERGED and dev.iterations > 0


def test_one_state(device_ctx):
    """One order-1 Bernoulli model of (x0, u0): the kernels' NS = 1 instances."""
    a = model('b', [0.1, -0.8, 1.2], np.eye(2, dtype=int), [[-4.0, 4.0], [-1.0, 1.0]], 65, np.random.default_rng(23), 0.05)
    args = dict(models=[a], states=['x0'], inputs=[['x0', 'u0']], controls=['u0'], y0=[0.2], t=(0.0, 7.5 * 0.1, 0.1))
    kw = dict(segments=4, targets={'x0': 0.5}, move_weight={'u0': 0.01}, previous=[0.0], starts=2, draw_weights=_weights(65), alpha=0.8,
              smoothing=0.05)
    _, _, rep = _first_pass(device_ctx, args, kw)
    assert rep['NS'] == 1 and rep['D'] == 4
    _trial_half(device_ctx, args, kw)
    dev, _ = _whole_cvar(device_ctx, args, [2.0], **kw)
    assert dev.status == optimize.CONVERGED and dev.iterations > 1


# ---------------------------------------------------------------------------------------------------------
# 4. regimes of the risk, all at 130 draws
# ---------------------------------------------------------------------------------------------------------

def _regime(E=130):
    args, kw = cvar_suite._case('product', E)
    kw.update(starts=2, alpha=0.8, epsilon=2e-3, draw_weights=_weights(E))
    return args, kw


def test_regime_no_draw_in_the_band(device_ctx):
    """128 live draws of equal weight (two of weight 0 among them, one per chunk): the weights normalise to exactly 1 / 128,
    alpha = 0.875 puts exactly 16 draws in the tail and eps lies far below the smallest gap between costs, so c = 0, H is the
    q-weighted sum alone and the step kernel takes its ``sc == 0`` branch."""
    args, kw = _regime()
    w = np.ones(130)
    w[[17, 100]] = 0.0
    kw.update(draw_weights=w, alpha=0.875, epsilon=1e-12)
    _, host, _ = _first_pass(device_ctx, args, kw)
    first = host['first_pass']
    assert np.all(first['c'] == 0) and np.all((first['q'] != 0).sum(axis=1) == 16) and np.all(first['q'][first['q'] != 0] == 1 / 16)
    live = np.flatnonzero(w)
    gaps = np.diff(np.sort(first['F_draws'][:, live], axis=1), axis=1)
    assert gaps.min() > 1e3 * 1e-12
    Hq = dynamics._pooled_sum_each(np.moveaxis(first['H_draws'], 0, -1), first['q'].T)          # [E, D, D, S], q [E, S]
    assert np.array_equal(np.moveaxis(Hq, -1, 0), first['H'])
    _trial_half(device_ctx, args, kw)


def test_regime_every_live_draw_in_the_band(device_ctx):
    args, kw = _regime()
    kw.update(epsilon=1.0)
    _, host, _ = _first_pass(device_ctx, args, kw)
    assert np.all((host['first_pass']['c'] != 0).sum(axis=1) == 129)
    _trial_half(device_ctx, args, kw)


def test_regime_130_copies_of_one_draw(device_ctx):
    """Every cost is the same F: the bisection ends in a bracket of width eps below F and a = F - m eps to rounding."""
    args, kw = _regime(1)
    args['models'] = [dict(m, betas=np.repeat(m['betas'], 130, axis=0)) for m in args['models']]
    kw.update(draw_weights=_weights(130))
    _, host, _ = _first_pass(device_ctx, args, kw)
    first = host['first_pass']
    F = first['F_draws'][:, 0]
    assert np.all(first['F_draws'][:, np.flatnonzero(kw['draw_weights'])] == F[:, np.newaxis])
    assert np.all(np.abs(first['a'] - (F - 0.2 * 2e-3)) <= 1e-12) and np.all((first['c'] != 0).sum(axis=1) == 129)
    _trial_half(device_ctx, args, kw)


def test_regime_a_thin_tail(device_ctx):
    """alpha = 0.999: m lies below the smallest live weight, exactly one draw is in the band and none beyond it."""
    args, kw = _regime()
    kw.update(alpha=0.999)
    _, host, _ = _first_pass(device_ctx, args, kw)
    w = kw['draw_weights'] / kw['draw_weights'].sum()
    first = host['first_pass']
    assert 1.0 - 0.999 < w[w > 0].min() and np.all((first['c'] != 0).sum(axis=1) == 1) and np.all((first['q'] != 0).sum(axis=1) == 1)
    _trial_half(device_ctx, args, kw)


def test_regime_a_whole_chunk_of_weight_zero(device_ctx):
    """Draws 64 .. 127 weigh nothing: chunk 1's sums are 0.0 and nothing else changes when those draws turn to NaN."""
    args, kw = _regime()
    w = kw['draw_weights'].copy()
    w[64:128] = 0.0
    kw.update(draw_weights=w)
    dev, host, _ = _first_pass(device_ctx, args, kw)
    assert np.isfinite(host['first_pass']['H']).all() and np.isfinite(host['first_pass']['phi']).all()
    got, _, _ = _trial_half(device_ctx, args, kw)
    quiet = cvar_suite._with_nan_draws(args, np.arange(64, 128))
    dev_nan, _, _ = _first_pass(device_ctx, quiet, kw)
    got_nan, _, _ = _trial_half(device_ctx, quiet, kw)
    for key in ('phi', 'a', 'q', 'c', 'g', 'H'):
        assert np.array_equal(dev_nan['first_pass'][key], dev['first_pass'][key]) and np.isfinite(dev['first_pass'][key]).all(), key
    for key in ('trial', 'slope', 'moved', 'phi_t', 'a_t', 'lane', 'z', 'Ft_draws'):
        assert np.array_equal(got_nan[key], got[key], equal_nan=True), key
    assert np.isfinite(got['phi_t']).all() and np.isnan(got['Ft_draws'][:, 64:128]).all()

"""dynamics.simulate_adaptive_host, the statement the device kernel is tested against (tests/test_simulate_adaptive_gpu.py):
a forced level against simulate_host on the refined grid bit for bit, a stiff linear model against its closed form, the
tolerance in the record, the kink at the wall of the box, a NaN member, the bookkeeping and every refusal -- none of which
needs a device."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from helpers import GOLDEN
from fokl_gpy_amd import _capi, dynamics, getKernels

BERN = getKernels.bernoulli()
SPLINES = getKernels.table_to_phis(np.load(os.path.join(GOLDEN, 'spline_phis.npz'))['table'])
RECORD = ('first_saturation', 'pairs', 'rejected', 'max_level', 'error', 'first_unresolved')


class _Reached(Exception):
    pass


class _NoDevice(_capi.DeviceContext):
    """Stands where the device context would be: a refused call must not reach the launch, a well-formed one ends here."""

    def __init__(self, expect_launch=False):
        self._h = None
        self.expect_launch = expect_launch

    def simulate_adaptive(self, p):
        if not self.expect_launch:
            pytest.fail("a refused call reached the launch")
        raise _Reached(p)


def _bern_model(betas, mtx, minmax):
    return dict(betas=np.asarray(betas, dtype=np.float64), mtx=np.asarray(mtx), phis=BERN, minmax=minmax,
                kernel='Bernoulli Polynomials')


def two_state_system(steps=24, h=0.0625, draws=6):
    """tests/test_simulate_host.py's two-state system (d T/dt reads T, c, u; d c/dt reads c, u, T) on a dyadic grid whose
    refinements np.arange reproduces exactly."""
    rng = np.random.default_rng(3)
    first = _bern_model(0.2 * rng.standard_normal((draws, 5)), [[1, 0, 0], [0, 2, 0], [0, 0, 1], [1, 1, 0]],
                        [[0.0, 2.0], [-1.0, 1.0], [0.0, 10.0]])
    by_name = {'T': ([0.5, 2.5], [1, 0, 2, 0, 1]), 'c': ([-2.0, 2.0], [0, 3, 1, 0, 0]), 'u': ([-5.0, 20.0], [0, 0, 0, 2, 1])}
    order = ['c', 'u', 'T']
    second = _bern_model(0.2 * rng.standard_normal((draws, 6)), np.stack([by_name[name][1] for name in order], axis=1),
                         [by_name[name][0] for name in order])
    u = 5.0 + 4.0 * np.sin(np.arange(steps) / 4.0)
    return dict(models=[first, second], states=['T', 'c'], inputs=[['T', 'c', 'u'], order], forcing={'u': u}, y0=[1.0, 0.1],
                t=(0.0, steps * h, h))


def spline_system():
    rng = np.random.default_rng(5)
    model = dict(betas=np.array([0.1, 0.8, -0.5]) * (1 + 0.2 * rng.standard_normal((4, 3))), mtx=np.array([[1], [2]]),
                 phis=SPLINES, minmax=[[0.0, 2.0]], kernel='Cubic Splines')
    return dict(models=[model], states=['y'], inputs=[['y']], y0=[0.7], t=(0.0, 12 * 0.0625, 0.0625))


def outside_system():
    """The second case of test_first_saturation_is_the_step_that_reaches_the_edge on a dyadic grid: member 1 starts outside
    the model's range of its state, far from the box."""
    model = _bern_model([[0.01, 0.02]], [[1]], [[0.0, 1.0]])
    return dict(models=[model], states=['y'], inputs=[['y']], y0=[[0.5], [1.25]], t=(0.0, 0.375, 0.125), bounds=[[-10.0, 10.0]],
                ReturnBounds=False)


def wall_system():
    """One member that integrates into the wall of its box: dy/dt = 0.6 + 3 B1(y) grows from 0.5 until it meets 1."""
    model = _bern_model([[0.6, 3.0]], [[1]], [[0.0, 1.0]])
    return dict(models=[model], states=['y'], inputs=[['y']], y0=[0.5], t=(0.0, 2.0, 0.125), bounds=[[0.0, 1.0]],
                ReturnBounds=False)


def stiff_linear(rates, y0=1.0, h=0.0625, steps=32, lo=0.0, hi=4.0):
    """dy/dt = a + b y as one order-1 Bernoulli model per draw, b h = rates[e], fixed point 2 -> (arguments, [b as Fraction],
    [fixed point as Fraction]) from the very doubles the model holds."""
    c0, c1 = (float(v) for v in BERN[0])
    betas = []
    for bh in rates:
        b = bh / h
        beta1 = b * (hi - lo) / c1
        betas.append([-2.0 * b - beta1 * c0, beta1])
    model = _bern_model(betas, [[1]], [[lo, hi]])
    F = Fraction
    b = [F(row[1]) * F(c1) / (F(hi) - F(lo)) for row in betas]
    a = [F(row[0]) + F(row[1]) * (F(c0) - F(c1) * F(lo) / (F(hi) - F(lo))) for row in betas]
    args = dict(models=[model], states=['y'], inputs=[['y']], y0=np.broadcast_to(y0, (len(rates),))[:, None] if np.ndim(y0) else [y0],
                t=(0.0, steps * h, h))
    return args, b, [-ai / bi for ai, bi in zip(a, b)]


def refined(args, L):
    """The arguments of the fixed-step run a forced level L must reproduce: step h / 2^(L + 1), every forcing row repeated."""
    n = 2 ** (L + 1)
    start, stop, h = args['t']
    forcing = {name: np.repeat(values, n) for name, values in (args.get('forcing') or {}).items()}
    return {**args, 't': (start, stop, h / n), 'forcing': forcing}, n


# ---------------------------------------------------------------------------------------------------------
# 1. a forced level is the refined fixed-step run
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('system, levels', [(two_state_system, (0, 1, 3)), (spline_system, (0, 1, 3)), (outside_system, (0, 2)),
                                            (wall_system, (0, 2))])
def test_forced_level_equals_the_refined_fixed_step_run(system, levels):
    args = system()
    for L in levels:
        fine_args, n = refined(args, L)
        fine = dynamics.simulate_host(**fine_args, keep='members')
        got = dynamics.simulate_adaptive_host(**args, keep=('members', 'levels'), min_halvings=L, max_halvings=L)
        steps = got.t.shape[0] - 1
        assert fine.t.shape[0] == steps * n + 1 and np.array_equal(fine.t[::n], got.t)
        assert got.members.shape == fine.members[:, :, ::n].shape
        assert np.array_equal(got.members, fine.members[:, :, ::n])
        assert np.array_equal(got.pairs, np.full(got.members.shape[0], steps * 2 ** L)) and got.pairs.dtype == np.int64
        assert not got.rejected.any() and got.rejected.dtype == np.int64
        assert got.first_saturation.dtype == np.int32 and np.array_equal(got.first_saturation, fine.first_saturation // n)
        assert (got.max_level == L).all() and (got.levels == L).all()
    if system is outside_system:
        assert got.first_saturation.tolist() == [-1, 0]
    if system is wall_system:
        assert got.first_saturation[0] > 0 and got.members[0, 0, -1] >= 1.0 - 1e-9 and got.first_unresolved[0] >= 0


# ---------------------------------------------------------------------------------------------------------
# 2. it does what it is for
# ---------------------------------------------------------------------------------------------------------

def test_a_stiff_member_is_resolved_where_the_fixed_step_fails():
    """dy/dt = a + b y, range [0, 4], fixed point 2, y0 = 1, h = 0.0625, 32 steps: b h = -3.2 and half that rate, against
    fp + (y0 - fp) exp(b t).  The adaptive error is within the sum of the accepted local tolerances (the system contracts and
    |y| <= 2); measured here: 8.4e-7 against about 1e-4.  The fixed step errs by 0.57 and 0.068."""
    rtol, atol = 1e-6, 1e-9
    args, b, fixed = stiff_linear([-3.2, -1.6])
    res = dynamics.simulate_adaptive_host(**args, keep='members', rtol=rtol, atol=atol)
    plain = dynamics.simulate_host(**args, keep='members')
    t = res.t
    for e in range(2):
        want = np.array([float(fixed[e]) + (1.0 - float(fixed[e])) * math.exp(float(b[e] * Fraction(float(ti)))) for ti in t])
        err = np.max(np.abs(res.members[e, 0] - want))
        bound = res.pairs[e] * (atol + rtol * 2)
        print(f"\ndraw {e}: b h = {float(b[e]) * 0.0625:.2f}, adaptive error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}; "
              f"pairs {res.pairs[e]}, rejected {res.rejected[e]}, max level {res.max_level[e]}; fixed-step error "
              f"{np.max(np.abs(plain.members[e, 0] - want)):.3f}")
        assert err <= bound
        assert np.max(np.abs(plain.members[e, 0] - want)) > 0.05
    assert res.first_saturation.tolist() == [-1, -1] and res.first_unresolved.tolist() == [-1, -1]
    assert res.saturated_fraction == 0.0 and res.unresolved_fraction == 0.0
    assert res.max_level[0] != res.max_level[1] and (res.rejected > 0).any()


# ---------------------------------------------------------------------------------------------------------
# 3. the tolerance is obeyed in the record
# ---------------------------------------------------------------------------------------------------------

def test_tolerance_is_obeyed_in_the_record():
    """Four draws of the stiff linear family (a contracting system, so accepted local errors do not grow) from different
    initial states, free between levels 0 and 7 and forced to level 7."""
    args, _, _ = stiff_linear([-0.5, -1.6, -3.2, -6.0], y0=np.array([1.0, 0.5, 3.0, 1.5]), steps=16)
    free = dynamics.simulate_adaptive_host(**args, keep='members', max_halvings=7)
    assert (free.first_unresolved == -1).all() and (free.rejected > 0).any() and len(set(free.max_level.tolist())) > 1
    assert np.all(free.error[free.first_unresolved == -1] <= 1.0) and np.all(free.error > 0.0)
    tight = dynamics.simulate_adaptive_host(**args, rtol=1e-8, max_halvings=7)
    print(f"\npairs at rtol 1e-6 {free.pairs.tolist()}, at rtol 1e-8 {tight.pairs.tolist()}; error {free.error.tolist()}")
    assert np.all(tight.pairs >= free.pairs) and (tight.pairs > free.pairs).any()
    forced = dynamics.simulate_adaptive_host(**args, keep='members', min_halvings=7, max_halvings=7)
    sc = free.atol[:, None] + free.rtol * np.max(np.abs(free.members), axis=2).T       # [state, member]
    bound = free.pairs * np.max(sc, axis=0)
    distance = np.max(np.abs(free.members - forced.members), axis=(1, 2))
    print(f"free against level 7: distance {distance.tolist()}, bound {bound.tolist()}")
    assert np.all(distance <= bound) and np.all(distance > 0)


# ---------------------------------------------------------------------------------------------------------
# 4. the kink is reported
# ---------------------------------------------------------------------------------------------------------

def test_the_wall_of_the_box_is_reported_as_unresolved():
    res = dynamics.simulate_adaptive_host(**wall_system(), keep=('members', 'levels'), max_halvings=6)
    y = res.members[0, 0]
    reaches = int(np.flatnonzero(y[1:] >= 1.0)[0])                    # the step that takes the member to the wall
    print(f"\nthe wall is reached in step {reaches}; first_unresolved {res.first_unresolved[0]}, first_saturation "
          f"{res.first_saturation[0]}, max level {res.max_level[0]}, error {res.error[0]:.3e}, pairs {res.pairs[0]}")
    assert res.first_unresolved.tolist() == [reaches] and res.unresolved_fraction == 1.0
    assert res.max_level.tolist() == [6] and res.levels[0, reaches] == 6
    assert res.error[0] > 1.0 and np.all(y[reaches + 1:] == y[reaches + 1])


# ---------------------------------------------------------------------------------------------------------
# 5. a NaN member ends and stays local
# ---------------------------------------------------------------------------------------------------------

def nan_system(draws=3, nan_draws=(1,), ReturnBounds=False):
    """The two-state system with a NaN coefficient in the second model of the draws ``nan_draws``: those members are NaN
    from their first step on.  With more draws and ``ReturnBounds`` the band is formed next to them."""
    args = two_state_system(steps=4, draws=draws)
    args['models'][1]['betas'][list(nan_draws), 2] = np.nan
    return dict(args, ReturnBounds=ReturnBounds, max_halvings=5)


def test_a_nan_member_ends_and_stays_local():
    args = nan_system()
    res = dynamics.simulate_adaptive_host(**args, keep=('members', 'levels'))
    assert res.first_unresolved.tolist() == [-1, 0, -1] and np.isfinite(res.error).all()
    assert res.max_level[1] == 5 and res.pairs[1] == 4 * 2 ** 5 and np.isnan(res.members[1, :, 1:]).any()
    for e in (0, 2):
        alone = dynamics.simulate_adaptive_host(**args, draws=np.array([e]), keep=('members', 'levels'))
        assert np.array_equal(alone.members[0], res.members[e]) and np.array_equal(alone.levels[0], res.levels[e])
        for key in RECORD:
            assert alone[key][0] == res[key][e], key


# ---------------------------------------------------------------------------------------------------------
# 6. bookkeeping
# ---------------------------------------------------------------------------------------------------------

def test_bookkeeping():
    """The two-state system with ten times the coefficients: members that reject, relax and meet the box."""
    args = two_state_system(steps=10)
    for model in args['models']:
        model['betas'] = 10.0 * model['betas']
    state = np.random.get_state()[1].copy()
    five = dynamics.simulate_adaptive_host(**args, draws=np.arange(5), keep=('members', 'levels'), rtol=1e-9)
    assert np.array_equal(np.random.get_state()[1], state)           # nothing is drawn
    for e in range(5):
        alone = dynamics.simulate_adaptive_host(**args, draws=np.array([e]), keep=('members', 'levels'), rtol=1e-9,
                                                ReturnBounds=False)
        assert np.array_equal(alone.members[0], five.members[e]) and np.array_equal(alone.levels[0], five.levels[e])
        for key in RECORD:
            assert alone[key][0] == five[key][e] and alone[key].dtype == five[key].dtype, key
    assert five.levels.shape == (5, 10) and five.levels.dtype == np.int8
    assert np.array_equal(five.levels.max(axis=1), five.max_level) and five.max_level.dtype == np.int32
    assert (five.rejected > 0).any() and len(set(five.max_level.tolist())) > 2     # the members differ in what they need
    # a step's pairs number at least one and at most 2^(its deepest level): coarser pairs inside it only lower the count
    filled = np.sum(2 ** five.levels.astype(np.int64), axis=1)
    assert np.all(10 <= five.pairs) and np.all(five.pairs <= filled) and np.all(filled <= 10 * 2 ** five.max_level.astype(np.int64))
    # ... with equality where the level is forced
    forced = dynamics.simulate_adaptive_host(**args, keep='levels', min_halvings=2, max_halvings=2)
    assert np.array_equal(np.sum(2 ** forced.levels.astype(np.int64), axis=1), forced.pairs)
    assert 'members' not in forced and 'levels' not in dynamics.simulate_adaptive_host(**args, keep='members')
    for key in ('t', 'mean', 'bounds', 'first_saturation', 'saturated_fraction', 'unresolved_fraction'):
        assert key in forced


# ---------------------------------------------------------------------------------------------------------
# 7. refusals: each before any launch, with a message that names the limit
# ---------------------------------------------------------------------------------------------------------

def test_refusals_name_the_limit_and_launch_nothing():
    model = _bern_model([[0.1, 0.2, 0.1], [0.1, 0.3, 0.2]], [[1, 0], [0, 1]], [[0.0, 1.0], [0.0, 5.0]])
    good = dict(models=[model], states=['y'], inputs=[['y', 'u']], forcing={'u': np.ones(10)}, y0=[0.5], t=(0.0, 1.0, 0.1))

    def refused(match, **changes):
        with pytest.raises(ValueError, match=match):
            dynamics.simulate_adaptive(**{**good, **changes}, device=_NoDevice())

    with pytest.raises(_Reached) as hit:
        dynamics.simulate_adaptive(**good, keep=('levels', 'members'), device=_NoDevice(expect_launch=True))
    p = hit.value.args[0]
    assert p['E'] == 2 and p['want_members'] and p['want_levels'] and (p['min_halvings'], p['max_halvings']) == (0, 10)
    assert p['rtol'] == 1e-6 and p['atol'].tolist() == [1e-9 * 1.0]  # the box is the training range [0, 1]
    for bad in (np.nan, np.inf, -1e-6):
        refused('rtol must be finite and not negative', rtol=bad)
    for bad in (-1e-9, np.nan, np.inf, [1e-9, -1.0]):
        refused('atol', atol=bad)
    refused('atol must be finite and not negative', atol=-1e-9)
    refused(r'atol needs one value per state \(1\)', atol=[1e-9, 1e-9])
    refused('rtol == 0 needs a positive atol', rtol=0.0, atol=0.0)
    for low, top in ((-1, 3), (4, 3), (0, 13), (13, 13)):
        refused('0 <= min_halvings <= max_halvings <= 12', min_halvings=low, max_halvings=top)
    refused('must be integers', max_halvings=2.5)
    refused('must be integers', min_halvings='1')
    for bad in ('particles', ('members', 'members'), ('members', 'levels', 'members'), (), 3):
        refused("keep must be None, 'members', 'levels' or a tuple", keep=bad)
    # a state no model reads has an unbounded box: the default atol does not exist
    free = _bern_model([[0.1, 0.2], [0.1, 0.3]], [[1]], [[0.0, 5.0]])
    unbounded = dict(models=[free], states=['y'], inputs=[['u']])
    refused("state 'y': its box is unbounded.*pass atol", **unbounded)
    with pytest.raises(_Reached):
        dynamics.simulate_adaptive(**{**good, **unbounded}, atol=1e-9, device=_NoDevice(expect_launch=True))
    with pytest.raises(_Reached):                                     # rtol == 0 alone is a pure absolute tolerance
        dynamics.simulate_adaptive(**good, rtol=0.0, device=_NoDevice(expect_launch=True))
    # what simulate refuses, with simulate's message
    refused('at least one fitted model', models=[])
    refused('not a fitted model', models=[object()])
    refused("'w' is neither a state", inputs=[['y', 'w']])
    refused(r'models\[0\] has 2 input columns .* names 1', inputs=[['y']])
    refused(r"forcing\['u'\] has 9 values but 10 steps", forcing={'u': np.ones(9)})
    refused('y0 holds NaN', y0=[np.nan])
    refused(r"forcing\['u'\] holds NaN", forcing={'u': np.r_[np.ones(9), np.nan]})
    refused("state 'y': its box is empty", bounds=[[1.0, 1.0]])
    refused('at least 2 members', draws='mean')
    refused('at most 16384 members', draws='mean', y0=np.full((16385, 1), 0.5))
    refused('draws', draws=2.5)
    one = _bern_model(np.full((2, 2), 0.1), [[1]], [[0.0, 1.0]])
    names = [f's{k}' for k in range(9)]
    refused('at most 8 states, the system has 9', models=[one] * 9, states=names, inputs=[[n] for n in names],
            y0=np.full(9, 0.5), forcing=None)
    wide = _bern_model(np.full((2, 301), 0.01), np.tile([[1]], (300, 1)), [[0.0, 1.0]])
    refused(r'needs 304 values per member in LDS \(1 \+ 1 factors \+ 1 normalised states \+ 301 coefficients\).* hold 288',
            models=[wide], inputs=[['y']], forcing=None)
    # the host statement refuses the same
    with pytest.raises(ValueError, match='rtol must be finite'):
        dynamics.simulate_adaptive_host(**good, rtol=np.nan)
    with pytest.raises(ValueError, match='0 <= min_halvings <= max_halvings <= 12'):
        dynamics.simulate_adaptive_host(**good, max_halvings=13)

"""dynamics.simulate_stiff_host, the statement the device kernel is tested against (tests/test_simulate_stiff_gpu.py): the
Rodas3 step against its stability function in exact arithmetic, its order, the stiff members it is for, the tolerance in the
record, the pivoting of its factorisation, the kink at the wall of the box, a NaN member, the bookkeeping and every refusal --
none of which needs a device."""
import math
from fractions import Fraction

import numpy as np
import pytest

from fokl_gpy_amd import _capi, dynamics
from test_simulate_adaptive_host import (BERN, _bern_model, nan_system, outside_system, stiff_linear, two_state_system,
                                         wall_system)

RECORD = ('first_saturation', 'steps', 'rejected', 'swaps', 'max_level', 'error', 'first_unresolved')
DTYPES = dict(first_saturation=np.int32, steps=np.int64, rejected=np.int64, swaps=np.int64, max_level=np.int32,
              error=np.float64, first_unresolved=np.int32, levels=np.int8)
RATES = (-0.4, -3.2, -64.0, -1000.0, -1e5)


class _Reached(Exception):
    pass


class _NoDevice(_capi.DeviceContext):
    """Stands where the device context would be: a refused call must not reach the launch, a well-formed one ends here."""

    def __init__(self, expect_launch=False):
        self._h = None
        self.expect_launch = expect_launch

    def simulate_stiff(self, p):
        if not self.expect_launch:
            pytest.fail("a refused call reached the launch")
        raise _Reached(p)


def stability(z):
    """R(z) of Rodas3, in whatever arithmetic z brings."""
    return 8 * (z ** 3 - 6 * z + 6) / (3 * (z - 2) ** 4)


def closed_form(b, fixed, L, points, y0=1.0, h=0.0625):
    """[members, points] of y* + R(b g)^n (y0 - y*) at the output points, g = h / 2^L, from Fractions."""
    out = np.empty((len(b), points))
    for e in range(len(b)):
        R = stability(b[e] * Fraction(h) / 2 ** L) ** (2 ** L)        # one output step
        for n in range(points):
            out[e, n] = float(fixed[e] + R ** n * (Fraction(y0) - fixed[e]))
    return out


def rotating_system(E=2, steps=8, h=0.0625, n_states=2):
    """States around the fixed point 2 of d(x - 2)/dt = A (x - 2), A = scale_e x pairs [[-1, -50], [50, -60]] on the diagonal
    (an odd last state reads its neighbour: 50 (x_prev - 2) - 60 (x - 2)): at level 0 a pair's part of W is
    [[32 + scale, 50 scale], [-50 scale, 32 + 60 scale]], so its first column takes its pivot from the row below (50 > 33).
    Order-1 Bernoulli models over [0, 4], each reading two states."""
    c0, c1 = (float(v) for v in BERN[0])
    scale = np.linspace(1.0, 1.5, E)
    names = [f'x{k}' for k in range(n_states)]
    models, inputs = [], []
    for k in range(n_states):
        first = k - k % 2 if k + 1 < n_states or k % 2 else k - 1
        row = [-1.0, -50.0] if k == first else [50.0, -60.0]
        beta = np.array(row) * 4.0 / c1
        models.append(_bern_model(scale[:, None] * np.array([-(beta[0] + beta[1]) * (c0 + 0.5 * c1), beta[0], beta[1]]),
                                  [[1, 0], [0, 1]], [[0.0, 4.0], [0.0, 4.0]]))
        inputs.append([names[first], names[first + 1]])
    return dict(models=models, states=names, inputs=inputs, y0=[2.5, 2.0] * (n_states // 2) + [2.0] * (n_states % 2),
                t=(0.0, steps * h, h))


# ---------------------------------------------------------------------------------------------------------
# 1. the closed form
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L', [0, 2])
def test_forced_level_is_the_stability_function_in_exact_arithmetic(L):
    """At most 128 steps of about 60 roundings each at 1.1e-16, with a margin of about 10: 1e-11 (|y0| + |y*|)."""
    args, b, fixed = stiff_linear(RATES, steps=32)
    res = dynamics.simulate_stiff_host(**args, keep=('members', 'levels'), min_halvings=L, max_halvings=L)
    want = closed_form(b, fixed, L, 33)
    err = np.max(np.abs(res.members[:, 0] - want), axis=1)
    print(f"\nlevel {L}: distance to the closed form {err.tolist()}")
    assert np.all(err <= 1e-11 * (1.0 + 2.0))
    assert np.array_equal(res.steps, np.full(5, 32 * 2 ** L)) and not res.rejected.any()
    assert (res.levels == L).all() and (res.max_level == L).all() and (res.first_saturation == -1).all()


def test_stability_function_is_l_stable():
    assert abs(stability(Fraction(-10 ** 12))) < 1e-11
    w = np.linspace(0.0, 200.0, 4001)
    assert np.max(np.abs(stability(1j * w))) <= 1.0 + 1e-12


# ---------------------------------------------------------------------------------------------------------
# 2. the order
# ---------------------------------------------------------------------------------------------------------

def test_order_three():
    """The two-state system on 6 output steps of 0.25, where the scheme's error at level 4 (6e-10) stands well above the
    reference's own: the explicit statement at rtol = 1e-11 with atol = 0 (its default atol, 1e-9 of the box, would be the
    larger error)."""
    args = two_state_system(steps=6, h=0.25)
    ref = dynamics.simulate_adaptive_host(**args, keep='members', rtol=1e-11, atol=0.0)
    assert (ref.first_unresolved == -1).all() and (ref.first_saturation == -1).all()
    err = []
    for L in (2, 3, 4):
        got = dynamics.simulate_stiff_host(**args, keep='members', min_halvings=L, max_halvings=L)
        err.append(np.max(np.abs(got.members[:, :, -1] - ref.members[:, :, -1])))
    print(f"\nend-point errors at levels 2, 3, 4: {err}; ratios {err[0] / err[1]:.2f}, {err[1] / err[2]:.2f}")
    assert 6.0 <= err[0] / err[1] <= 10.0 and 6.0 <= err[1] / err[2] <= 10.0


# ---------------------------------------------------------------------------------------------------------
# 3. what it is for
# ---------------------------------------------------------------------------------------------------------

def test_a_decayed_fast_mode_no_longer_chooses_the_step():
    rtol, atol = 1e-4, 1e-9
    args, b, fixed = stiff_linear([-64.0, -1000.0], steps=32)
    res = dynamics.simulate_stiff_host(**args, keep=('members', 'levels'), rtol=rtol, atol=atol)
    explicit = dynamics.simulate_adaptive_host(**args, keep=('members', 'levels'), rtol=rtol, atol=atol)
    assert res.first_unresolved[0] == -1                              # no forced step for b h = -64
    assert (res.levels[:, 2:] == 0).all()
    assert explicit.levels[0, 2:].min() >= 4 and explicit.levels[1, 2:].min() >= 9
    for e in range(2):
        want = np.array([float(fixed[e]) + (1.0 - float(fixed[e])) * math.exp(float(b[e] * Fraction(float(ti)))) for ti in res.t])
        err = np.max(np.abs(res.members[e, 0] - want))
        bound = res.steps[e] * (atol + 2 * rtol)
        print(f"\ndraw {e}: b h = {float(b[e]) * 0.0625:.0f}: steps {res.steps[e]} against {explicit.pairs[e]} pairs, rejected "
              f"{res.rejected[e]}, max level {res.max_level[e]}, levels from step 2 on {res.levels[e, 2:].max()} against "
              f"{explicit.levels[e, 2:].min()}..{explicit.levels[e, 2:].max()}, error {err:.3e}, bound {bound:.3e}, first_unresolved "
              f"{res.first_unresolved[e]}, error ratio {res.error[e]:.3g}")
        assert 4 * res.steps[e] < explicit.pairs[e]
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------
# 4. the tolerance in the record
# ---------------------------------------------------------------------------------------------------------

def test_tolerance_is_obeyed_in_the_record():
    args, _, _ = stiff_linear([-0.5, -1.6, -3.2, -6.0], y0=np.array([1.0, 0.5, 3.0, 1.5]), steps=16)
    ref = dynamics.simulate_adaptive_host(**args, keep='members', rtol=1e-11)
    runs, rtol = [], 1e-3
    for _ in range(11):                                               # 1e-3 halved down to about 1e-6
        runs.append(dynamics.simulate_stiff_host(**args, keep='members', rtol=rtol))
        rtol /= 2
    for res in runs:
        assert np.all(res.error[res.first_unresolved < 0] <= 1.0) and np.all(res.error > 0.0)
    steps = np.array([res.steps for res in runs])
    print(f"\nsteps per member as rtol halves from 1e-3:\n{steps.T}")
    assert np.all(np.diff(steps, axis=0) >= 0) and np.all(steps[-1] > steps[0])
    loose = dynamics.simulate_stiff_host(**args, keep='members', rtol=1e-4)
    tight = dynamics.simulate_stiff_host(**args, keep='members', rtol=1e-6)
    far = np.max(np.abs(loose.members - ref.members), axis=(1, 2))
    near = np.max(np.abs(tight.members - ref.members), axis=(1, 2))
    print(f"distance to the explicit reference at rtol 1e-4 {far.tolist()}, at 1e-6 {near.tolist()}")
    assert np.all(near < far)


# ---------------------------------------------------------------------------------------------------------
# 5. pivoting
# ---------------------------------------------------------------------------------------------------------

def test_the_factorisation_exchanges_rows_and_solves():
    args = rotating_system()
    seen = []
    res = dynamics.simulate_stiff_host(**args, keep='members', min_halvings=0, max_halvings=0,
                                       trial_hook=lambda s, live, W, LU, rows, F0, K1: seen.append((W, rows, F0, K1)))
    assert (res.swaps > 0).all() and res.swaps.dtype == np.int64
    assert np.array_equal(res.swaps, res.steps)                       # level 0 throughout: column 0 exchanges in every step
    free = dynamics.simulate_stiff_host(**args, keep='members')
    assert (free.swaps > 0).all() and (free.swaps < free.steps).any() and (free.first_unresolved == -1).all()
    assert len(seen) == 8
    for W, rows, F0, K1 in seen:
        assert (rows[0] == 1).all() and (np.abs(W[1, 0]) > np.abs(W[0, 0])).all()
        for m in range(W.shape[2]):
            want = np.linalg.solve(W[:, :, m], F0[:, m])
            assert np.max(np.abs(K1[:, m] - want)) <= 1e-12 * np.max(np.abs(want))


def test_pivot_ties_go_to_the_lowest_row():
    W = np.zeros((3, 3, 4))
    W[:, :, 0] = [[2.0, 1.0, 0.0], [-2.0, 3.0, 1.0], [2.0, 0.0, 5.0]]         # all equal: row 0 stays
    W[:, :, 1] = [[1.0, 1.0, 0.0], [-2.0, 3.0, 1.0], [2.0, 0.0, 5.0]]         # rows 1 and 2 tie above row 0: row 1
    W[:, :, 2] = [[1.0, 1.0, 0.0], [2.0, 3.0, 1.0], [-3.0, 0.0, 5.0]]         # no tie: row 2
    W[:, :, 3] = [[4.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, -1.0, 5.0]]         # a tie in column 1: row 1 stays
    LU, rows, exchanges = dynamics.stiff_lu(W)
    assert rows[0].tolist() == [0, 1, 2, 0] and rows[1, 3] == 1 and rows[2].tolist() == [2, 2, 2, 2]
    assert exchanges[0] == int(rows[1, 0] != 1) and exchanges[3] == 0 and exchanges[2] >= 1
    b = np.arange(1.0, 13.0).reshape(3, 4)
    x = dynamics.stiff_solve(LU, rows, b)
    for m in range(4):
        assert np.allclose(W[:, :, m] @ x[:, m], b[:, m], rtol=0, atol=1e-13 * 20)


# ---------------------------------------------------------------------------------------------------------
# 6. kinks and locality
# ---------------------------------------------------------------------------------------------------------

def test_the_wall_of_the_box_is_reported_as_unresolved():
    """dy/dt <= 0.6 + 3 B1(1) = 2.1, and behind the wall the slope rule holds the state: it ends between the wall and one
    finest step behind it."""
    res = dynamics.simulate_stiff_host(**wall_system(), keep=('members', 'levels'), max_halvings=6)
    y = res.members[0, 0]
    print(f"\nfirst_saturation {res.first_saturation[0]}, first_unresolved {res.first_unresolved[0]}, end {y[-1]!r}, error "
          f"{res.error[0]:.3e}, steps {res.steps[0]}, max level {res.max_level[0]}")
    assert res.first_saturation[0] > 0 and res.first_unresolved[0] >= 0 and res.unresolved_fraction == 1.0
    assert 1.0 - 1e-9 <= y[-1] <= 1.0 + 2.1 * 0.125 / 2 ** 6
    assert res.max_level[0] == 6 and res.error[0] > 1.0


def test_a_member_outside_the_range_is_reported_from_step_zero():
    res = dynamics.simulate_stiff_host(**outside_system())
    assert res.first_saturation.tolist() == [-1, 0]


def test_a_nan_member_ends_and_stays_local():
    args = nan_system()
    res = dynamics.simulate_stiff_host(**args, keep=('members', 'levels'))
    assert res.first_unresolved.tolist() == [-1, 0, -1] and np.isfinite(res.error).all()
    assert res.max_level[1] == 5 and res.steps[1] == 4 * 2 ** 5 and np.isnan(res.members[1, :, 1:]).any()
    for e in (0, 2):
        alone = dynamics.simulate_stiff_host(**args, draws=np.array([e]), keep=('members', 'levels'))
        assert np.array_equal(alone.members[0], res.members[e]) and np.array_equal(alone.levels[0], res.levels[e])
        for key in RECORD:
            assert alone[key][0] == res[key][e], key


# ---------------------------------------------------------------------------------------------------------
# 7. bookkeeping and refusals
# ---------------------------------------------------------------------------------------------------------

def test_bookkeeping():
    args = two_state_system(steps=10)
    for model in args['models']:
        model['betas'] = 10.0 * model['betas']
    state = np.random.get_state()[1].copy()
    both = dynamics.simulate_stiff_host(**args, keep=('members', 'levels'), rtol=1e-7)
    assert np.array_equal(np.random.get_state()[1], state)           # nothing is drawn
    assert both.members.shape == (6, 2, 11) and both.levels.shape == (6, 10) and both.mean.shape == (2, 11)
    assert both.bounds.shape == (2, 11, 2) and both.t.shape == (11,)
    for key in RECORD:
        assert both[key].shape == (6,) and both[key].dtype == DTYPES[key], key
    assert both.levels.dtype == np.int8 and np.array_equal(both.levels.max(axis=1), both.max_level)
    assert (both.rejected > 0).any() and np.all(both.steps >= 10)
    assert np.all(both.steps <= np.sum(2 ** both.levels.astype(np.int64), axis=1))
    assert 'pairs' not in both and both.rtol == 1e-7 and both.atol.shape == (2,)
    for keep, has in ((None, ()), ('members', ('members',)), ('levels', ('levels',)), (('levels', 'members'), ('members', 'levels'))):
        res = dynamics.simulate_stiff_host(**args, keep=keep, rtol=1e-7)
        assert [name for name in ('members', 'levels') if name in res] == list(has)
        for key in RECORD + ('mean', 'bounds') + has:
            assert np.array_equal(res[key], both[key]), key
        for key in ('t', 'saturated_fraction', 'unresolved_fraction', 'states'):
            assert key in res
    forced = dynamics.simulate_stiff_host(**args, keep='levels', min_halvings=2, max_halvings=2)
    assert np.array_equal(np.sum(2 ** forced.levels.astype(np.int64), axis=1), forced.steps)


def test_refusals_name_the_limit_and_launch_nothing():
    model = _bern_model([[0.1, 0.2, 0.1], [0.1, 0.3, 0.2]], [[1, 0], [0, 1]], [[0.0, 1.0], [0.0, 5.0]])
    good = dict(models=[model], states=['y'], inputs=[['y', 'u']], forcing={'u': np.ones(10)}, y0=[0.5], t=(0.0, 1.0, 0.1))

    def refused(match, **changes):
        with pytest.raises(ValueError, match=match):
            dynamics.simulate_stiff(**{**good, **changes}, device=_NoDevice())

    with pytest.raises(_Reached) as hit:
        dynamics.simulate_stiff(**good, keep=('levels', 'members'), device=_NoDevice(expect_launch=True))
    p = hit.value.args[0]
    assert p['E'] == 2 and p['want_members'] and p['want_levels'] and (p['min_halvings'], p['max_halvings']) == (0, 10)
    assert p['rtol'] == 1e-4 and p['atol'].tolist() == [1e-9 * 1.0]  # the box is the training range [0, 1]
    assert p['lds_rows'] == 2 * (1 + 2 + 1) + 3
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
    free = _bern_model([[0.1, 0.2], [0.1, 0.3]], [[1]], [[0.0, 5.0]])
    unbounded = dict(models=[free], states=['y'], inputs=[['u']])
    refused("state 'y': its box is unbounded.*pass atol", **unbounded)
    with pytest.raises(_Reached):
        dynamics.simulate_stiff(**{**good, **unbounded}, atol=1e-9, device=_NoDevice(expect_launch=True))
    with pytest.raises(_Reached):                                     # rtol == 0 alone is a pure absolute tolerance
        dynamics.simulate_stiff(**good, rtol=0.0, device=_NoDevice(expect_launch=True))
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
    # the tangent rows: a system simulate still takes (288 values) needs 291 here
    fits = _bern_model(np.full((2, 285), 0.01), np.tile([[1]], (284, 1)), [[0.0, 1.0]])
    refused(r'needs 291 values per member in LDS \(2 x \(1 \+ 1 factors \+ 1 normalised states\) \+ 285 coefficients.*tangent '
            r'rows\), a wavefront.s 144 KB hold 288', models=[fits], inputs=[['y']], forcing=None)
    dynamics.simulate_host(**{**good, 'models': [fits], 'inputs': [['y']], 'forcing': None})
    # the host statement refuses the same
    with pytest.raises(ValueError, match='rtol must be finite'):
        dynamics.simulate_stiff_host(**good, rtol=np.nan)
    with pytest.raises(ValueError, match='0 <= min_halvings <= max_halvings <= 12'):
        dynamics.simulate_stiff_host(**good, max_halvings=13)
    with pytest.raises(ValueError, match='needs 291 values per member in LDS'):
        dynamics.simulate_stiff_host(**{**good, 'models': [fits], 'inputs': [['y']], 'forcing': None})

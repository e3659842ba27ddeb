"""dynamics.assimilate_host, the statement the particle-filter kernel is tested against (tests/test_assimilate_gpu.py):
without noise it is simulate_host, on a linear system it is a Kalman filter up to Monte-Carlo error, its lane reductions
have the documented orders, and resampling, missing data, collapse, pooling and every refusal behave as the module
docstring of fokl_gpy_amd/dynamics.py says -- none of which needs a device."""
import math

import numpy as np
import pytest

import assimilate_cases as cases
from fokl_gpy_amd import _capi, dynamics


class _NoDevice(_capi.DeviceContext):
    """Stands where the device context would be and counts the launches asked of it."""

    def __init__(self):
        self._h = None
        self.calls = 0

    def assimilate_ensemble(self, p):
        self.calls += 1
        raise RuntimeError('reached the launch')


def _noise_free(args, points, observe, n_cols):
    data = np.linspace(-0.5, 0.5, len(points) * n_cols).reshape(len(points), n_cols)
    return dict(args, observe=observe, data=data, obs_points=points, obs_sd=[0.3] * n_cols, process_sd=0.0, y0_sd=0.0,
                resample_below=0.0, keep='particles')


# ---------------------------------------------------------------------------------------------------------
# 1. with no noise the filter is simulate
# ---------------------------------------------------------------------------------------------------------

def test_without_noise_every_particle_is_simulates_member():
    args = cases.two_state(E=3, steps=40)
    points = [0, 5, 17, 40]
    res = dynamics.assimilate_host(**_noise_free(args, points, ['c', 'T'], 2))
    sim = dynamics.simulate_host(**args, ReturnBounds=False, keep='members')
    assert res.particles.shape == (3, 4, 64, 2) and res.t_obs.tolist() == sim.t[points].tolist()
    want = sim.members[:, :, points].transpose(0, 2, 1)               # [E, n_obs, K]
    assert np.array_equal(res.particles, np.broadcast_to(want[:, :, np.newaxis, :], res.particles.shape))
    assert np.array_equal(res.first_saturation, sim.first_saturation) and not res.resampled.any()
    assert np.array_equal(res.particle_weights, np.full((3, 4, 64), 1.0 / 64)) and np.all(res.ess == 64.0)
    assert np.array_equal(res.draw_mean, want.transpose(0, 2, 1)) and np.all(res.draw_var == 0.0)
    assert (res.collapsed == -1).all() and np.isfinite(res.log_evidence).all()


# ---------------------------------------------------------------------------------------------------------
# 2. a linear system: the Kalman filter
# ---------------------------------------------------------------------------------------------------------

KALMAN = dict(steps=40, every=4, process_sd=0.2, obs_sd=0.1, y0=1.0, y0_sd=0.1, E=256)
MEAN_FIGURES = (0.0083, 0.0184, 0.0254, 0.0170, 0.0167)              # seeds 0 .. 4, see the test's docstring
VAR_FIGURES = (0.0297, 0.0232, 0.0283, 0.0150, 0.0255)


def _kalman_case():
    k = KALMAN
    model, h, A, c = cases.linear_model(k['E'])
    q = k['process_sd'] * np.sqrt(h)
    rng = np.random.default_rng(123)
    y, data = k['y0'] + k['y0_sd'] * rng.standard_normal(), []
    mean, var, log_evidence, exact = k['y0'], k['y0_sd'] ** 2, 0.0, []
    for s in range(k['steps']):
        y = A * y + c + q * rng.standard_normal()
        mean, var = A * mean + c, A * A * var + q * q                # the scalar Kalman recursion: predict ...
        if (s + 1) % k['every'] == 0:
            data.append(y + k['obs_sd'] * rng.standard_normal())
            S = var + k['obs_sd'] ** 2                               # ... and update
            log_evidence += -0.5 * math.log(2 * math.pi * S) - 0.5 * (data[-1] - mean) ** 2 / S
            gain = var / S
            mean, var = mean + gain * (data[-1] - mean), (1 - gain) * var
            exact.append((mean, var, log_evidence))
    args = dict(models=[model], states=['y'], inputs=[['y']], y0=[k['y0']], t=(0.0, (k['steps'] - 0.5) * h, h),
                bounds=[[-100.0, 100.0]], observe=['y'], data=np.array(data)[:, np.newaxis], every=k['every'],
                obs_sd=[k['obs_sd']], process_sd=[k['process_sd']], y0_sd=[k['y0_sd']], resample_below=0.5)
    return args, np.array(exact)


def test_linear_system_is_the_kalman_filter():
    """The one-state linear model of test_linear_system_follows_rk4s_amplification: its RK4 step is y <- A y + c, so with
    Gaussian process and observation noise the exact filter is the scalar Kalman recursion above.  256 ensembles of the
    same betas row under the draw ids 0 .. 255, 10 observations, obs_sd 0.1 next to a predictive spread of about 0.1.

    Evidence: the particle estimate is unbiased, |mean(r) - 1| <= 4 std(r) / 16 with r = exp(log_evidence - exact).
    Tried on this host at the committed seed 0 and at seeds 1 and 2: |mean(r) - 1| = 0.0031, 0.0251, 0.0408 against
    bounds 0.1330, 0.1423, 0.1265.

    Filtered mean and variance: biased at order 1 / 64.  Measured with this statement over the seeds 0 .. 4, the largest
    over the 10 observations of |pooled mean - Kalman mean| / Kalman sd: 0.0083, 0.0184, 0.0254, 0.0170, 0.0167; of
    |pooled variance - Kalman variance| / Kalman variance: 0.0297, 0.0232, 0.0283, 0.0150, 0.0255.  All far below 0.1.
    The test asserts three times the largest of each; the margin covers the seed-to-seed spread."""
    args, exact = _kalman_case()
    res = dynamics.assimilate_host(**args, seed=0)
    assert (res.first_saturation == -1).all() and (res.collapsed == -1).all()
    assert res.resampled.any() and not res.resampled.all()
    r = np.exp(res.log_evidence[:, -1] - exact[-1, 2])
    print(f"\nevidence: |mean(r) - 1| = {abs(r.mean() - 1):.4f}, bound {4 * r.std() / 16:.4f}")
    assert abs(r.mean() - 1) <= 4 * r.std() / 16
    mean_error = np.max(np.abs(res.mean[0] - exact[:, 0]) / np.sqrt(exact[:, 1]))
    var_error = np.max(np.abs(res.sd[0] ** 2 - exact[:, 1]) / exact[:, 1])
    print(f"pooled mean error / Kalman sd {mean_error:.4f}, relative variance error {var_error:.4f}")
    assert max(MEAN_FIGURES) <= 0.1 and max(VAR_FIGURES) <= 0.1
    assert mean_error <= 3 * max(MEAN_FIGURES) and var_error <= 3 * max(VAR_FIGURES)


# ---------------------------------------------------------------------------------------------------------
# 3. the lane reductions
# ---------------------------------------------------------------------------------------------------------

def test_lane_reductions_have_the_documented_order():
    rng = np.random.default_rng(4)
    v = rng.random((5, 64)) * 10.0 ** rng.integers(-3, 3, (5, 64))
    total, top, scan = dynamics.lane_sum(v), dynamics.lane_max(v), dynamics.lane_scan(v)
    for row in range(5):
        assert abs(total[row] - math.fsum(v[row])) <= 1e-15 * math.fsum(v[row])
        assert top[row] == v[row].max()
        exact = np.cumsum(v[row].astype(np.longdouble))
        assert np.all(np.abs(scan[row] - exact) <= 1e-15 * exact)
        # the documented order, lane by lane
        a = list(v[row])
        for offset in (32, 16, 8, 4, 2, 1):
            a = [a[i] + a[i ^ offset] for i in range(64)]
        assert a == [total[row]] * 64
        m = list(v[row])
        for offset in (32, 16, 8, 4, 2, 1):
            m = [max(m[i], m[i ^ offset]) for i in range(64)]
        assert m == [top[row]] * 64
        c = list(v[row])
        for offset in (1, 2, 4, 8, 16, 32):
            c = [c[i] + c[i - offset] if i >= offset else c[i] for i in range(64)]
        assert c == list(scan[row])
    with_nan = v[0].copy()
    with_nan[[3, 40]] = np.nan
    assert dynamics.lane_max(with_nan) == np.nanmax(with_nan) and np.isnan(dynamics.lane_max(np.full(64, np.nan)))
    assert np.isnan(dynamics.lane_sum(with_nan))


# ---------------------------------------------------------------------------------------------------------
# 4. resampling
# ---------------------------------------------------------------------------------------------------------

def test_systematic_resampling():
    rng = np.random.default_rng(6)
    W = rng.random((40, 64)) ** 8                                     # a few heavy particles
    W[7, 5:] = 0.0
    W[8] = 0.0
    W[8, 63] = 1.0
    W = W / dynamics.lane_sum(W)[:, np.newaxis]
    u = np.concatenate([[0.0, 1.0 - 2.0 ** -53], rng.random(38)])
    ancestors = dynamics.systematic_ancestors(W, u)
    assert ancestors.shape == (40, 64) and ancestors.min() >= 0 and ancestors.max() <= 63
    assert np.all(np.diff(ancestors, axis=1) >= 0)
    for e in range(40):
        copies = np.bincount(ancestors[e], minlength=64)
        assert np.all(np.abs(copies - 64 * W[e]) <= 1.0), e
    assert (ancestors[8] == 63).all() and ancestors[7].max() <= 4


def test_resample_below_zero_never_and_one_wherever_ess_is_short():
    args = cases.two_state(E=4, steps=30)
    rng = np.random.default_rng(2)
    noisy = dict(args, observe=['T'], data=0.3 + 0.2 * rng.standard_normal((6, 1)), every=5, obs_sd=[0.2],
                 process_sd=[0.1, 0.05], y0_sd=[0.05, 0.05], seed=3, keep='particles')
    never = dynamics.assimilate_host(**noisy, resample_below=0.0)
    assert not never.resampled.any() and (never.ess < 32).any()       # the weights degenerate, and are left to
    always = dynamics.assimilate_host(**noisy, resample_below=1.0)
    assert np.array_equal(always.resampled, always.ess < 64.0) and always.resampled.all()
    # after a resampling the weights start again from 1 / 64: the next row's weights are its likelihoods alone
    half = dynamics.assimilate_host(**noisy, resample_below=0.5)
    assert half.resampled.any() and not half.resampled.all()
    assert np.array_equal(half.resampled, half.ess < 32.0)
    assert np.allclose(half.particle_weights.sum(axis=2), 1.0, rtol=0, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------
# 5. missing data
# ---------------------------------------------------------------------------------------------------------

def test_missing_entries_rows_and_the_ends_of_the_axis():
    args = cases.two_state(E=3, steps=20)
    rng = np.random.default_rng(8)
    values = 0.3 + 0.1 * rng.standard_normal(4)
    common = dict(obs_points=[0, 7, 13, 20], process_sd=[0.1, 0.05], y0_sd=[0.05, 0.02], resample_below=0.5, seed=11,
                  keep='particles')
    one = dynamics.assimilate_host(**args, observe=['T'], data=values[:, np.newaxis], obs_sd=[0.05], **common)
    assert one.t_obs[0] == 0.0 and one.t_obs[-1] == dynamics.simulate_host(**args, ReturnBounds=False).t[-1]
    assert np.isfinite(one.log_evidence).all() and one.resampled.any()
    # a sensor that never reports is a sensor that does not exist
    two = dynamics.assimilate_host(**args, observe=['T', 'c'], data=np.stack([values, np.full(4, np.nan)], axis=1),
                                   obs_sd=[0.05, 0.3], **common)
    for key in ('log_evidence', 'particle_weights', 'particles', 'ess', 'resampled', 'draw_mean'):
        assert np.array_equal(one[key], two[key]), key
    # ... and one that reports once is counted once
    partly = np.stack([values, [np.nan, np.nan, -0.1, np.nan]], axis=1)
    three = dynamics.assimilate_host(**args, observe=['T', 'c'], data=partly, obs_sd=[0.05, 0.3], **common)
    assert np.array_equal(three.log_evidence[:, :2], one.log_evidence[:, :2])
    assert not np.array_equal(three.log_evidence[:, 2], one.log_evidence[:, 2])
    # a row of NaN changes nothing, but is reported with its ESS
    gap = dynamics.assimilate_host(**args, observe=['T'], data=np.insert(values, 2, np.nan)[:, np.newaxis], obs_sd=[0.05],
                                   **dict(common, obs_points=[0, 7, 10, 13, 20]))
    rest = [0, 1, 3, 4]
    for key in ('log_evidence', 'particle_weights', 'particles', 'ess', 'resampled'):
        assert np.array_equal(gap[key][:, rest], one[key][:, :]), key
    assert np.array_equal(gap.log_evidence[:, 2], gap.log_evidence[:, 1]) and not gap.resampled[:, 2].any()
    assert np.all((gap.ess[:, 2] > 1.0) & (gap.ess[:, 2] <= 64.0)) and gap.particles[:, 2].std() > 0


# ---------------------------------------------------------------------------------------------------------
# 6. collapse
# ---------------------------------------------------------------------------------------------------------

def collapse_case(E=3, far=1):
    """Draw ``far`` starts 1e3 obs_sd from the data; no process noise.  -> (arguments, arguments without that draw)"""
    args = cases.two_state(E=E, steps=10)
    obs_sd = 1e-3
    y0 = np.tile(args['y0'], (E, 1))
    y0[far, 0] += 1e3 * obs_sd
    sim = dynamics.simulate_host(**dict(args, y0=np.tile(args['y0'], (E, 1))), ReturnBounds=False, keep='members')
    data = sim.members[0, :1, [5, 10]]                               # what draw 0 measures of T at the two points
    full = dict(args, y0=y0, observe=['T'], data=data, obs_points=[5, 10], obs_sd=[obs_sd], process_sd=0.0,
                y0_sd=[2e-3, 1e-3], resample_below=0.5, seed=2, keep='particles')
    others = [e for e in range(E) if e != far]
    return full, dict(full, y0=y0[others], draws=np.array(others)), others


def test_a_collapsed_draw_has_no_evidence_and_touches_no_other():
    full, without, others = collapse_case()
    res, rest = dynamics.assimilate_host(**full), dynamics.assimilate_host(**without)
    assert res.collapsed.tolist() == [-1, 0, -1] and res.collapsed.dtype == np.int32
    assert np.all(res.log_evidence[1] == -np.inf) and res.weights[1] == 0.0 and abs(res.weights.sum() - 1.0) <= 1e-15
    assert np.array_equal(res.particle_weights[1], np.full((2, 64), 1.0 / 64)) and not res.resampled[1].any()
    assert np.isfinite(res.log_evidence[others]).all() and np.isfinite(res.mean).all() and np.isfinite(res.sd).all()
    for key in ('log_evidence', 'particles', 'particle_weights', 'draw_mean', 'draw_var', 'ess', 'resampled'):
        assert np.array_equal(res[key][others], rest[key]), key
    assert 1 not in res.draw_index


# ---------------------------------------------------------------------------------------------------------
# 7. pooling
# ---------------------------------------------------------------------------------------------------------

def test_pooling_over_the_draws():
    E = 12
    args = cases.two_state(E=E, steps=20)
    rng = np.random.default_rng(12)
    call = dict(args, observe=['T', 'c'], data=np.array([0.3, -0.2]) + 0.1 * rng.standard_normal((4, 2)), every=5,
                obs_sd=[0.1, 0.1], process_sd=[0.1, 0.05], y0_sd=[0.05, 0.02])
    res = dynamics.assimilate_host(**call, seed=21)
    assert abs(res.weights.sum() - 1.0) <= 1e-14 and res.weights.min() >= 0
    assert res.ess_draws == pytest.approx(1.0 / np.sum(res.weights ** 2), rel=1e-14) and 1.0 <= res.ess_draws <= E
    top = res.log_evidence[:, -1].max()
    want = np.exp(res.log_evidence[:, -1] - top) / np.exp(res.log_evidence[:, -1] - top).sum()
    assert np.allclose(res.weights, want, rtol=1e-13, atol=0)
    again = dynamics.assimilate_host(**call, seed=21)
    assert np.array_equal(res.draw_index, again.draw_index) and res.draw_index.shape == (E,)
    copies = np.bincount(res.draw_index, minlength=E)
    assert np.all(np.abs(copies - E * res.weights) <= 1.0) and np.all(np.diff(res.draw_index) >= 0)
    other = dynamics.assimilate_host(**call, seed=22)
    assert not np.array_equal(other.log_evidence, res.log_evidence)
    # total variance = within + between, with the running draw weights
    for k in range(4):
        w = np.exp(res.log_evidence[:, k] - res.log_evidence[:, k].max())
        w = w / w.sum()
        mean = (w[:, np.newaxis] * res.draw_mean[:, :, k]).sum(axis=0)
        within = (w[:, np.newaxis] * res.draw_var[:, :, k]).sum(axis=0)
        between = (w[:, np.newaxis] * (res.draw_mean[:, :, k] - mean) ** 2).sum(axis=0)
        assert np.allclose(res.mean[:, k], mean, rtol=1e-13, atol=1e-15)
        assert np.allclose(res.sd[:, k] ** 2, within + between, rtol=1e-12, atol=0)
    # a subset of the draws reproduces the full run's
    some = dynamics.assimilate_host(**call, seed=21, draws=np.array([7, 2]))
    assert np.array_equal(some.log_evidence, res.log_evidence[[7, 2]]) and np.array_equal(some.draw_mean, res.draw_mean[[7, 2]])
    assert set(some.draw_index) <= {2, 7}
    with_bounds = dynamics.assimilate_host(**call, seed=21, keep='particles')
    assert with_bounds.bounds.shape == (2, 4, 2)
    assert np.all(with_bounds.bounds[..., 0] <= res.mean) and np.all(res.mean <= with_bounds.bounds[..., 1])


def test_the_filter_leaves_numpys_stream_alone():
    args = cases.two_state(E=2, steps=10)
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    dynamics.assimilate_host(**args, observe=['T'], data=np.full((2, 1), 0.3), every=5, obs_sd=[0.1], process_sd=0.1)
    assert np.array_equal(np.random.get_state()[1], state)


# ---------------------------------------------------------------------------------------------------------
# 8. refusals: each before any launch, with a message that names the limit
# ---------------------------------------------------------------------------------------------------------

def test_refusals_name_the_limit_and_launch_nothing():
    args = cases.two_state(E=3, steps=20)
    good = dict(args, observe=['T'], data=np.full((4, 1), 0.3), every=5, obs_sd=[0.1], process_sd=[0.1, 0.1])
    ctx = _NoDevice()

    def refused(match, **changes):
        with pytest.raises(ValueError, match=match):
            dynamics.assimilate(**{**good, **changes}, device=ctx)

    refused("observe: 'q' is not a state", observe=['q'])
    refused('observe must name at least one', observe=[])
    refused('observe names a state twice', observe=['T', 'T'], data=np.full((4, 2), 0.3), obs_sd=[0.1, 0.1])
    refused(r'data must be \[4, 1\]', data=np.full((5, 1), 0.3))
    refused(r'data must be \[4, 1\]', data=np.full((4, 2), 0.3))
    refused(r'obs_points must lie in 0 \.\. 20', every=None, obs_points=[5, 21], data=np.full((2, 1), 0.3))
    refused(r'obs_points must lie in 0 \.\. 20', every=None, obs_points=[-1, 5], data=np.full((2, 1), 0.3))
    refused('strictly increasing', every=None, obs_points=[5, 5], data=np.full((2, 1), 0.3))
    refused('strictly increasing', every=None, obs_points=[7, 5], data=np.full((2, 1), 0.3))
    refused('exactly one of the two', obs_points=[5, 10, 15, 20])
    refused('exactly one of the two', every=None)
    refused('every must be a positive integer', every=0)
    refused('obs_sd must be positive', obs_sd=[0.0])
    refused('obs_sd must be positive', obs_sd=[-1.0])
    refused('obs_sd needs one value per observed state', obs_sd=[0.1, 0.1])
    refused('process_sd must be non-negative', process_sd=[0.1, -0.1])
    refused('process_sd needs one value per state', process_sd=[0.1, 0.1, 0.1])
    refused('y0_sd must be non-negative', y0_sd=[-0.1, 0.0])
    refused(r'resample_below must lie in \[0, 1\]', resample_below=1.5)
    refused(r'resample_below must lie in \[0, 1\]', resample_below=-0.1)
    refused('no observation', every=21, data=np.zeros((0, 1)))
    refused('no observation', every=None, obs_points=[], data=np.zeros((0, 1)))
    refused('no observation: every entry of data is NaN', data=np.full((4, 1), np.nan))
    refused("keep must be None or 'particles'", keep='members')
    # what simulate refuses
    refused("'w' is neither a state", inputs=[['T', 'c', 'w'], ['T', 'c']])
    refused('y0 holds NaN', y0=[np.nan, 0.0])
    refused("state 'T': its box is empty", bounds=[[1.0, 1.0], [-1.0, 1.0]])
    refused(r"forcing\['u'\] has 9 values but 20 steps", forcing={'u': np.ones(9)})
    one = cases.model('b', [0.1, 0.1], [[1]], [[0.0, 1.0]], 2, np.random.default_rng(0))
    names = [f's{k}' for k in range(9)]
    refused('at most 8 states, the system has 9', models=[one] * 9, states=names, inputs=[[n] for n in names],
            y0=np.full(9, 0.5), forcing=None, observe=['s0'], process_sd=0.0)
    # ... except its LDS bound per member: 304 values per member do not fit simulate, but they fit here
    wide = cases.model('b', np.full(301, 0.01), np.tile([[1]], (300, 1)), [[0.0, 1.0]], 2, np.random.default_rng(0))
    lds = dict(models=[wide], states=['y'], inputs=[['y']], forcing=None, y0=[0.5], observe=['y'], process_sd=0.0)
    with pytest.raises(ValueError, match='needs 304 values per member in LDS'):
        dynamics.simulate(**{k: {**good, **lds}[k] for k in ('models', 'states', 'inputs', 'forcing', 'y0', 't')}, device=ctx)
    assert ctx.calls == 0
    with pytest.raises(RuntimeError, match='reached the launch'):
        dynamics.assimilate(**{**good, **lds}, device=ctx)
    assert ctx.calls == 1
    # its own: the coefficients once, everything else per lane
    huge = cases.model('b', np.full(18200, 0.01), np.tile([[1]], (18199, 1)), [[0.0, 1.0]], 2, np.random.default_rng(0))
    refused(r'needs 147648 bytes of LDS \(\(3 factor and state rows \+ the exchange row\) x 64 x 8 \+ 18200 coefficients x 8\), '
            r'a wavefront has 147456', **dict(lds, models=[huge]))
    assert ctx.calls == 1
    with pytest.raises(RuntimeError, match='reached the launch'):
        dynamics.assimilate(**good, device=ctx)
    assert ctx.calls == 2


def test_the_random_numbers_are_their_own_streams():
    ids = np.array([0, 5, 77], dtype=np.uint32)
    z = _capi.assimilate_rng(9, ids, 3, 1, 64)
    assert z.shape == (3, 64) and np.array_equal(z, _capi.assimilate_rng(9, ids, 3, 1, 64))
    assert np.array_equal(_capi.assimilate_rng(9, ids[1:2], 3, 1, 64)[0], z[1])       # a draw's numbers are its id's
    assert not np.array_equal(z[0], _capi.infer_rng(9, 0, 3, 3, 64))                 # the fourth counter word differs
    u = _capi.assimilate_rng(9, ids, 3, _capi.ASSIMILATE_RESAMPLE, 4)
    assert np.all((u >= 0) & (u < 1)) and abs(_capi.assimilate_rng(1, ids, 0, 0, 4096).mean()) < 0.05
    with pytest.raises(_capi.FoklNativeError):
        _capi.assimilate_rng(9, ids, 3, 11, 4)

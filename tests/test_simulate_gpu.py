"""dynamics.simulate on the MI355X against its statement dynamics.simulate_host (pinned without a device by
tests/test_simulate_host.py): every member and every saturation record bit for bit, the bounds as the order statistics of
the returned members, the mean within the rounding of a sum of E terms (the device's summation tree is not numpy's)."""
import os
import warnings

import numpy as np
import pytest

from helpers import GOLDEN
from band_reference import band_next_to_nan, band_rows, mean_rows, same_rows
from test_simulate_adaptive_host import nan_system
from fokl_gpy_amd import dynamics, getKernels
from fokl_gpy_amd.GP_Integrate import bounds_cut

pytestmark = pytest.mark.gpu

BERN = getKernels.bernoulli()
SPLINES = getKernels.table_to_phis(np.load(os.path.join(GOLDEN, 'spline_phis.npz'))['table'])
KERNELS = {'b': ('Bernoulli Polynomials', BERN), 's': ('Cubic Splines', SPLINES)}


def _model(kind, mean, mtx, minmax, E, rng, spread=0.1):
    mean = np.asarray(mean, dtype=np.float64)
    kernel, phis = KERNELS[kind]
    return dict(betas=mean * (1 + spread * rng.standard_normal((E, mean.shape[0]))), mtx=np.asarray(mtx, dtype=int), phis=phis,
                minmax=minmax, kernel=kernel)


def _system(seed, n_states, kinds, E, steps, n_forcing=0, orders=(1, 2, 3), h=0.05):
    """Model k reads its own state, the next one and (with forcing) column k % n_forcing, each through a range of its own;
    one term per column plus their product."""
    rng = np.random.default_rng(seed)
    states = [f'x{k}' for k in range(n_states)]
    forcing = {f'u{c}': 5.0 + 4.0 * np.sin(np.arange(steps + 3) / (2.0 + c)) for c in range(n_forcing)}
    models, inputs = [], []
    for k in range(n_states):
        names = [states[k]] + ([states[(k + 1) % n_states]] if n_states > 1 else []) + ([f'u{k % n_forcing}'] if n_forcing else [])
        m = len(names)
        mtx = np.concatenate([np.diag(rng.choice(orders, size=m)), np.ones((1, m), dtype=int)])
        minmax = [[0.0, 10.0] if name in forcing else [-1.0 - 0.125 * k, 1.0 + 0.25 * k] for name in names]
        models.append(_model(kinds[k % len(kinds)], 0.3 * rng.standard_normal(m + 2), mtx, minmax, E, rng))
        inputs.append(names)
    return dict(models=models, states=states, inputs=inputs, forcing=forcing, y0=rng.uniform(-0.5, 0.5, (E, n_states)),
                t=(0.0, (steps - 0.5) * h, h))


def _compare(ctx, **args):
    """simulate against simulate_host -> (device result, host result)."""
    host = dynamics.simulate_host(**args, keep='members')
    dev = dynamics.simulate(**args, keep='members', device=ctx)
    E = host.members.shape[0]
    assert np.isfinite(host.members).all()
    assert dev.members.shape == host.members.shape and np.array_equal(dev.t, host.t)
    differ = dev.members != host.members
    if differ.any():
        e, k, q = np.argwhere(differ)[0]
        print(f"\n{int(differ.sum())} values differ, first at member {e} state {k} point {q}: device {dev.members[e, k, q]!r} "
              f"host {host.members[e, k, q]!r}")
    assert np.array_equal(dev.members, host.members)
    assert dev.first_saturation.dtype == np.int32 and np.array_equal(dev.first_saturation, host.first_saturation)
    assert dev.saturated_fraction == host.saturated_fraction
    if args.get('ReturnBounds', True):
        srt, cut = np.sort(dev.members, axis=0), bounds_cut(E)
        assert np.array_equal(dev.bounds[..., 0], srt[cut]) and np.array_equal(dev.bounds[..., 1], srt[E - cut])
    else:
        assert 'bounds' not in dev
    assert np.all(np.abs(dev.mean - dev.members.mean(0)) <= E * 2.0 ** -52 * np.max(np.abs(dev.members), axis=0))
    return dev, host


@pytest.mark.parametrize('E', [1, 63, 64, 65, 130])
def test_members_pad_lanes_and_fill_workgroups(device_ctx, E):
    args = _system(10 + E, 2, 'b', E, steps=12, n_forcing=1)
    dev, _ = _compare(device_ctx, **args, ReturnBounds=E > 1)
    rep = device_ctx.simulate_report()
    assert rep['NS'] == 2 and rep['members'] == E and rep['workgroups'] == -(-E // 64) and rep['launches'] == 1
    assert rep['spline_factors'] == 0 and rep['bernoulli_factors'] > 0 and rep['lds_bytes'] % 512 == 0
    assert dev.members.shape == (E, 2, 13)
    # reproducible, and without the members the same mean and bounds
    again = dynamics.simulate(**args, ReturnBounds=E > 1, device=device_ctx)
    assert 'members' not in again and np.array_equal(again.mean, dev.mean)
    assert E == 1 or np.array_equal(again.bounds, dev.bounds)
    if E == 130:                                                     # member e of a large run is member e run alone
        alone = dynamics.simulate(**{**args, 'y0': args['y0'][77]}, draws=np.array([77]), ReturnBounds=False, keep='members',
                                  device=device_ctx)
        assert np.array_equal(alone.members[0], dev.members[77])


@pytest.mark.parametrize('n_states', [1, 3, 8])
def test_every_instance_of_the_kernel(device_ctx, n_states):
    _compare(device_ctx, **_system(20 + n_states, n_states, 'bs', 5, steps=6, n_forcing=min(n_states - 1, 2)))
    rep = device_ctx.simulate_report()
    assert rep['NS'] == n_states and rep['workgroups'] == 1 and rep['members'] == 5


def test_term_shapes(device_ctx):
    """Terms of 1, 3 and 4 factors (the last continues in a second entry) next to a model that is only its constant."""
    rng = np.random.default_rng(31)
    E = 5
    first = _model('b', [0.05, 0.3, -0.4, 0.5, 0.2], [[1, 0, 0, 0], [1, 2, 1, 0], [1, 1, 2, 1], [0, 0, 0, 3]],
                   [[-1.0, 1.0], [-2.0, 2.0], [0.0, 10.0], [-3.0, 3.0]], E, rng)
    constant = _model('b', [0.4], np.zeros((0, 0)), [], E, rng)
    u = 5.0 + 4.0 * np.sin(np.arange(8) / 2.0)
    args = dict(models=[first, constant], states=['a', 'b'], inputs=[['a', 'b', 'u', 'w'], []],
                forcing={'u': u, 'w': np.linspace(-2.0, 2.0, 8)}, y0=[0.2, -0.3], t=(0.0, 0.275, 0.05))
    dev, host = _compare(device_ctx, **args)
    assert np.all(np.diff(host.members[:, 1], axis=1) > 0) and device_ctx.simulate_report()['NS'] == 2


@pytest.mark.parametrize('kinds', ['s', 'b', 'sb'])
def test_kernels_alone_and_mixed(device_ctx, kinds):
    _compare(device_ctx, **_system(40 + len(kinds), 2, kinds, 7, steps=6, n_forcing=1, orders=(1, 2, 7)))
    rep = device_ctx.simulate_report()
    assert (rep['spline_factors'] > 0) == ('s' in kinds) and (rep['bernoulli_factors'] > 0) == ('b' in kinds)


def test_bernoulli_orders_1_and_20(device_ctx):
    rng = np.random.default_rng(51)
    model = _model('b', [0.1, -0.5, 0.02, 0.01], [[1, 0], [20, 0], [1, 20]], [[-1.0, 1.0], [0.0, 10.0]], 9, rng)
    u = 5.0 + 4.0 * np.sin(np.arange(8) / 2.0)
    _compare(device_ctx, models=[model], states=['y'], inputs=[['y', 'u']], forcing={'u': u},
             y0=np.linspace(-0.9, 0.9, 9)[:, None], t=(0.0, 0.275, 0.05))


def test_spline_inputs_on_the_knots(device_ctx):
    """The state's range is [0, 499], so y = k is v = k / 499: v = 0, several knots and v = 1 start a member each; the
    small slopes keep the first stages on or next to the knot."""
    rng = np.random.default_rng(61)
    model = _model('s', [0.0, 0.5, -0.4, 0.3], [[1], [2], [7]], [[0.0, 499.0]], 12, rng)
    model['betas'][:, 0] = 0.0
    model['betas'][::2] *= 1e-3
    y0 = np.array([0.0, 0.0, 1.0, 1.0, 2.0, 250.0, 250.0, 497.0, 498.0, 498.0, 499.0, 499.0])[:, None]
    dev, host = _compare(device_ctx, models=[model], states=['y'], inputs=[['y']], y0=y0, t=(0.0, 0.275, 0.05))
    assert (host.first_saturation[[0, 1, 10, 11]] >= -1).all()


@pytest.mark.parametrize('n_forcing', [0, 1, 2])
def test_forcing_none_one_and_two_columns(device_ctx, n_forcing):
    args = _system(70 + n_forcing, 2, 'bs', 6, steps=7, n_forcing=n_forcing)
    assert sorted({name for names in args['inputs'] for name in names if name.startswith('u')}) == [f'u{c}' for c in range(n_forcing)]
    _compare(device_ctx, **args)


def test_the_horizon_cut_changes_no_bit(device_ctx, monkeypatch):
    args = _system(80, 2, 'sb', 70, steps=11, n_forcing=1)
    monkeypatch.delenv('FOKL_SIMULATE_STEPS_PER_LAUNCH', raising=False)
    whole, _ = _compare(device_ctx, **args)
    assert device_ctx.simulate_report()['launches'] == 1
    for per_launch, launches in (('1', 11), ('5', 3)):
        monkeypatch.setenv('FOKL_SIMULATE_STEPS_PER_LAUNCH', per_launch)
        cut_up = dynamics.simulate(**args, keep='members', device=device_ctx)
        rep = device_ctx.simulate_report()
        assert rep['launches'] == launches and rep['steps_per_launch'] == int(per_launch)
        for key in ('members', 'mean', 'bounds', 'first_saturation'):
            assert np.array_equal(whole[key], cut_up[key]), (per_launch, key)


def test_shared_y0_sweep_and_mean_draws(device_ctx):
    args = _system(90, 2, 'b', 40, steps=6, n_forcing=1)
    shared, _ = _compare(device_ctx, **{**args, 'y0': args['y0'][0]})
    sweep, _ = _compare(device_ctx, **args)
    assert np.array_equal(shared.members[0], sweep.members[0]) and not np.array_equal(shared.members[1], sweep.members[1])
    one, _ = _compare(device_ctx, **{**args, 'y0': args['y0'][0]}, draws='mean', ReturnBounds=False)
    assert one.members.shape[0] == 1 and np.array_equal(one.mean, one.members[0])
    _compare(device_ctx, **args, draws='mean')                       # the mean model over the sweep of initial states


def test_saturation_flags_and_trajectories(device_ctx):
    """Half the members get a large positive constant and run into the upper edge of the box; one starts outside a
    model's range of a state, so the clamp acts in its first stage."""
    rng = np.random.default_rng(100)
    E = 66
    first = _model('b', [0.1, -0.3, 0.2], [[1, 0], [0, 2]], [[-1.0, 1.0], [-2.0, 2.0]], E, rng)
    second = _model('s', [-0.05, 0.3, -0.2], [[1, 0], [1, 2]], [[-1.5, 1.5], [-0.5, 0.5]], E, rng)
    first['betas'][::2, 0] = 6.0
    y0 = rng.uniform(-0.4, 0.4, (E, 2))
    y0[5] = [-0.6, 0.2]                                              # p below the second model's range of it: a clamp in step 0
    dev, host = _compare(device_ctx, models=[first, second], states=['p', 'q'], inputs=[['p', 'q'], ['q', 'p']], y0=y0,
                         t=(0.0, 0.975, 0.05))
    assert (host.first_saturation[::2] >= 0).all() and host.first_saturation[5] == 0
    assert 0 < (host.first_saturation < 0).sum() < E and 0.5 <= dev.saturated_fraction < 1.0
    assert (host.members[::2, 0, -1] >= 0.5).all()                   # the box of p is [-0.5, 0.5]


@pytest.mark.parametrize('nan_draws', [(1,), (1, 40)])
def test_the_band_next_to_nan_members(device_ctx, nan_draws):
    """The two-state system of tests/test_simulate_adaptive_host.py with 70 draws, of which ``nan_draws`` hold a NaN
    coefficient: every member is the host statement's bit for bit (NaN where it is NaN), the bounds are np.sort's order
    statistics of the returned members and the host statement's own, the mean is the band kernel's summation tree over the
    host's members.  Cut 2: with one NaN member the upper bound is the largest finite value, with two it is NaN."""
    args = {key: value for key, value in nan_system(draws=70, nan_draws=nan_draws, ReturnBounds=True).items() if key != 'max_halvings'}
    host = dynamics.simulate_host(**args, keep='members')
    dev = dynamics.simulate(**args, keep='members', device=device_ctx)
    assert same_rows(dev.members, host.members) and np.array_equal(dev.first_saturation, host.first_saturation)
    lower, upper = band_rows(dev.members, bounds_cut(70))
    assert same_rows(dev.bounds[..., 0], lower) and same_rows(dev.bounds[..., 1], upper) and same_rows(dev.bounds, host.bounds)
    assert same_rows(dev.mean, mean_rows(host.members)) and np.array_equal(np.isnan(dev.mean), np.isnan(host.mean))
    band_next_to_nan(dev.members, dev.mean, dev.bounds, nan_draws, bounds_cut(70))


def test_end_to_end_between_fits(device_ctx):
    """A small Bernoulli fit on the device, a 1-state system simulated from its draws on the same backend, then the same
    fit again: bit for bit as before, so simulate leaves the context clean."""
    from fokl_gpy_amd import FoKLRoutines
    rng = np.random.default_rng(31)
    n = 600
    x = rng.random((n, 2))
    data = 0.6 * np.sin(3 * x[:, 1]) - 0.8 * x[:, 0] + 0.01 * rng.standard_normal(n)

    def fit():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', burnin=60, draws=60, tolerance=2, UserWarnings=False,
                                      ConsoleOutput=False)
            np.random.seed(40)
            betas, mtx, _ = model.fit(x, data, clean=True)
        return model, np.array(betas), np.array(mtx)

    model, betas, mtx = fit()
    state = np.random.get_state()[1].copy()
    args = dict(models=[model], states=['y'], inputs=[['y', 'u']], forcing={'u': 0.5 + 0.4 * np.sin(np.arange(20) / 3.0)},
                y0=[0.3], t=(0.0, 0.95, 0.05))
    dev, host = _compare(FoKLRoutines.device_backend(), **args)
    assert dev.members.shape == (betas.shape[0], 1, 20)
    assert (dev.bounds[..., 0] <= dev.bounds[..., 1]).all() and (dev.members.max(0) > dev.members.min(0)).any()
    assert np.array_equal(np.random.get_state()[1], state)           # numpy's stream is left alone
    model_again, betas_again, mtx_again = fit()
    assert np.array_equal(mtx_again, mtx) and np.array_equal(betas_again, betas)
    assert np.isfinite(model_again.evaluate(x)).all()

"""dynamics.simulate_adaptive on the MI355X against its statement dynamics.simulate_adaptive_host (pinned without a device by
tests/test_simulate_adaptive_host.py): every member, every level and every record bit for bit; a forced level against the
device's own simulate on the refined grid; the bounds as the order statistics of the returned members, the mean within the
rounding of a sum of E terms.  The shapes are the smallest at which the kernel can go wrong: lanes that pad a wavefront, more
than one workgroup, lanes of one wavefront at different levels, every instance of the kernel, one step per launch."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from band_reference import band_next_to_nan, band_rows, mean_rows, same_rows
from fokl_gpy_amd import dynamics, getKernels
from fokl_gpy_amd.GP_Integrate import bounds_cut
from test_simulate_adaptive_host import nan_system, refined, stiff_linear, wall_system

pytestmark = pytest.mark.gpu

BERN = getKernels.bernoulli()
SPLINES = getKernels.table_to_phis(np.load(os.path.join(GOLDEN, 'spline_phis.npz'))['table'])
KERNELS = {'b': ('Bernoulli Polynomials', BERN), 's': ('Cubic Splines', SPLINES)}
RECORD = ('first_saturation', 'pairs', 'rejected', 'max_level', 'error', 'first_unresolved', 'levels')
DTYPES = dict(first_saturation=np.int32, pairs=np.int64, rejected=np.int64, max_level=np.int32, error=np.float64,
              first_unresolved=np.int32, levels=np.int8)
H = 0.0625


def _system(seed, n_states, kinds, E, steps, n_forcing=0, orders=(1, 2, 3), stiffness=1.0, spread=1.0):
    """tests/test_simulate_gpu.py's system on a dyadic grid: model k reads its own state, the next one and (with forcing)
    column k % n_forcing, each through a range of its own; one term per column plus their product.  ``stiffness`` scales
    every coefficient, and member e's once more by a factor that grows evenly from 1 to ``spread`` over the members."""
    rng = np.random.default_rng(seed)
    states = [f'x{k}' for k in range(n_states)]
    forcing = {f'u{c}': 5.0 + 4.0 * np.sin(np.arange(steps) / (2.0 + c)) for c in range(n_forcing)}
    models, inputs = [], []
    for k in range(n_states):
        names = [states[k]] + ([states[(k + 1) % n_states]] if n_states > 1 else []) + ([f'u{k % n_forcing}'] if n_forcing else [])
        m = len(names)
        mtx = np.concatenate([np.diag(rng.choice(orders, size=m)), np.ones((1, m), dtype=int)])
        minmax = [[0.0, 10.0] if name in forcing else [-1.0 - 0.125 * k, 1.0 + 0.25 * k] for name in names]
        mean = stiffness * 0.3 * rng.standard_normal(m + 2)
        kernel, phis = KERNELS[kinds[k % len(kinds)]]
        betas = mean * (1 + 0.1 * rng.standard_normal((E, m + 2))) * np.linspace(1.0, spread, E)[:, None]
        models.append(dict(betas=betas, mtx=mtx, phis=phis, minmax=minmax,
                           kernel=kernel))
        inputs.append(names)
    return dict(models=models, states=states, inputs=inputs, forcing=forcing, y0=rng.uniform(-0.5, 0.5, (E, n_states)),
                t=(0.0, steps * H, H))


def _compare(ctx, **args):
    """simulate_adaptive against simulate_adaptive_host in every field -> (device result, host result)."""
    host = dynamics.simulate_adaptive_host(**args, keep=('members', 'levels'))
    dev = dynamics.simulate_adaptive(**args, keep=('members', 'levels'), device=ctx)
    E = host.members.shape[0]
    assert dev.members.shape == host.members.shape and np.array_equal(dev.t, host.t)
    differ = ~((dev.members == host.members) | (np.isnan(dev.members) & np.isnan(host.members)))
    if differ.any():
        e, k, q = np.argwhere(differ)[0]
        print(f"\n{int(differ.sum())} values differ, first at member {e} state {k} point {q}: device {dev.members[e, k, q]!r} "
              f"host {host.members[e, k, q]!r}; pairs {dev.pairs[e]} / {host.pairs[e]}, rejected {dev.rejected[e]} / {host.rejected[e]}")
    assert not differ.any()
    for key in RECORD:
        assert dev[key].dtype == DTYPES[key] and dev[key].shape == host[key].shape, key
        assert np.array_equal(dev[key], host[key]), (key, dev[key], host[key])
    assert dev.saturated_fraction == host.saturated_fraction and dev.unresolved_fraction == host.unresolved_fraction
    rep = ctx.simulate_adaptive_report()
    assert rep['pairs'] == host.pairs.sum() and rep['rejected'] == host.rejected.sum() and rep['members'] == E
    assert rep['NS'] == host.members.shape[1] and rep['workgroups'] == -(-E // 64)
    finite = np.isfinite(host.members).all(axis=0)
    if args.get('ReturnBounds', True):
        lower, upper = band_rows(dev.members, bounds_cut(E))          # np.sort's order statistics: a NaN member sorts last
        assert same_rows(dev.bounds[..., 0], lower) and same_rows(dev.bounds[..., 1], upper)
        assert same_rows(dev.bounds, host.bounds)                    # the members are the host's, so are the bounds
    else:
        assert 'bounds' not in dev
    with np.errstate(invalid='ignore'):
        close = np.abs(dev.mean - dev.members.mean(0)) <= E * 2.0 ** -52 * np.max(np.abs(dev.members), axis=0)
    assert np.all(close[finite]) and np.isnan(dev.mean[~finite]).all()
    # the mean bit for bit: the kernel's order of additions over the host's members, NaN where the host's mean is NaN
    assert same_rows(dev.mean, mean_rows(host.members)) and np.array_equal(np.isnan(dev.mean), np.isnan(host.mean))
    return dev, host


# ---------------------------------------------------------------------------------------------------------
# 1. padding, lanes and workgroups
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 63, 64, 65, 130])
def test_members_pad_lanes_and_fill_workgroups(device_ctx, E):
    args = _system(10 + E, 2, 'b', E, steps=6, n_forcing=1, stiffness=2.0, spread=8.0)
    forced, _ = _compare(device_ctx, **args, ReturnBounds=E > 1, min_halvings=2, max_halvings=2)
    assert (forced.pairs == 6 * 4).all() and not forced.rejected.any()
    dev, host = _compare(device_ctx, **args, ReturnBounds=E > 1)
    rep = device_ctx.simulate_adaptive_report()
    assert rep['NS'] == 2 and rep['members'] == E and rep['workgroups'] == -(-E // 64) and rep['launches'] == 1
    assert rep['lds_bytes'] % 512 == 0 and rep['spline_factors'] == 0 and rep['bernoulli_factors'] > 0
    assert (rep['min_halvings'], rep['max_halvings'], rep['steps_per_launch']) == (0, 10, 64)
    assert dev.members.shape == (E, 2, 7)
    if E >= 63:
        assert host.rejected.sum() > 0                               # the free run is not the output grid's
    again = dynamics.simulate_adaptive(**args, ReturnBounds=E > 1, device=device_ctx)    # reproducible, and without the members
    assert 'members' not in again and 'levels' not in again and np.array_equal(again.mean, dev.mean)
    assert E == 1 or np.array_equal(again.bounds, dev.bounds)
    assert np.array_equal(again.pairs, dev.pairs) and np.array_equal(again.error, dev.error)
    if E == 130:                                                     # member e of a large run is member e run alone
        alone = dynamics.simulate_adaptive(**{**args, 'y0': args['y0'][77]}, draws=np.array([77]), ReturnBounds=False,
                                           keep=('members', 'levels'), device=device_ctx)
        assert np.array_equal(alone.members[0], dev.members[77])
        for key in RECORD:
            assert np.array_equal(alone[key][0], dev[key][77]), key


# ---------------------------------------------------------------------------------------------------------
# 2. a forced level against the device's own simulate, every instance of the kernel
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_states', [1, 3, 8])
def test_forced_level_is_the_devices_own_simulate_on_the_refined_grid(device_ctx, n_states):
    args = _system(20 + n_states, n_states, 'bs', 5, steps=6, n_forcing=min(n_states - 1, 2))
    got = dynamics.simulate_adaptive(**args, keep='members', min_halvings=1, max_halvings=1, device=device_ctx)
    rep = device_ctx.simulate_adaptive_report()
    assert rep['NS'] == n_states and rep['bernoulli_factors'] > 0 and (n_states == 1 or rep['spline_factors'] > 0)
    fine_args, n = refined(args, 1)
    fine = dynamics.simulate(**fine_args, keep='members', device=device_ctx)
    assert n == 4 and fine.members.shape[2] == 6 * n + 1 and np.isfinite(fine.members).all()
    assert np.array_equal(got.members, fine.members[:, :, ::n])
    assert np.array_equal(got.first_saturation, fine.first_saturation // n)
    assert (got.pairs == 12).all() and not got.rejected.any() and (got.max_level == 1).all()


# ---------------------------------------------------------------------------------------------------------
# 3. lanes of one wavefront at different levels
# ---------------------------------------------------------------------------------------------------------

def divergent_system():
    """70 members of the stiff linear family, b h spread evenly over [-0.5, -8], the initial state swept over the box."""
    args, _, _ = stiff_linear(np.linspace(-0.5, -8.0, 70), y0=np.linspace(0.25, 3.75, 70), steps=12)
    return args


@pytest.fixture(scope='module')
def divergent_host():
    host = dynamics.simulate_adaptive_host(**divergent_system(), keep=('members', 'levels'))
    wave = slice(0, 64)
    assert len(set(host.max_level[wave].tolist())) >= 3 and host.rejected[wave].sum() >= 1
    assert (np.diff(host.levels[wave].astype(int), axis=1) < 0).any()      # a lane relaxed its level between two steps
    return host


def test_divergent_lanes(device_ctx, divergent_host):
    dev, host = _compare(device_ctx, **divergent_system())
    assert np.array_equal(host.members, divergent_host.members) and np.array_equal(host.levels, divergent_host.levels)
    assert (dev.first_unresolved == -1).all() and dev.error.max() <= 1.0


# ---------------------------------------------------------------------------------------------------------
# 4. nonlinear, several states
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_states', [3, 8])
def test_nonlinear_systems_of_several_states(device_ctx, n_states):
    args = _system(40 + n_states, n_states, 'sb', 9, steps=5, n_forcing=min(n_states - 1, 2), orders=(1, 2, 7), stiffness=6.0,
                   spread=2.0)
    dev, host = _compare(device_ctx, **args)
    print(f"\n{n_states} states: pairs {host.pairs.tolist()}, rejected {host.rejected.tolist()}, max level {host.max_level.tolist()}")
    assert host.rejected.sum() >= 1 and host.max_level.max() >= 1


# ---------------------------------------------------------------------------------------------------------
# 5. the launch cut changes no bit
# ---------------------------------------------------------------------------------------------------------

def test_the_launch_cut_changes_no_bit(device_ctx, divergent_host, monkeypatch):
    args = divergent_system()
    monkeypatch.delenv('FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH', raising=False)
    whole = dynamics.simulate_adaptive(**args, keep=('members', 'levels'), device=device_ctx)
    assert device_ctx.simulate_adaptive_report()['launches'] == 1
    monkeypatch.setenv('FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH', '1')
    cut_up = dynamics.simulate_adaptive(**args, keep=('members', 'levels'), device=device_ctx)
    rep = device_ctx.simulate_adaptive_report()
    assert rep['launches'] == 12 and rep['steps_per_launch'] == 1
    for key in ('members', 'mean', 'bounds') + RECORD:
        assert np.array_equal(whole[key], cut_up[key]), key
        assert key in ('mean', 'bounds') or np.array_equal(whole[key], divergent_host[key]), key


# ---------------------------------------------------------------------------------------------------------
# 6. the wall and the NaN member
# ---------------------------------------------------------------------------------------------------------

def test_the_wall_of_the_box_is_reported_as_unresolved(device_ctx):
    dev, host = _compare(device_ctx, **wall_system(), max_halvings=6)
    reaches = int(np.flatnonzero(host.members[0, 0, 1:] >= 1.0)[0])
    assert dev.first_unresolved.tolist() == [reaches] and dev.max_level.tolist() == [6] and dev.error[0] > 1.0


def test_a_nan_member_ends_and_stays_local(device_ctx):
    args = nan_system()
    dev, host = _compare(device_ctx, **args)
    assert dev.first_unresolved.tolist() == [-1, 0, -1] and np.isfinite(dev.error).all() and dev.pairs[1] == 4 * 2 ** 5
    for e in (0, 2):
        alone = dynamics.simulate_adaptive(**args, draws=np.array([e]), keep=('members', 'levels'), device=device_ctx)
        assert np.array_equal(alone.members[0], dev.members[e])
        for key in RECORD:
            assert np.array_equal(alone[key][0], dev[key][e]), key


@pytest.mark.parametrize('nan_draws', [(1,), (1, 40)])
def test_the_band_next_to_nan_members(device_ctx, nan_draws):
    """70 draws, cut 2: with one NaN member the upper bound is the largest finite value, with two it is NaN; the lower
    bound stays finite and the mean is NaN wherever a member is -- the host statement's np.sort and np.mean (``_compare``)."""
    dev, host = _compare(device_ctx, **nan_system(draws=70, nan_draws=nan_draws, ReturnBounds=True))
    band_next_to_nan(dev.members, dev.mean, dev.bounds, nan_draws, bounds_cut(70))


# ---------------------------------------------------------------------------------------------------------
# 7. mean and bounds
# ---------------------------------------------------------------------------------------------------------

def test_mean_and_bounds_are_formed_from_the_returned_members(device_ctx, monkeypatch):
    """More members than one workgroup and three launches of four steps: the band and the mean of every launch's points
    (``_compare``)."""
    args = _system(70, 2, 'sb', 100, steps=9, n_forcing=1, spread=8.0)
    monkeypatch.setenv('FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH', str(4 << 8))
    dev, _ = _compare(device_ctx, **args, max_halvings=8)
    assert device_ctx.simulate_adaptive_report()['launches'] == 3
    assert dev.bounds.shape == (2, 10, 2) and (dev.bounds[..., 0] <= dev.bounds[..., 1]).all()
    assert (dev.bounds[:, 1:, 0] < dev.bounds[:, 1:, 1]).any() and dev.mean.shape == (2, 10)

"""dynamics.simulate_stiff on the MI355X against its statement dynamics.simulate_stiff_host (pinned without a device by
tests/test_simulate_stiff_host.py): every member, every level and every record bit for bit; the bounds as the order
statistics of the returned members, the mean within the rounding of a sum of E terms.  The shapes are the smallest at which
the kernel can go wrong: lanes that pad a wavefront, more than one workgroup, lanes of one wavefront at different levels, the
instances 1, 2, 3 and 8 of the kernel, row exchanges in the factorisation, a few steps per launch.  max_halvings <= 6 and at
most 16 output steps throughout."""
import numpy as np
import pytest

from fokl_gpy_amd import dynamics
from fokl_gpy_amd.GP_Integrate import bounds_cut
from band_reference import band_next_to_nan, band_rows, mean_rows, same_rows
from test_simulate_adaptive_gpu import _system
from test_simulate_adaptive_host import nan_system, stiff_linear, wall_system
from test_simulate_stiff_host import DTYPES, RATES, closed_form, rotating_system

pytestmark = pytest.mark.gpu

RECORD = ('first_saturation', 'steps', 'rejected', 'swaps', 'max_level', 'error', 'first_unresolved', 'levels')
TOP = 6


def _compare(ctx, **args):
    """simulate_stiff against simulate_stiff_host in every field -> (device result, host result)."""
    args.setdefault('max_halvings', TOP)
    host = dynamics.simulate_stiff_host(**args, keep=('members', 'levels'))
    dev = dynamics.simulate_stiff(**args, keep=('members', 'levels'), device=ctx)
    E = host.members.shape[0]
    assert dev.members.shape == host.members.shape and np.array_equal(dev.t, host.t)
    differ = ~((dev.members == host.members) | (np.isnan(dev.members) & np.isnan(host.members)))
    if differ.any():
        e, k, q = np.argwhere(differ)[0]
        print(f"\n{int(differ.sum())} values differ, first at member {e} state {k} point {q}: device {dev.members[e, k, q]!r} "
              f"host {host.members[e, k, q]!r}; steps {dev.steps[e]} / {host.steps[e]}, rejected {dev.rejected[e]} / "
              f"{host.rejected[e]}, swaps {dev.swaps[e]} / {host.swaps[e]}")
    assert not differ.any()
    for key in RECORD:
        assert dev[key].dtype == DTYPES[key] and dev[key].shape == host[key].shape, key
        assert np.array_equal(dev[key], host[key]), (key, dev[key], host[key])
    assert dev.saturated_fraction == host.saturated_fraction and dev.unresolved_fraction == host.unresolved_fraction
    rep = ctx.simulate_stiff_report()
    assert rep['steps'] == host.steps.sum() and rep['rejected'] == host.rejected.sum() and rep['swaps'] == host.swaps.sum()
    assert rep['NS'] == host.members.shape[1] and rep['members'] == E and rep['workgroups'] == -(-E // 64)
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
# 8a. padding, lanes and workgroups; 10. member e of a large run is member e run alone
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 64, 65, 130])
def test_members_pad_lanes_and_fill_workgroups(device_ctx, E):
    args = _system(10 + E, 2, 'b', E, steps=6, n_forcing=1, stiffness=2.0, spread=8.0)
    dev, host = _compare(device_ctx, **args, ReturnBounds=E > 1)
    rep = device_ctx.simulate_stiff_report()
    assert rep['launches'] == 1 and rep['lds_bytes'] % 512 == 0 and rep['lds_bytes'] >= 512 * dynamics.stiff_lds_rows(2, 2, 10)
    assert (rep['min_halvings'], rep['max_halvings'], rep['steps_per_launch']) == (0, TOP, 65536 >> TOP)
    assert dev.members.shape == (E, 2, 7)
    again = dynamics.simulate_stiff(**args, ReturnBounds=E > 1, max_halvings=TOP, device=device_ctx)
    assert 'members' not in again and 'levels' not in again and np.array_equal(again.mean, dev.mean)
    assert E == 1 or np.array_equal(again.bounds, dev.bounds)
    assert np.array_equal(again.steps, dev.steps) and np.array_equal(again.error, dev.error)
    if E == 130:
        for e in (5, 77):                                            # one of each workgroup
            alone = dynamics.simulate_stiff(**{**args, 'y0': args['y0'][e]}, draws=np.array([e]), ReturnBounds=False,
                                            keep=('members', 'levels'), max_halvings=TOP, device=device_ctx)
            assert np.array_equal(alone.members[0], dev.members[e])
            for key in RECORD:
                assert np.array_equal(alone[key][0], dev[key][e]), key


# ---------------------------------------------------------------------------------------------------------
# 8b. the instances of the kernel: Bernoulli, splines and mixed models, with and without forcing
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_states, kinds, n_forcing', [(1, 's', 0), (1, 'b', 1), (2, 's', 1), (2, 'bs', 0), (3, 'sb', 2),
                                                        (8, 'bs', 2), (8, 'b', 0)])
def test_every_instance_and_kernel(device_ctx, n_states, kinds, n_forcing):
    args = _system(40 + 3 * n_states + n_forcing, n_states, kinds, 9, steps=5, n_forcing=n_forcing, orders=(1, 2, 7),
                   stiffness=6.0, spread=2.0)
    dev, host = _compare(device_ctx, **args)
    print(f"\n{n_states} states '{kinds}': steps {host.steps.tolist()}, rejected {host.rejected.tolist()}, swaps "
          f"{host.swaps.tolist()}, max level {host.max_level.tolist()}")
    assert device_ctx.simulate_stiff_report()['NS'] == n_states and np.all(host.steps >= 5)


# ---------------------------------------------------------------------------------------------------------
# 8c. lanes of one wavefront at different levels; 9. the launch cut
# ---------------------------------------------------------------------------------------------------------

def divergent_system():
    """70 members of the stiff linear family, b h spread evenly over [-0.5, -200], the initial state swept over the box."""
    args, _, _ = stiff_linear(np.linspace(-0.5, -200.0, 70), y0=np.linspace(0.25, 3.75, 70), steps=12)
    return dict(args, max_halvings=TOP)


@pytest.fixture(scope='module')
def divergent_host():
    host = dynamics.simulate_stiff_host(**divergent_system(), keep=('members', 'levels'))
    wave = slice(0, 64)
    assert host.rejected.max() > 0 and len(set(host.max_level[wave].tolist())) >= 3
    assert (np.diff(host.levels[wave].astype(int), axis=1) < 0).any()      # a lane relaxed its level between two steps
    return host


def test_divergent_lanes(device_ctx, divergent_host):
    dev, host = _compare(device_ctx, **divergent_system())
    assert np.array_equal(host.members, divergent_host.members) and np.array_equal(host.levels, divergent_host.levels)
    assert dev.rejected.max() > 0 and len(set(dev.max_level[:64].tolist())) > 1


def test_the_launch_cut_changes_no_bit(device_ctx, divergent_host, monkeypatch):
    args = divergent_system()
    monkeypatch.delenv('FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH', raising=False)
    whole = dynamics.simulate_stiff(**args, keep=('members', 'levels'), device=device_ctx)
    assert device_ctx.simulate_stiff_report()['launches'] == 1
    monkeypatch.setenv('FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH', str(5 << TOP))
    cut_up = dynamics.simulate_stiff(**args, keep=('members', 'levels'), device=device_ctx)
    rep = device_ctx.simulate_stiff_report()
    assert rep['launches'] == 3 and rep['steps_per_launch'] == 5      # 5 + 5 + 2 steps
    for key in ('members', 'mean', 'bounds') + RECORD:
        assert np.array_equal(whole[key], cut_up[key]), key
        assert key in ('mean', 'bounds') or np.array_equal(whole[key], divergent_host[key]), key
    monkeypatch.setenv('FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH', '1')
    single = dynamics.simulate_stiff(**args, keep=('members', 'levels'), device=device_ctx)
    assert device_ctx.simulate_stiff_report()['launches'] == 12
    for key in ('members', 'mean', 'bounds') + RECORD:
        assert np.array_equal(whole[key], single[key]), key


# ---------------------------------------------------------------------------------------------------------
# 8d. row exchanges
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_states', [2, 3, 8])
def test_the_factorisation_exchanges_rows(device_ctx, n_states):
    args = rotating_system(E=70, n_states=n_states)
    dev, host = _compare(device_ctx, **args)
    assert (host.swaps > 0).all() and (host.swaps < (n_states + 1) // 2 * host.steps).any()
    forced, _ = _compare(device_ctx, **args, min_halvings=0, max_halvings=0)
    print(f"\n{n_states} states: exchanges per step at level 0 {(forced.swaps // forced.steps).tolist()[:4]} ...")
    assert np.all(forced.swaps >= n_states // 2 * forced.steps)      # every pair's first column takes the row below


# ---------------------------------------------------------------------------------------------------------
# 8e. the wall and the NaN member
# ---------------------------------------------------------------------------------------------------------

def test_the_wall_of_the_box_is_reported_as_unresolved(device_ctx):
    dev, host = _compare(device_ctx, **wall_system())
    assert dev.first_saturation[0] > 0 and dev.first_unresolved[0] >= 0 and dev.max_level.tolist() == [TOP]
    assert dev.error[0] > 1.0 and dev.members[0, 0, -1] >= 1.0 - 1e-9


def test_a_nan_member_ends_and_stays_local(device_ctx):
    args = nan_system()
    dev, host = _compare(device_ctx, **args)
    assert dev.first_unresolved.tolist() == [-1, 0, -1] and np.isfinite(dev.error).all() and dev.steps[1] == 4 * 2 ** 5
    for e in (0, 2):
        alone = dynamics.simulate_stiff(**args, draws=np.array([e]), keep=('members', 'levels'), device=device_ctx)
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
# 11. a forced level is the stability function
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L', [0, 2])
def test_forced_level_is_the_stability_function(device_ctx, L):
    args, b, fixed = stiff_linear(RATES, steps=16)
    dev = dynamics.simulate_stiff(**args, keep=('members', 'levels'), min_halvings=L, max_halvings=L, device=device_ctx)
    err = np.max(np.abs(dev.members[:, 0] - closed_form(b, fixed, L, 17)), axis=1)
    print(f"\nlevel {L}: distance to the closed form {err.tolist()}")
    assert np.all(err <= 1e-11 * (1.0 + 2.0))
    assert np.array_equal(dev.steps, np.full(5, 16 * 2 ** L)) and not dev.rejected.any() and (dev.levels == L).all()


# ---------------------------------------------------------------------------------------------------------
# the entry point repeats the checks
# ---------------------------------------------------------------------------------------------------------

def test_the_entry_point_refuses_what_the_plan_refuses(device_ctx):
    """A system that simulate_adaptive's plan still takes (288 values per member) handed to the entry point directly: the
    tangent rows make it 291.  Then a tolerance and levels the plan would have refused."""
    from fokl_gpy_amd import _capi
    from test_simulate_adaptive_host import _bern_model
    fits = _bern_model(np.full((2, 285), 0.01), np.tile([[1]], (284, 1)), [[0.0, 1.0]])
    plan = dynamics._prepare_adaptive([fits], ['y'], [['y']], None, [0.5], (0.0, 1.0, 0.125), None, None, True, None, 1e-4, None,
                                      0, TOP)
    with pytest.raises(_capi.FoklNativeError, match=r'needs 291 values per member in LDS .*tangent rows.* 144 KB hold 288'):
        device_ctx.simulate_stiff(plan)
    assert device_ctx.simulate_stiff_report()['launches'] == 0
    args, _, _ = stiff_linear([-1.0, -2.0], steps=4)
    good = dynamics._prepare_stiff(args['models'], args['states'], args['inputs'], None, args['y0'], args['t'], None, None, True,
                                   None, 1e-4, None, 0, TOP)
    for change, match in ((dict(rtol=-1.0), 'rtol must be finite and not negative'), (dict(atol=np.array([np.nan])), 'atol must be'),
                          (dict(max_halvings=13), '0 <= min_halvings <= max_halvings <= 12')):
        with pytest.raises(_capi.FoklNativeError, match=match):
            device_ctx.simulate_stiff({**good, **change})
    assert device_ctx.simulate_stiff_report()['NS'] == 0
    device_ctx.simulate_stiff(good)
    assert device_ctx.simulate_stiff_report()['NS'] == 1

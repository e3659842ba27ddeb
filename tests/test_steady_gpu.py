"""dynamics.steady_states on the MI355X against its statement dynamics.steady_states_host (pinned without a device by
tests/test_steady_host.py): every per-member field bit for bit, the Jacobian included.  The shapes are the smallest at which
the kernel can go wrong: lanes that pad a wavefront, more than one workgroup, more than one operating point, lanes of one
wavefront that end in different ways, the instances 1, 2, 3 and 8 of the kernel, row exchanges in the factorisation, a few points
per launch.  At most 130 members and 3 points throughout."""
import numpy as np
import pytest

from fokl_gpy_amd import _capi, dynamics
from test_simulate_adaptive_gpu import _system
from test_simulate_adaptive_host import _bern_model
from test_simulate_stiff_host import rotating_system
from test_steady_host import DTYPES, FIELDS, cubic_system, linear_system, mixed_system, wall_root_system

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def _compare(ctx, **args):
    """steady_states against steady_states_host in every field -> (device result, host result)."""
    host = dynamics.steady_states_host(**args, keep='jacobian')
    dev = dynamics.steady_states(**args, keep='jacobian', device=ctx)
    for key in FIELDS:
        assert dev[key].dtype == DTYPES[key] and dev[key].shape == host[key].shape, key
        differ = ~((dev[key] == host[key]) | ((dev[key] != dev[key]) & (host[key] != host[key])))
        if differ.any():
            at = tuple(np.argwhere(differ)[0])
            print(f"\n{key}: {int(differ.sum())} values differ, first at {at}: device {dev[key][at]!r} host {host[key][at]!r}; "
                  f"status {dev.status[at[:3]]} / {host.status[at[:3]]}, iterations {dev.iterations[at[:3]]} / "
                  f"{host.iterations[at[:3]]}")
        assert not differ.any(), key
    for key in ('eig', 'stable', 'n_roots', 'n_stable', 'multiplicity', 'unique_fraction', 'unique_mean', 'unique_bounds'):
        assert np.array_equal(dev[key], host[key], equal_nan=True), key
    Q, E, S, K = host.y.shape
    rep = ctx.steady_report()
    assert (rep['NS'], rep['members'], rep['points'], rep['workgroups']) == (K, E * S, Q, -(-E * S // 64) * Q)
    assert rep['iterations'] == host.iterations.sum() and rep['halvings'] == host.halvings.sum()
    return dev, host


def _steady(seed, n_states, kinds, E, Q, n_forcing, **more):
    """tests/test_simulate_adaptive_gpu.py's system with its forcing rows as operating points."""
    args = _system(seed, n_states, kinds, E, steps=Q, n_forcing=n_forcing, **more)
    return dict(models=args['models'], states=args['states'], inputs=args['inputs'], at=args['forcing'])


# ---------------------------------------------------------------------------------------------------------
# padding, lanes, workgroups and points
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E, S', [(1, 1), (8, 8), (5, 13), (10, 13)])
@pytest.mark.parametrize('Q', [1, 3])
def test_members_pad_lanes_and_fill_workgroups(device_ctx, E, S, Q):
    args = _steady(10 + E, 2, 'b', E, Q, 1)
    dev, host = _compare(device_ctx, **args, starts=S)
    rep = device_ctx.steady_report()
    assert rep['launches'] == 1 and rep['lds_bytes'] % 512 == 0 and rep['lds_bytes'] >= 512 * dynamics.stiff_lds_rows(2, 2, 10)
    assert dev.y.shape == (Q, E, S, 2)
    print(f"\nE {E} S {S} Q {Q}: status counts {np.bincount(host.status.ravel(), minlength=4).tolist()}, iterations up to "
          f"{host.iterations.max()}, halvings up to {host.halvings.max()}")
    bare = dynamics.steady_states(**args, starts=S, device=device_ctx)
    assert 'jacobian' not in bare and np.array_equal(bare.stable, dev.stable) and _same(bare.y, dev.y)


@pytest.mark.parametrize('n_states, kinds, n_forcing', [(1, 's', 0), (1, 'b', 1), (2, 's', 1), (2, 'bs', 0), (3, 'sb', 2),
                                                        (8, 'bs', 2), (8, 'b', 0)])
def test_every_instance_and_kernel(device_ctx, n_states, kinds, n_forcing):
    args = _steady(40 + 3 * n_states + n_forcing, n_states, kinds, 5, 3 if n_forcing else 1, n_forcing, orders=(1, 2, 7))
    if not n_forcing:
        args.pop('at')
    dev, host = _compare(device_ctx, **args, starts=13)
    print(f"\n{n_states} states '{kinds}': status counts {np.bincount(host.status.ravel(), minlength=4).tolist()}, iterations up "
          f"to {host.iterations.max()}, halvings up to {host.halvings.max()}, held states {int(host.on_wall.sum())}")
    assert device_ctx.steady_report()['NS'] == n_states and host.iterations.max() >= 2


def test_closed_forms_on_the_device(device_ctx):
    args, A, B, c = linear_system()
    dev, _ = _compare(device_ctx, **args, at={'u': np.array([0.6, 1.7])})
    assert (dev.status == 0).all() and (dev.iterations <= 2).all() and dev.stable.all()
    dev, _ = _compare(device_ctx, **wall_root_system(), starts=5)
    assert dev.on_wall[..., 0].all() and (dev.y[..., 0] == 4.0).all() and (dev.status == 0).all()
    dev, _ = _compare(device_ctx, **mixed_system(), at={'u': np.array([0.2, 0.9])}, starts=7)
    assert (dev.status == 0).any()


# ---------------------------------------------------------------------------------------------------------
# lanes of one wavefront that end in different ways
# ---------------------------------------------------------------------------------------------------------

def divergent_system():
    """50 members in one wavefront at u = 1.9, where the draw with kappa = 1 has lost its two lower roots and the others have
    not: a start next to the remaining root (one iteration), starts that overshoot (line search), starts on the left of the
    vanished roots (stalled) and a draw with a NaN coefficient."""
    args = cubic_system((1.0, 1.25, 1.0, 1.5, 1.75), with_u=True)
    args['models'][0]['betas'][2, 2] = np.nan
    at = {'u': 1.9}
    upper = dynamics.steady_states_host(**args, at=at, draws=np.array([0]), starts=np.array([[3.9]])).y[0, 0, 0, 0]
    starts = np.concatenate([dynamics.steady_starts(9, np.array([[0.0, 4.0]])), [[upper + 1e-6]]])
    return dict(args, at=at, starts=starts)


def test_divergent_lanes(device_ctx):
    dev, host = _compare(device_ctx, **divergent_system())
    assert host.y.shape == (1, 5, 10, 1) and device_ctx.steady_report()['workgroups'] == 1
    assert host.iterations[0, 0, 9] == 1 and host.status[0, 0, 9] == 0
    assert (host.status[0, 0] == 2).any() and (host.status[0, 2] == 3).all() and (host.status[0, [1, 3, 4]] == 0).all()
    assert (host.halvings[host.status == 0] > 0).any() and len(set(host.iterations.ravel().tolist())) >= 4
    assert dev.n_roots.tolist() == [[1, 3, 0, 3, 3]]


# ---------------------------------------------------------------------------------------------------------
# invariances
# ---------------------------------------------------------------------------------------------------------

def test_a_draw_alone_a_point_alone_and_the_launch_cut(device_ctx, monkeypatch):
    args = _steady(21, 2, 'bs', 10, 3, 1)
    monkeypatch.delenv('FOKL_STEADY_POINTS_PER_LAUNCH', raising=False)
    whole, _ = _compare(device_ctx, **args, starts=13)
    assert device_ctx.steady_report()['launches'] == 1
    for e in (3, 7):                                                  # one of each workgroup
        alone = dynamics.steady_states(**args, starts=13, draws=np.array([e]), keep='jacobian', device=device_ctx)
        for key in FIELDS:
            assert _same(alone[key][:, 0], whole[key][:, e]), key
    for q in (0, 2):
        at = {name: values[q:q + 1] for name, values in args['at'].items()}
        alone = dynamics.steady_states(**{**args, 'at': at}, starts=13, keep='jacobian', device=device_ctx)
        for key in FIELDS:
            assert _same(alone[key][0], whole[key][q]), key
    for bound, launches in (('2', 2), ('1', 3)):
        monkeypatch.setenv('FOKL_STEADY_POINTS_PER_LAUNCH', bound)
        cut_up = dynamics.steady_states(**args, starts=13, keep='jacobian', device=device_ctx)
        rep = device_ctx.steady_report()
        assert rep['launches'] == launches and rep['iterations'] == whole.iterations.sum()
        for key in FIELDS:
            assert _same(cut_up[key], whole[key]), key


# ---------------------------------------------------------------------------------------------------------
# row exchanges
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_states', [2, 8])
def test_the_factorisation_exchanges_rows(device_ctx, n_states):
    system = rotating_system(E=10, n_states=n_states)
    args = dict(models=system['models'], states=system['states'], inputs=system['inputs'])
    dev, host = _compare(device_ctx, **args, starts=7)
    assert (host.status == 0).all() and np.max(np.abs(host.y - 2.0)) <= 1e-6 and host.iterations.max() >= 1
    _, _, exchanges = dynamics.stiff_lu(-np.moveaxis(host.jacobian.reshape(-1, n_states, n_states), 0, 2))
    assert np.all(exchanges >= n_states // 2)                         # every pair's first column takes the row below


# ---------------------------------------------------------------------------------------------------------
# the entry point repeats the checks
# ---------------------------------------------------------------------------------------------------------

def test_the_entry_point_refuses_what_the_plan_refuses(device_ctx):
    """A system that simulate's plan still takes (288 values per member) handed to the entry point directly: the tangent rows
    make it 291.  Then iteration limits and a tolerance the plan would have refused."""
    fits = _bern_model(np.full((2, 285), 0.01), np.tile([[1]], (284, 1)), [[0.0, 1.0]])
    plan = dynamics._prepare([fits], ['y'], [['y']], None, [0.5], (0.0, 1.0, 1.0), None, None, False, None)
    plan.update(Q=1, S=1, starts=np.array([[0.5]]), ftol=np.array([1e-9]), max_iter=50, max_halvings=8)
    with pytest.raises(_capi.FoklNativeError, match=r'needs 291 values per member in LDS .*tangent rows.* 144 KB hold 288'):
        device_ctx.steady_states(plan)
    assert set(device_ctx.steady_report().values()) == {0}
    good = dynamics._prepare_steady(**cubic_system(), at=None, draws=None, bounds=None, starts=9, ftol=None, time_scale=1.0,
                                    max_iter=50, max_halvings=8, merge_tol=1e-6, keep=None)
    for change, match in ((dict(max_iter=0), r'max_iter must lie in 1\.\.200'), (dict(max_iter=201), r'max_iter must lie in 1\.\.200'),
                          (dict(max_halvings=-1), r'max_halvings must lie in 0\.\.30'),
                          (dict(max_halvings=31), r'max_halvings must lie in 0\.\.30'),
                          (dict(ftol=np.array([0.0])), 'ftol must be positive and finite'),
                          (dict(ftol=np.array([np.nan])), 'ftol must be positive and finite'),
                          (dict(box=np.array([[1.0, 1.0]])), "a state's box is empty")):
        with pytest.raises(_capi.FoklNativeError, match=match):
            device_ctx.steady_states({**good, **change})
        assert set(device_ctx.steady_report().values()) == {0}
    out = device_ctx.steady_states(good)
    rep = device_ctx.steady_report()
    assert (rep['NS'], rep['members'], rep['points'], rep['launches'], rep['workgroups']) == (1, 36, 1, 1, 1)
    assert rep['lds_bytes'] == 512 * dynamics.stiff_lds_rows(3, 1, 4) and rep['iterations'] == out[2].sum() > 0
    assert rep['halvings'] == out[4].sum()

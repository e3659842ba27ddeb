"""GP_Integrate over an ensemble (one integration per posterior draw / initial state, on the device): argument handling
without a device, and on the MI355X every member against the host integrator -- itself pinned to the reference's own
trajectory by tests/golden/gp_integrate.npz (test_gp_integrate.py)."""
import os
import warnings

import numpy as np
import pytest

from helpers import GOLDEN
from band_reference import band_next_to_nan, band_rows, mean_rows, same_rows
from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd.GP_Integrate import GP_Integrate, GP_Integrate_ensemble, bounds_cut


def _case():
    g = np.load(os.path.join(GOLDEN, 'gp_integrate.npz'))
    phis = getKernels.table_to_phis(np.load(os.path.join(GOLDEN, 'spline_phis.npz'))['table'])
    return g, phis, [g['betas0'], g['betas1']], [g['mtx0'], g['mtx1']]


def _golden_args(g, phis, betas, mtx, y0):
    return (betas, mtx, g['b'], g['norms'], phis, float(g['start']), float(g['stop']), y0, float(g['h']),
            [row for row in g['used']])


class _Reached(Exception):
    pass


class _NoDevice(_capi.DeviceContext):
    """Stands where the device context would be: the CPU tests end here, after every check that needs no device."""

    def __init__(self):
        self._h = None

    def gp_integrate_ensemble(self, n_members, n_states, *args):
        raise _Reached(n_members, n_states, args)


def _device_stub():
    return _NoDevice()


def _members_seen(*args, **kwargs):
    with pytest.raises(_Reached) as hit:
        GP_Integrate_ensemble(*args, device=_device_stub(), **kwargs)
    return hit.value.args


# ---------------------------------------------------------------------------------------------------------
# no device: shapes and refusals
# ---------------------------------------------------------------------------------------------------------

def test_member_count_from_mixed_shapes():
    g, phis, betas, mtx = _case()
    rng = np.random.default_rng(1)
    draws0 = betas[0] * (1 + 0.05 * rng.standard_normal((7, betas[0].shape[0])))
    draws1 = betas[1] * (1 + 0.05 * rng.standard_normal((7, betas[1].shape[0])))
    y0s = np.tile(g['y0'], (7, 1))
    # 2-D betas for one state, 1-D for the other, shared y0
    n, ns, rest = _members_seen(*_golden_args(g, phis, [draws0, betas[1]], mtx, g['y0']))
    assert (n, ns) == (7, 2) and rest[3].tolist() == [1, 0]
    # both 2-D and a per-member y0
    n, ns, rest = _members_seen(*_golden_args(g, phis, [draws0, draws1], mtx, y0s))
    assert (n, ns) == (7, 2) and rest[3].tolist() == [1, 1]
    # 1-D betas shared by an initial-condition sweep
    n, ns, rest = _members_seen(*_golden_args(g, phis, betas, mtx, y0s))
    assert (n, ns) == (7, 2) and rest[3].tolist() == [0, 0]
    # everything 1-D: one member, which has no bounds
    n, ns, rest = _members_seen(*_golden_args(g, phis, betas, mtx, g['y0']), ReturnBounds=False)
    assert (n, ns) == (1, 2)
    # the cut handed down is evaluate()'s
    n, ns, rest = _members_seen(*_golden_args(g, phis, [draws0, draws1], mtx, g['y0']))
    assert rest[-2] == bounds_cut(7) == 1 and bounds_cut(1000) == 26
    # y0 is not touched (GP_Integrate advances it)
    assert np.array_equal(y0s, np.tile(g['y0'], (7, 1)))


def test_mismatched_member_counts_are_refused():
    g, phis, betas, mtx = _case()
    draws0 = np.tile(betas[0], (7, 1))
    draws1 = np.tile(betas[1], (6, 1))
    with pytest.raises(ValueError, match='disagree'):
        GP_Integrate_ensemble(*_golden_args(g, phis, [draws0, draws1], mtx, g['y0']), device=_device_stub())
    with pytest.raises(ValueError, match='disagree'):
        GP_Integrate_ensemble(*_golden_args(g, phis, [draws0, betas[1]], mtx, np.tile(g['y0'], (5, 1))),
                              device=_device_stub())
    with pytest.raises(ValueError):            # a coefficient row of the wrong length
        GP_Integrate_ensemble(*_golden_args(g, phis, [draws0[:, :-1], betas[1]], mtx, g['y0']), device=_device_stub())
    with pytest.raises(ValueError):            # y0 with three axes
        GP_Integrate_ensemble(*_golden_args(g, phis, betas, mtx, np.zeros((2, 2, 2))), device=_device_stub())


def test_bounds_need_two_members():
    g, phis, betas, mtx = _case()
    with pytest.raises(ValueError, match='at least 2 members'):
        GP_Integrate_ensemble(*_golden_args(g, phis, betas, mtx, g['y0']), device=_device_stub())
    with pytest.raises(ValueError, match='at least 2 members'):
        GP_Integrate_ensemble(*_golden_args(g, phis, [betas[0][None, :], betas[1]], mtx, g['y0']), device=_device_stub())


def test_the_errors_of_the_single_trajectory():
    g, phis, betas, mtx = _case()
    args = (g['norms'], phis, 2.0, 3.0)
    used = [row for row in g['used']]
    kw = dict(ReturnBounds=False, device=_device_stub())
    with pytest.raises(ValueError, match='cubic-spline'):
        GP_Integrate_ensemble(betas, mtx, g['b'], g['norms'], getKernels.bernoulli(), 2.0, 3.0, g['y0'], 0.05, used, **kw)
    cases = [
        (IndexError, (betas, mtx, g['b'], *args, g['y0'], 0.05, [np.array([2, 1, 3]), np.array([1, 1, 1])])),
        (IndexError, (betas, mtx, g['b'][:3], *args, g['y0'], 0.05, used)),
        (IndexError, (betas, mtx, g['b'], *args, g['y0'], 0.05, [np.array([1, 1, 0]), np.array([1, 1, 1])])),
        (ValueError, (betas[:1], mtx, g['b'], *args, g['y0'], 0.05, used)),
        (ValueError, (betas, mtx, g['b'], g['norms'].T.copy()[:1], phis, 2.0, 3.0, g['y0'], 0.05, used)),
    ]
    for exc, call in cases:
        with pytest.raises(exc) as single:
            GP_Integrate(*[a.copy() if isinstance(a, np.ndarray) else a for a in call])
        with pytest.raises(exc) as ensemble:
            GP_Integrate_ensemble(*call, **kw)
        assert str(single.value) == str(ensemble.value)


# ---------------------------------------------------------------------------------------------------------
# MI355X: every member against the host integrator
# ---------------------------------------------------------------------------------------------------------

def _host_members(betas, mtx, b, norms, phis, start, stop, y0, h, used, n_members):
    out = []
    for e in range(n_members):
        be = [np.asarray(bk)[e] if np.ndim(bk) == 2 else bk for bk in betas]
        ye = (y0[e] if np.ndim(y0) == 2 else y0).copy()
        out.append(GP_Integrate(be, mtx, b, norms, phis, start, stop, ye, h, used)[1])
    return np.array(out)


def _spread(g, betas, n_members, seed):
    """betas = golden means x (1 + 0.05 N(0, 1)) per member, y0 spread over and slightly beyond norms."""
    rng = np.random.default_rng(seed)
    draws = [bk * (1 + 0.05 * rng.standard_normal((n_members, bk.shape[0]))) for bk in betas]
    lo, hi = g['norms']
    y0 = lo - 0.05 * (hi - lo) + 1.1 * (hi - lo) * rng.random((n_members, 2))
    y0[0] = g['y0']
    if n_members >= 3:
        y0[1], y0[2] = lo, hi                  # members that start on a bound
    return draws, y0


@pytest.mark.gpu
def test_one_member_is_the_golden_trajectory(device_ctx):
    g, phis, betas, mtx = _case()
    y0 = g['y0'].copy()
    T, mean, members = GP_Integrate_ensemble(*_golden_args(g, phis, betas, mtx, y0), ReturnBounds=False,
                                             ReturnMembers=True, device=device_ctx)
    assert np.array_equal(T, g['T']) and members.shape == (1,) + g['Y'].shape
    assert np.array_equal(y0, g['y0'])                       # not advanced
    assert np.array_equal(members[0][:, 0], g['y0'])
    err = np.max(np.abs(members[0] - g['Y']))
    print(f"\nE = 1 against the reference's trajectory: max abs difference {err:.3e}")
    assert err <= 1e-13
    assert np.array_equal(mean, members[0])
    assert (g['Y'][0] >= g['norms'][1, 0]).any()             # the golden saturates: the clamps are exercised


@pytest.mark.gpu
@pytest.mark.parametrize('n_members', [2, 63, 64, 65, 1000])
def test_every_member_matches_the_host_integrator(device_ctx, n_members):
    g, phis, betas, mtx = _case()
    draws, y0 = _spread(g, betas, n_members, 100 + n_members)
    args = _golden_args(g, phis, draws, mtx, y0)
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    want = _host_members(*args, n_members)
    err = np.max(np.abs(members - want))
    print(f"\nE = {n_members}: max abs difference to the host integrator over {members.shape[2] - 1} steps {err:.3e}")
    assert err <= 1e-13
    lo, hi = g['norms']
    if n_members >= 3:
        assert (want[:, :, 0] <= lo).any() and (want[:, :, 0] >= hi).any()      # members that start saturated
    # mean and bounds are those of the returned members: the mean to rounding, the order statistics exactly
    np.testing.assert_allclose(mean, members.mean(0), rtol=0, atol=1e-14 * np.max(np.abs(members)))
    cut = bounds_cut(n_members)
    srt = np.sort(members, axis=0)
    assert np.array_equal(bounds[..., 0], srt[cut]) and np.array_equal(bounds[..., 1], srt[n_members - cut])
    # reproducible bit for bit
    again = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    for a, b in zip((mean, bounds, members), again[1:]):
        assert np.array_equal(a, b)
    # without members the same mean and bounds
    T2, mean2, bounds2 = GP_Integrate_ensemble(*args, device=device_ctx)
    assert np.array_equal(mean2, mean) and np.array_equal(bounds2, bounds)


@pytest.mark.gpu
def test_shared_betas_with_an_initial_condition_sweep(device_ctx):
    g, phis, betas, mtx = _case()
    _, y0 = _spread(g, betas, 40, 7)
    args = _golden_args(g, phis, [betas[0], np.tile(betas[1], (40, 1))], mtx, y0)
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    want = _host_members(*args, 40)
    assert np.max(np.abs(members - want)) <= 1e-13


@pytest.mark.gpu
def test_other_system_shapes(device_ctx):
    g, phis, betas, mtx = _case()
    rng = np.random.default_rng(5)
    E = 70
    # one state, no forcing (n_other = 0)
    m1, b1 = np.array([[1.0], [2.0]]), np.array([0.2, -0.4, 0.1])
    d1 = b1 * (1 + 0.1 * rng.standard_normal((E, 3)))
    args = ([d1], [m1], np.zeros((0,)), np.array([[0.0], [1.0]]), phis, 0.0, 4.0, rng.random((E, 1)), 0.1, [np.array([1])])
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    assert members.shape == (E, 1, len(T))
    assert np.max(np.abs(members - _host_members(*args, E))) <= 1e-13
    # a model that ignores the forcing next to one that uses it
    used = [np.array([1, 1, 0]), np.array([1, 1, 1])]
    mtx2 = [np.array([[1, 0], [0, 1], [2, 1]]), g['mtx1']]
    d0 = np.array([0.05, -0.3, 0.2, 0.1]) * (1 + 0.1 * rng.standard_normal((E, 4)))
    args = ([d0, betas[1]], mtx2, g['b'], g['norms'], phis, 2.0, 12.0, g['y0'], 0.05, used)
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    assert np.max(np.abs(members - _host_members(*args, E))) <= 1e-13
    # three states, models of different widths, two forcing columns, a four-factor term (it spans two term entries)
    b2 = np.stack([g['b'], 0.5 + 0.4 * np.cos(np.arange(g['b'].shape[0]) / 9.0)], axis=1)
    used = [np.array([1, 1, 1, 1, 1]), np.array([1, 0, 1, 0, 0]), np.array([0, 1, 1, 1, 1])]
    mtx3 = [np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 1], [1, 2, 1, 1, 0], [0, 0, 3, 0, 0], [0, 0, 0, 2, 0]]),
            np.array([[1, 0], [0, 1], [1, 1]]),
            np.array([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 1]])]
    means = [np.array([0.02, -0.4, 0.3, 0.5, 0.2, -0.1]), np.array([-0.03, 0.3, -0.35, 0.2]),
             np.array([0.01, -0.25, -0.3, 0.4])]
    d3 = [mk * (1 + 0.1 * rng.standard_normal((E, mk.shape[0]))) for mk in means]
    norms3 = np.array([[0.0, 0.1, -0.2], [1.0, 0.9, 0.6]])
    y03 = norms3[0] + (norms3[1] - norms3[0]) * rng.random((E, 3))
    args = (d3, mtx3, b2, norms3, phis, 0.0, 10.0, y03, 0.05, used)
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    assert members.shape == (E, 3, len(T))
    assert np.max(np.abs(members - _host_members(*args, E))) <= 1e-13
    srt = np.sort(members, axis=0)
    assert np.array_equal(bounds[..., 0], srt[bounds_cut(E)]) and np.array_equal(bounds[..., 1], srt[E - bounds_cut(E)])


@pytest.mark.gpu
def test_four_states(device_ctx):
    """integrate_ensemble_kernel<4>: models of 7, 2, 4 and 3 input columns, two forcing columns (the second used forcing
    input appends its column once more: four states + three forcing inputs), and a term of seven factors, which spans
    three term entries.  Every member against the host integrator at the file's gate."""
    g, phis, betas, mtx = _case()
    rng = np.random.default_rng(9)
    E = 70
    b2 = np.stack([g['b'], 0.5 + 0.4 * np.cos(np.arange(g['b'].shape[0]) / 9.0)], axis=1)
    used = [np.array([1, 1, 1, 1, 1, 1]), np.array([1, 0, 1, 0, 0, 0]), np.array([0, 1, 1, 1, 1, 1]), np.array([0, 0, 0, 1, 1, 0])]
    mtx4 = [np.array([[1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 1, 0, 0], [1, 2, 1, 1, 1, 2, 3], [0, 0, 3, 0, 0, 0, 0], [0, 0, 0, 2, 0, 1, 0]]),
            np.array([[1, 0], [0, 1], [1, 1]]),
            np.array([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 1]]),
            np.array([[1, 0, 0], [0, 1, 1], [2, 0, 3]])]
    means = [np.array([0.02, -0.4, 0.3, 0.5, 0.2, -0.1]), np.array([-0.03, 0.3, -0.35, 0.2]),
             np.array([0.01, -0.25, -0.3, 0.4]), np.array([0.02, -0.3, 0.25, -0.2])]
    assert all(np.abs(mk).sum() <= 2.0 for mk in means)
    d4 = [mk * (1 + 0.1 * rng.standard_normal((E, mk.shape[0]))) for mk in means]
    norms4 = np.array([[0.0, 0.1, -0.2, -1.0], [1.0, 0.9, 0.6, 1.0]])
    y04 = norms4[0] - 0.05 * (norms4[1] - norms4[0]) + 1.1 * (norms4[1] - norms4[0]) * rng.random((E, 4))
    args = (d4, mtx4, b2, norms4, phis, 0.0, 1.95, y04, 0.05, used)
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    rep = device_ctx.gp_integrate_report()
    assert rep['NS'] == 4 and rep['members'] == E and rep['workgroups'] == 2 and len(T) <= 41
    routed = [[0, 1, 2, 3, -1, -2, -2], [0, 2], [1, 2, 3, -1, -2, -2], [3, -1, -2]]     # a model's inputs: states, then forcing
    factors = {(routed[k][j], order) for k in range(4) for row in mtx4[k] for j, order in enumerate(row) if order}
    assert len(factors) == 12 and rep['lds_bytes'] == (1 + len(factors) + 4 + sum(mk.shape[0] for mk in means)) * 512
    assert members.shape == (E, 4, len(T))
    want = _host_members(*args, E)
    err = np.max(np.abs(members - want))
    print(f"\nfour states, {len(T) - 1} steps: max abs difference to the host integrator {err:.3e}")
    assert err <= 1e-13
    assert (np.abs(np.diff(want, axis=2)) > 0).any(axis=(0, 2)).all()      # every state moves
    srt = np.sort(members, axis=0)
    assert np.array_equal(bounds[..., 0], srt[bounds_cut(E)]) and np.array_equal(bounds[..., 1], srt[E - bounds_cut(E)])


def _wide_model(rows, rng, E=70):
    """One state ruled by ``rows`` terms of itself alone, orders 1 .. 3 in turn (duplicate rows), sum |beta| = 1.5."""
    mtx = (np.arange(rows) % 3 + 1)[:, None]
    mean = rng.standard_normal(rows + 1)
    mean *= 1.5 / np.abs(mean).sum()
    draws = mean * (1 + 0.1 * rng.standard_normal((E, rows + 1)))
    phis = _case()[1]
    return ([draws], [mtx], np.zeros((0,)), np.array([[0.0], [1.0]]), phis, 0.0, 1.95, rng.random((E, 1)), 0.05, [np.array([1])])


@pytest.mark.gpu
@pytest.mark.parametrize('rows', [130, 282])
def test_wide_models_opt_in_to_more_lds(device_ctx, rows):
    """LDS rows per member = 1 + factors + states + coefficients.  130 terms: 1 + 3 + 1 + 131 = 136 rows of 512 bytes, above
    the 64 KB a kernel has without asking; 282 terms: 288 rows, exactly the 144 KB budget -- the largest admitted system."""
    args = _wide_model(rows, np.random.default_rng(rows))
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    rep = device_ctx.gp_integrate_report()
    assert rep['lds_bytes'] == (1 + 3 + 1 + rows + 1) * 512 > 64 * 1024 and rep['NS'] == 1 and len(T) <= 41
    assert rows != 282 or rep['lds_bytes'] == 288 * 512 == 144 * 1024
    want = _host_members(*args, 70)
    err = np.max(np.abs(members - want))
    print(f"\n{rows} terms, {len(T) - 1} steps: max abs difference to the host integrator {err:.3e}")
    assert err <= 1e-13 and np.ptp(want[:, 0, -1]) > 0.01 and (np.abs(want[:, 0, -1] - want[:, 0, 0]) > 1e-3).any()
    srt = np.sort(members, axis=0)
    assert np.array_equal(bounds[..., 0], srt[bounds_cut(70)]) and np.array_equal(bounds[..., 1], srt[70 - bounds_cut(70)])


@pytest.mark.gpu
def test_one_term_above_the_lds_budget_is_refused(device_ctx):
    g, phis, betas, mtx = _case()
    golden = lambda: GP_Integrate_ensemble(*_golden_args(g, phis, betas, mtx, g['y0'].copy()), ReturnBounds=False,
                                           ReturnMembers=True, device=device_ctx)
    before = golden()
    with pytest.raises(_capi.FoklNativeError, match="do not fit a wavefront's LDS") as err:
        GP_Integrate_ensemble(*_wide_model(283, np.random.default_rng(283)), device=device_ctx)
    assert err.value.code == -2 and device_ctx.gp_integrate_report()['members'] == 0
    after = golden()                                          # the context still integrates, bit for bit
    assert np.max(np.abs(after[2][0] - g['Y'])) <= 1e-13
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_the_band_next_to_nan_members(device_ctx):
    """Three NaN-coefficient members among 130 (cut 4): each is NaN from its first step on, like its host trajectory; the
    bounds are np.sort's order statistics of the returned members (the three NaN sort last, so the upper bound is the
    largest finite value), the mean is the kernel's summation tree and NaN from point 1 on."""
    g, phis, betas, mtx = _case()
    E, gone = 130, (5, 64, 129)
    draws, y0 = _spread(g, betas, E, 21)
    for e, (k, c) in zip(gone, ((0, 1), (1, 2), (0, 0))):
        draws[k][e, c] = np.nan
    args = _golden_args(g, phis, draws, mtx, y0)
    T, mean, bounds, members = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    want = _host_members(*args, E)
    assert np.array_equal(np.isnan(members), np.isnan(want)) and np.isnan(members[list(gone)][:, :, 1:]).all()
    alive = np.delete(np.arange(E), gone)
    assert np.max(np.abs(members[alive] - want[alive])) <= 1e-13
    lower, upper = band_rows(members, bounds_cut(E))
    assert same_rows(bounds[..., 0], lower) and same_rows(bounds[..., 1], upper) and same_rows(mean, mean_rows(members))
    band_next_to_nan(members, mean, bounds, gone, bounds_cut(E))
    assert bounds_cut(E) == 4 and np.isfinite(bounds).all() and np.isnan(mean[:, 1:]).all()


@pytest.mark.gpu
def test_the_horizon_cut_changes_no_bit(device_ctx, monkeypatch):
    g, phis, betas, mtx = _case()
    draws, y0 = _spread(g, betas, 130, 11)
    args = _golden_args(g, phis, draws, mtx, y0)
    monkeypatch.setenv('FOKL_INTEGRATE_STEPS_PER_LAUNCH', '100000')
    whole = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
    for per_launch in ('1', '7', '64', '399'):
        monkeypatch.setenv('FOKL_INTEGRATE_STEPS_PER_LAUNCH', per_launch)
        cut_up = GP_Integrate_ensemble(*args, ReturnMembers=True, device=device_ctx)
        for a, b in zip(whole, cut_up):
            assert np.array_equal(a, b), per_launch


@pytest.mark.gpu
def test_refusals_launch_nothing(device_ctx):
    g, phis, betas, mtx = _case()
    table, nb, width = getKernels.pack_phis(phis, 0)

    def call(n_states=2, mtx0=None, n_basis=nb, w=width, n_members=4):
        import ctypes
        orders = [np.ascontiguousarray(mtx0 if mtx0 is not None else g['mtx0'], dtype=np.int32),
                  np.ascontiguousarray(g['mtx1'], dtype=np.int32)]
        coeffs = [np.ascontiguousarray(betas[0]), np.ascontiguousarray(betas[1])]
        src = [np.array([0, 1, -1], dtype=np.int32)] * 2
        k = min(n_states, 2)
        ptrs = lambda arrays: (ctypes.c_void_p * n_states)(*[_capi._ptr(arrays[i % k]) for i in range(n_states)])
        rows = np.array([orders[i % k].shape[0] for i in range(n_states)], dtype=np.int32)
        cols = np.array([3] * n_states, dtype=np.int32)
        norms = np.ascontiguousarray(np.tile(g['norms'], (1, n_states))[:, :n_states])
        return device_ctx.gp_integrate_ensemble(n_members, n_states, 1, 10, ptrs(coeffs), np.zeros(n_states, dtype=np.int32),
                                                ptrs(orders), rows, cols, ptrs(src), np.array([3] * n_states, dtype=np.int32),
                                                np.ascontiguousarray(g['b'][:10, None]), norms, table, n_basis, w, 0.05,
                                                np.full(n_states, 0.5), 1)

    mean, bounds, _ = call()                                  # the well-formed call goes through
    assert np.isfinite(mean).all() and np.isfinite(bounds).all()
    bad = g['mtx0'].copy()
    bad[0, 0] = nb + 1
    for kwargs, text in ((dict(mtx0=bad), 'outside the spline table'), (dict(w=498), '499'),
                         (dict(n_states=_capi.INTEGRATE_MAX_STATES + 1), 'at most')):
        with pytest.raises(_capi.FoklNativeError) as err:
            call(**kwargs)
        assert err.value.code == -2 and text in str(err.value)
    with pytest.raises(_capi.FoklNativeError, match='16384'):   # bounds over more members than the LDS sort holds
        call(n_members=16385)


@pytest.mark.gpu
def test_end_to_end_between_fits(device_ctx):
    """Two small cubic-spline fits on the device, set up as the golden's generator sets the system up; the posterior
    draws integrated as an ensemble; then the same backend fits again, bit for bit as before."""
    from fokl_gpy_amd import FoKLRoutines
    g, phis, _, _ = _case()
    rng = np.random.default_rng(31)
    n = 600
    states, force = rng.random((n, 2)), rng.random((n, 1))
    x = np.concatenate([states, force], axis=1)
    rhs = [0.6 * np.sin(3 * states[:, 1]) - 0.8 * states[:, 0] + 0.5 * force[:, 0],
           0.7 * states[:, 0] * (1 - states[:, 1]) - 0.3 * force[:, 0]]
    data = [rhs[k] + 0.01 * rng.standard_normal(n) for k in range(2)]

    def fit(k):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = FoKLRoutines.FoKL(kernel='Cubic Splines', phis=phis, burnin=60, draws=60, tolerance=2,
                                      UserWarnings=False, ConsoleOutput=False)
            np.random.seed(40 + k)
            betas, mtx, _ = model.fit(x, data[k], clean=True)
        return model, np.array(betas), np.array(mtx)

    fits = [fit(k) for k in range(2)]
    draws = [f[1] for f in fits]                 # fit returns the draws after burn-in: every one is a member
    E = draws[0].shape[0]
    backend = FoKLRoutines.device_backend()
    T, mean, bounds, members = GP_Integrate_ensemble(draws, [f[2] for f in fits], g['b'], g['norms'], phis, 2.0, 12.0,
                                                     g['y0'], 0.05, [np.array([1, 1, 1])] * 2, ReturnMembers=True,
                                                     device=backend)
    assert members.shape == (E, 2, len(T)) and np.isfinite(members).all()
    spread = members.max(0) - members.min(0)
    live = spread > 0
    assert live.any()
    assert (bounds[..., 0] <= mean)[live].all() and (mean <= bounds[..., 1])[live].all()
    assert (bounds[..., 0] <= bounds[..., 1]).all()
    # the context still fits and evaluates, with unchanged results
    model, betas_again, mtx_again = fit(0)
    assert np.array_equal(mtx_again, fits[0][2]) and np.array_equal(betas_again, fits[0][1])
    assert np.isfinite(model.evaluate(x)).all()

"""ensemble_band_kernel and ensemble_transpose_kernel (csrc/fokl_integrate_device.inc) on designed rows, on the MI355X.

Point 0 of every run is y0 bit for bit, and the raw DeviceContext.gp_integrate_ensemble takes a per-member y0 and any cut
in 1 .. members - 1: a one-input model per state and 0 to 2 steps hand the band any row one designs.  Every case compares
the bounds with np.sort's order statistics of the RETURNED members (band_reference.band_rows: NaN after +inf), the mean with
the kernel's summation tree restated in numpy (band_reference.mean_rows), both bit for bit, and point 0 of the members
with y0 bit for bit.  The member counts sit on both sides of every path of the kernel: the 256-thread stride, the powers
of two, the switch from 4 workgroups per CU to 1 above 32 KB of list (4 097 members), the LDS opt-in above 64 KB (8 193)
and the largest list (16 384); fokl_gp_integrate_report says which path ran."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN
from band_reference import EDGE_ROWS, FINITE_ROWS, band_rows, designed_row, mean_rows, same_rows
from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd.GP_Integrate import bounds_cut

pytestmark = pytest.mark.gpu

PHIS = getKernels.table_to_phis(np.load(os.path.join(GOLDEN, 'spline_phis.npz'))['table'])
COUNTS = (2, 3, 70, 255, 256, 257, 1024, 1025, 4096, 4097, 8192, 8193, 16383, 16384)


def _cuts(E):
    return sorted({1, bounds_cut(E), E - 1} & set(range(1, E)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run(ctx, y0, n_steps, cut, want_members=True, scale=1.0, h=0.05):
    """K = y0.shape[1] states, state k ruled by a two-term cubic-spline model of itself alone (no forcing), range [0, 1],
    coefficients shared by the members -> (mean [K, P], bounds [K, P, 2] or None, members [E, K, P] or None)."""
    y0 = np.ascontiguousarray(y0, dtype=np.float64)
    E, K = y0.shape
    table, n_basis, width = getKernels.pack_phis(PHIS, 0)
    betas = [np.ascontiguousarray(scale * np.array([0.2, -0.4, 0.1]) * (1.0 + 0.25 * k)) for k in range(K)]
    orders = [np.array([[1], [2]], dtype=np.int32) for _ in range(K)]
    sources = [np.array([k], dtype=np.int32) for k in range(K)]
    ptrs = lambda arrays: (ctypes.c_void_p * K)(*[_capi._ptr(a) for a in arrays])
    ones, norms = np.ones(K, dtype=np.int32), np.ascontiguousarray(np.stack([np.zeros(K), np.ones(K)]))
    return ctx.gp_integrate_ensemble(E, K, 0, n_steps, ptrs(betas), np.zeros(K, dtype=np.int32), ptrs(orders), 2 * ones, ones,
                                     ptrs(sources), ones, None, norms, table, n_basis, width, h, y0, cut, want_members)


def _check(ctx, y0, n_steps, cut, scale=1.0, h=0.05, tag=''):
    """One call with bounds and members against the statement -> (mean, bounds, members, report)."""
    mean, bounds, members = _run(ctx, y0, n_steps, cut, scale=scale, h=h)
    rep = ctx.gp_integrate_report()
    E, K = y0.shape
    assert members.shape == (E, K, n_steps + 1) and mean.shape == (K, n_steps + 1) and bounds.shape == (K, n_steps + 1, 2)
    assert np.array_equal(_bits(members[:, :, 0]), _bits(y0)), f"{tag}: point 0 of the members is not y0"
    lo, hi = band_rows(members, cut)
    want_mean = mean_rows(members)
    for name, got, want in (('lower', bounds[..., 0], lo), ('upper', bounds[..., 1], hi), ('mean', mean, want_mean)):
        if not same_rows(got, want):
            at = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
            k, q = at[0]
            print(f"\n{tag}: {name} differs in {len(at)} of {got.size} rows, first at state {k} point {q}: device "
                  f"{got[k, q]!r}, statement {want[k, q]!r}")
        assert same_rows(got, want), (tag, name)
    npow2 = 2
    while npow2 < E:
        npow2 *= 2
    per_cu = 1 if npow2 * 8 > 32 * 1024 else 4
    assert rep['members'] == E and rep['NS'] == K and rep['band_lds_bytes'] == npow2 * 8 and rep['compute_units'] > 0
    assert rep['band_workgroups'] == min(rep['band_rows'], rep['compute_units'] * per_cu)
    return mean, bounds, members, rep


# ---------------------------------------------------------------------------------------------------------
# 1. every member count, every cut, every kind of row
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', COUNTS)
def test_designed_rows_at_every_member_count(device_ctx, E):
    rng = np.random.default_rng(E)
    for cut in _cuts(E):
        for i, kind in enumerate(FINITE_ROWS + EDGE_ROWS):
            row = designed_row(kind, E, cut, rng)
            mean, bounds, members, rep = _check(device_ctx, row[:, None], (i + cut) % 3, cut, tag=f"E {E} cut {cut} {kind}")
            if kind == 'permutation':                                # integers: the mean of point 0 is exact
                assert mean[0, 0] == row.sum() / E
            if kind == 'all_nan':
                assert np.isnan(mean).all() and np.isnan(bounds).all()
            if kind == 'nan_cut':                                    # the upper bound turns NaN once `cut` members are NaN
                assert np.isnan(bounds[0, 0, 1]) and np.isnan(mean[0, 0]) and (E - cut <= cut or np.isfinite(bounds[0, 0, 0]))
            if kind == 'nan_cut_minus_1' and cut > 1:
                assert bounds[0, 0, 1] == np.nanmax(row)
            if i == 0:                                               # without the members the same mean and bounds
                mean2, bounds2, none = _run(device_ctx, row[:, None], (i + cut) % 3, cut, want_members=False)
                assert none is None and same_rows(mean2, mean) and same_rows(bounds2, bounds)
    assert (rep['band_lds_bytes'] > 64 * 1024) == (E > 8192) and rep['band_lds_bytes'] <= 128 * 1024


def test_the_smallest_plain_case(device_ctx):
    """Members 0, NaN, 2, 3, ..., 69 with cut 2: np.sort gives (3, 69).  Under a plain ``>`` the network gave (2, 68)."""
    row = np.array([0.0, np.nan, 2.0] + [float(v) for v in range(3, 70)])
    mean, bounds, members, _ = _check(device_ctx, row[:, None], 0, 2, tag='0, NaN, 2 .. 69')
    print(f"\nbounds of 0, NaN, 2 .. 69 at cut 2: {bounds[0, 0].tolist()}")
    assert bounds[0, 0].tolist() == [3.0, 69.0] and np.isnan(mean[0, 0])


# ---------------------------------------------------------------------------------------------------------
# 2. more (state, point) rows than workgroups: the loop round the grid
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_nan', [False, True])
@pytest.mark.parametrize('shape', ['four_states_small_list', 'one_state_long_list'])
def test_a_workgroup_goes_round_the_grid(device_ctx, monkeypatch, shape, with_nan):
    """4 states x (2 CUs + 1) points at 64 members is more than twice the 4 workgroups per CU of a small list; 1 state x
    (CUs + 44) points at 4 097 members is more than the 1 per CU of a list above 32 KB.  The output buffers are not
    cleared between calls: every case has values and coefficients of its own, so a row left unwritten shows."""
    monkeypatch.setenv('FOKL_INTEGRATE_STEPS_PER_LAUNCH', '100000')
    _run(device_ctx, np.full((2, 1), 0.5), 0, 1)
    cus = device_ctx.gp_integrate_report()['compute_units']
    K, E, points = (4, 64, 2 * cus + 1) if shape == 'four_states_small_list' else (1, 4097, cus + 44)
    seed = 10 * (shape == 'one_state_long_list') + with_nan
    rng = np.random.default_rng(500 + seed)
    y0 = rng.uniform(-0.2, 1.2, (E, K))
    if with_nan:
        gone = rng.choice(E, size=bounds_cut(E) + 1, replace=False)
        y0[gone[1:], 0] = np.nan                                     # `cut` NaN: the upper bound of state 0 is NaN throughout
        y0[gone[0], K - 1] = np.inf
    # a step of 0.001: no member comes to rest within the run
    mean, bounds, members, rep = _check(device_ctx, y0, points - 1, bounds_cut(E), scale=1.0 + 0.01 * seed, h=0.001, tag=shape)
    assert rep['launches'] == 1 and rep['band_rows'] == K * points and rep['band_workgroups'] < rep['band_rows']
    assert rep['band_workgroups'] == cus * (4 if E == 64 else 1)
    finite = members[np.isfinite(members[:, 0, 0])][:, 0]
    assert (np.abs(np.diff(finite, axis=1)) > 0).any(axis=0).all()   # the members move at every step: no row repeats another
    if with_nan:
        assert np.isnan(bounds[0, :, 1]).all() and np.isfinite(bounds[0, :, 0]).all() and np.isnan(mean[0]).all()


# ---------------------------------------------------------------------------------------------------------
# 3. the transpose: members and points on both sides of a 32 x 32 tile, one point per launch
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [31, 32, 33])
def test_transpose_tiles(device_ctx, monkeypatch, E):
    rng = np.random.default_rng(40 + E)
    y0 = rng.uniform(-0.2, 1.2, (E, 3))
    y0[E // 2, 1] = np.nan
    monkeypatch.setenv('FOKL_INTEGRATE_STEPS_PER_LAUNCH', '100000')
    whole = {}
    for steps in (30, 31, 32, 33):                                   # 31 .. 34 points
        whole[steps] = _check(device_ctx, y0, steps, bounds_cut(E), tag=f"E {E} steps {steps}")[:3]
        assert same_rows(whole[steps][2][:, :, :31], whole[30][2])   # a longer run starts as the shorter one
    monkeypatch.setenv('FOKL_INTEGRATE_STEPS_PER_LAUNCH', '1')       # 1 or 2 points per transpose, a strided copy per launch
    cut_up = _check(device_ctx, y0, 33, bounds_cut(E), tag=f"E {E} one step per launch")
    assert cut_up[3]['launches'] == 33 and cut_up[3]['steps_per_launch'] == 1 and cut_up[3]['band_rows'] == 6
    for a, b in zip(whole[33], cut_up[:3]):
        assert same_rows(a, b)


# ---------------------------------------------------------------------------------------------------------
# 4. mean only: no list, no limit on the members
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [16385, 70000])
def test_mean_only_has_no_member_limit_and_no_list(device_ctx, E):
    rng = np.random.default_rng(E)
    row = designed_row('permutation', E, 1, rng)
    for nan_at in (None, E - 1):
        if nan_at is not None:
            row[nan_at] = np.nan
        mean, bounds, members = _run(device_ctx, row[:, None], 2, None)
        rep = device_ctx.gp_integrate_report()
        assert bounds is None and rep['band_lds_bytes'] == 0 and rep['members'] == E and rep['workgroups'] == -(-E // 64)
        assert np.array_equal(_bits(members[:, :, 0]), _bits(row[:, None]))
        assert same_rows(mean, mean_rows(members))
        assert np.isnan(mean).all() if nan_at is not None else mean[0, 0] == row.sum() / E
    with pytest.raises(_capi.FoklNativeError, match='16384'):       # the bounds over as many stay refused ...
        _run(device_ctx, row[:, None], 2, 1)
    assert device_ctx.gp_integrate_report()['members'] == 0         # ... and a refused call reports nothing

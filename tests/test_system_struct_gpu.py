"""The seven entry points that take a fokl_system (include/fokl_hip_internal.h) at what they share on the host side: the
chunk loop of the three simulate calls with one step per launch at the member padding (E = 1, 64, 65), and the refusal of
a null struct."""
import ctypes

import numpy as np
import pytest

from fokl_gpy_amd import _capi, dynamics
from test_simulate_adaptive_gpu import RECORD as ADAPTIVE_RECORD, _system
from test_simulate_stiff_gpu import RECORD as STIFF_RECORD

pytestmark = pytest.mark.gpu

STEPS = 3
# the call, its host statement, the environment variable that bounds a launch, its report, its per-member record, keep
CALLS = dict(
    simulate=(dynamics.simulate, dynamics.simulate_host, 'FOKL_SIMULATE_STEPS_PER_LAUNCH', 'simulate_report',
              ('first_saturation',), 'members'),
    simulate_adaptive=(dynamics.simulate_adaptive, dynamics.simulate_adaptive_host, 'FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH',
                       'simulate_adaptive_report', ADAPTIVE_RECORD, ('members', 'levels')),
    simulate_stiff=(dynamics.simulate_stiff, dynamics.simulate_stiff_host, 'FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH',
                    'simulate_stiff_report', STIFF_RECORD, ('members', 'levels')))


def band_mean(members):
    """ensemble_band_kernel's mean of members [E <= 256, ...] as fokl_integrate_device.inc states it: thread i of 256 holds
    member i (the others 0.0), the partial sums are added by the halving tree.  The host statements form their mean in
    numpy's order, which rounds differently; this is the order the device documents, applied to the host's members."""
    E = members.shape[0]
    partial = np.zeros((256,) + members.shape[1:])
    partial[:E] = members
    half = 128
    while half:
        partial[:half] = partial[:half] + partial[half:2 * half]
        half //= 2
    return partial[0] / E


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    return a == b


@pytest.mark.parametrize('E', [1, 64, 65])
@pytest.mark.parametrize('name', list(CALLS))
def test_one_step_per_launch_at_the_member_padding(device_ctx, monkeypatch, name, E):
    """Every launch holds one step, so the band, the transpose and the strided member copy run once per point, and E = 1,
    64, 65 puts the member padding at none, a full wavefront and one member past it.  Every returned field equals the host
    statement's bit for bit (the mean: the band kernel's summation tree over the host's members); bounds are requested
    wherever there are any (one member has none: the plan refuses them)."""
    run, host_run, env, report, record, keep = CALLS[name]
    # seed 301: with 64 and 65 members the adaptive calls refine to their deepest level, the last member included
    args = _system(301, 2, 'b', E, steps=STEPS, n_forcing=1, stiffness=2.0, spread=8.0)
    monkeypatch.setenv(env, '1')
    host = host_run(**args, ReturnBounds=E > 1, keep=keep)
    dev = run(**args, ReturnBounds=E > 1, keep=keep, device=device_ctx)
    rep = getattr(device_ctx, report)()
    assert rep['launches'] == STEPS and rep['steps_per_launch'] == 1 and rep['workgroups'] == -(-E // 64) and rep['members'] == E
    assert np.isfinite(host['members']).all() and host['members'].shape == (E, 2, STEPS + 1)
    assert sorted(dev) == sorted(host) and ('bounds' in dev) == (E > 1) and all(key in dev for key in record + ('members',))
    for key in host:
        want = band_mean(host['members']) if key == 'mean' else host[key]
        assert same(dev[key], want), (key, dev[key], want)
    if E == 65:                                                      # the member past the full wavefront is that draw run alone
        alone = run(**{**args, 'y0': args['y0'][64]}, draws=np.array([64]), ReturnBounds=False, keep=keep, device=device_ctx)
        assert getattr(device_ctx, report)()['launches'] == STEPS
        for key in record + ('members',):
            assert same(alone[key][0], dev[key][64]), key


# ---------------------------------------------------------------------------------------------------------
# a null fokl_system / fokl_control_problem
# ---------------------------------------------------------------------------------------------------------

REPORTS = dict(fokl_simulate_ensemble=('fokl_simulate_report', 8), fokl_simulate_adaptive=('fokl_simulate_adaptive_report', 12),
               fokl_simulate_stiff=('fokl_simulate_stiff_report', 11), fokl_assimilate_ensemble=('fokl_assimilate_report', 9),
               fokl_control_solve=('fokl_control_report', 8), fokl_control_pooled_solve=('fokl_control_pooled_report', 15),
               fokl_control_cvar_solve=('fokl_control_cvar_report', 18))
NULL_CASES = [(name, 'system') for name in REPORTS] + [(name, 'problem') for name in REPORTS if 'control' in name]


@pytest.mark.parametrize('name,null', NULL_CASES)
def test_a_null_struct_is_refused(device_ctx, name, null):
    lib = _capi.load()
    args = _system(400, 2, 'b', 3, steps=STEPS, n_forcing=1)
    p = dynamics._prepare(args['models'], args['states'], args['inputs'], args['forcing'], args['y0'], args['t'], None, None, True,
                          'members')
    system, held = _capi._system_struct(p, 'test', coef_by_draw=name not in ('fokl_simulate_ensemble', 'fokl_simulate_adaptive',
                                                                             'fokl_simulate_stiff'))
    # every other argument is usable: pointers into a zeroed scratch buffer, sizes of 1, scales of 0.5; no first_trial
    scratch = np.zeros(4096, dtype=np.float64)
    kinds = _capi.SIGNATURES[name][1]
    call = [scratch.ctypes.data if kind is ctypes.c_void_p else 0.5 if kind is ctypes.c_double else 1 for kind in kinds]
    call[0] = device_ctx._h
    call[1] = None if null == 'system' else ctypes.addressof(system)
    if 'control' in name:
        problem = _capi._ControlProblemStruct(n_controls=1, n_segments=1, n_starts=1, **{
            field: scratch.ctypes.data for field, kind in _capi._ControlProblemStruct._fields_ if kind is ctypes.c_void_p})
        call[2] = None if null == 'problem' else ctypes.addressof(problem)
        if name != 'fokl_control_solve':
            call[-1] = None
    report, length = REPORTS[name]
    seen = np.ones(length, dtype=np.int64)
    assert getattr(lib, name)(*call) == -2                           # FOKL_ERR_ARG
    assert lib.fokl_last_error(device_ctx._h).decode() == f"{name}: null pointer, negative size or empty system"
    assert getattr(lib, report)(device_ctx._h, seen.ctypes.data) == 0 and not seen.any()
    del held
    # the context is as good as before
    host = dynamics.simulate_host(**args, keep='members')
    dev = dynamics.simulate(**args, keep='members', device=device_ctx)
    assert np.array_equal(dev.members, host.members) and device_ctx.simulate_report()['members'] == 3

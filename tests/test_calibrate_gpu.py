"""fokl_calibrate_ensemble (csrc/fokl_calibrate_device.inc) against dynamics.calibrate_host, the statement of the calibration of
a fitted dynamic system: every kept lp recomputed from the device's own positions bit for bit, the replayed trajectories,
whole chains by their accept flags, the bitwise invariances counter-based numbers give, and every native refusal -- at the
smallest shapes at which the kernel can go wrong (tests/test_calibrate_host.py: case_a, case_b, case_c)."""
import numpy as np
import pytest

from test_calibrate_host import W, case_a, case_b, case_c, lp_from_simulate_host, rows_of
from test_infer_gpu import follows
from fokl_gpy_amd import _capi, dynamics

pytestmark = pytest.mark.gpu

CASES = {'A': case_a, 'B': case_b, 'C': case_c}
LDS_BYTES = {'A': (1 + 2 + 1 + 7 * 1) * 512 + 3 * 8, 'B': (1 + 11 + 4 + 7 * 2) * 512 + 12 * 8, 'C': (1 + 32 + 16 + 7 * 16) * 512 + 40 * 8}
NS = {'A': 1, 'B': 2, 'C': 8}


# ---------------------------------------------------------------------------------------------------------
# 1., 2. lp bit for bit from the device's own positions; the replay of the final ensemble
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('jump_every', [0, 1])
@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_kept_lp_and_replay_are_the_host_statements_bit_for_bit(device_ctx, name, jump_every):
    """No comparison of two chains: whatever the device accepted, the lp and the saturation flag it kept at a position are
    the host statement's at that position, and the trajectories it replays are ``simulate_host``'s members."""
    args = dict(CASES[name](), burnin=0, draws_kept=6, thin=1, jump_every=jump_every, seed=3, keep=['x', 'trajectories'])
    dev = dynamics.calibrate(**args, device=device_ctx)
    rep = device_ctx.calibrate_report()
    p = dynamics._prepare_calibrate(**args)
    E, d = p['E'], p['d']
    assert rep['NS'] == NS[name] and rep['draws'] == E and rep['lds_bytes'] == LDS_BYTES[name] == p['lds_bytes']
    assert rep['launches'] == 2 and rep['iterations'] == 6 and rep['evaluations'] == int(dev.evals.sum())
    assert rep['kernel_us'] > 0
    assert dev.x.shape == (E * 6 * W, d) and not dev.invalid.any()
    assert np.all((dev.x > p['lo']) & (dev.x < p['hi']))
    with np.errstate(all='ignore'):
        lp, sat = dynamics.calibrate_target(p, dev.x.reshape(E, 6 * W, d))
    assert np.array_equal(dev.lp, lp.reshape(-1)) and np.array_equal(dev.saturated, sat.reshape(-1))
    moved = rows_of(dev)[:, -1] != p['starts']
    print(f"\ncase {name}, jump_every {jump_every}: {dev.lp.size} kept lp equal the host's bit for bit; "
          f"{int(dev.saturated.sum())} saturated, {int(moved.any(axis=-1).sum())} of {E * W} walkers moved")
    assert jump_every == 1 or moved.any(axis=-1).sum() > E * W // 2    # (a jump in 16 dimensions is seldom accepted)
    # ... and through simulate_host itself, a handful of rows: the first, the last, one of every draw and half
    x = rows_of(dev)
    for e, r, w in [(0, 0, 0), (E - 1, 5, W - 1), (0, 3, 64), (E - 1, 2, 63)]:
        want, want_sat, y = lp_from_simulate_host(args, p, x[e, r, w], e)
        assert dev.lp.reshape(E, 6, W)[e, r, w] == want and dev.saturated.reshape(E, 6, W)[e, r, w] == want_sat
        if r == 5:
            assert np.array_equal(dev.trajectories[e, w], y)
    # the replay: the final ensemble is the last kept row
    with np.errstate(all='ignore'):
        points = dynamics.calibrate_target(p, x[:, -1], trajectories=True)[2]
    assert dev.trajectories.shape == points.shape and np.array_equal(dev.trajectories, points)


# ---------------------------------------------------------------------------------------------------------
# 3. whole chains
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('jump_every', [2, 0])
def test_chains_follow_the_host_statement(device_ctx, jump_every):
    args = dict(case_b(), burnin=0, draws_kept=40, thin=1, jump_every=jump_every, seed=1)
    dev, host = dynamics.calibrate(**args, device=device_ctx), dynamics.calibrate_host(**args)
    p = dynamics._prepare_calibrate(**args)
    E = p['E']
    width = p['hi'] - p['lo']
    same = follows(rows_of(dev) / width, rows_of(host) / width, p['starts'] / width, E - 1)
    lp_dev, lp_host = dev.lp.reshape(E, 40, W)[same], host.lp.reshape(E, 40, W)[same]
    assert np.max(np.abs(lp_dev - lp_host) / np.abs(lp_host)) <= 1e-9
    assert np.array_equal(dev.accept[same], host.accept[same], equal_nan=True) and np.array_equal(dev.evals[same], host.evals[same])
    assert np.array_equal(dev.saturated.reshape(E, 40, W)[same], host.saturated.reshape(E, 40, W)[same])
    assert np.allclose(dev.rhat[same], host.rhat[same], rtol=1e-9) and not dev.invalid.any()
    assert dev.evals.min() > W and dev.accept[:, 0].min() > 0.1
    if jump_every == 0:                                                # no transcendental enters a stretch proposal
        assert np.array_equal(rows_of(dev)[same], rows_of(host)[same]) and np.array_equal(lp_dev, lp_host)
        assert np.isnan(dev.accept[:, 1]).all()
    else:
        assert dev.accept[:, 1].min() > 0.0


# ---------------------------------------------------------------------------------------------------------
# 4. invariances, bit for bit
# ---------------------------------------------------------------------------------------------------------

PER_DRAW = ('x', 'lp', 'saturated', 'draw')


def test_invariances_bit_for_bit(device_ctx, monkeypatch):
    monkeypatch.delenv('FOKL_CALIBRATE_STEPS_PER_LAUNCH', raising=False)
    args = dict(case_b(), burnin=3, draws_kept=9, thin=1, jump_every=3, seed=5, keep=['x', 'trajectories'])
    whole = dynamics.calibrate(**args, device=device_ctx)
    rep = device_ctx.calibrate_report()
    assert rep['launches'] == 2 and rep['iterations_per_launch'] == 65536 // 60 and rep['iterations'] == 12
    again = dynamics.calibrate(**args, device=device_ctx)
    for key in PER_DRAW + ('trajectories', 'rhat', 'accept', 'evals', 'mean', 'fit_bounds'):
        assert np.array_equal(again[key], whole[key], equal_nan=True), key
    alone = dynamics.calibrate(**args, draws=np.array([4]), device=device_ctx)
    pick = whole.draw == 4
    for key in PER_DRAW:
        assert np.array_equal(alone[key], whole[key][pick]), key
    assert np.array_equal(alone.trajectories[0], whole.trajectories[4]) and np.array_equal(alone.rhat, whole.rhat[4:5])
    assert np.array_equal(alone.evals, whole.evals[4:5]) and np.array_equal(alone.accept, whole.accept[4:5])
    thinned = dynamics.calibrate(**dict(args, thin=3), device=device_ctx)
    assert np.array_equal(rows_of(thinned), rows_of(whole)[:, ::3])
    assert np.array_equal(thinned.lp.reshape(6, 3, W), whole.lp.reshape(6, 9, W)[:, ::3])
    assert np.array_equal(thinned.rhat, whole.rhat) and np.array_equal(thinned.trajectories, whole.trajectories)
    monkeypatch.setenv('FOKL_CALIBRATE_STEPS_PER_LAUNCH', '1')          # a launch holds one iteration
    cut_up = dynamics.calibrate(**args, device=device_ctx)
    rep = device_ctx.calibrate_report()
    assert rep['launches'] == 13 and rep['iterations_per_launch'] == 1
    for key in PER_DRAW + ('trajectories', 'rhat', 'accept', 'evals', 'mean', 'invalid'):
        assert np.array_equal(cut_up[key], whole[key]), key
    monkeypatch.setenv('FOKL_CALIBRATE_STEPS_PER_LAUNCH', '300')        # 5 iterations: the cut falls inside both halves of the sums
    cut_up = dynamics.calibrate(**args, device=device_ctx)
    assert device_ctx.calibrate_report()['launches'] == 4
    for key in PER_DRAW + ('trajectories', 'rhat', 'accept', 'evals'):
        assert np.array_equal(cut_up[key], whole[key]), key
    monkeypatch.delenv('FOKL_CALIBRATE_STEPS_PER_LAUNCH')
    bare = dynamics.calibrate(**dict(args, keep=None), device=device_ctx)
    assert bare.x is None and 'trajectories' not in bare and device_ctx.calibrate_report()['launches'] == 1
    assert np.array_equal(bare.rhat, whole.rhat) and np.array_equal(bare.accept, whole.accept)
    # the host statement's sums are the device's wherever the chains are the same: all of these short ones or all but one
    host = dynamics.calibrate_host(**args)
    same = [e for e in range(6) if np.array_equal(rows_of(host)[e], rows_of(whole)[e])]
    assert len(same) >= 5 and np.array_equal(host.rhat[same], whole.rhat[same])


def test_a_nan_coefficient_invalidates_its_draw_only(device_ctx):
    args = dict(case_b(), burnin=0, draws_kept=4, thin=1, jump_every=2, seed=5)
    clean = dynamics.calibrate(**args, device=device_ctx)
    args['models'][1] = dict(args['models'][1], betas=args['models'][1]['betas'].copy())
    args['models'][1]['betas'][2, 1] = np.nan
    res = dynamics.calibrate(**args, device=device_ctx)
    assert res.invalid.tolist() == [False, False, True, False, False, False]
    rest = clean.draw != 2
    assert np.array_equal(res.x[rest], clean.x[rest]) and np.array_equal(res.lp[rest], clean.lp[rest])
    assert np.isnan(res.lp[~rest]).all()
    starts = dynamics._prepare_calibrate(**args)['starts']
    assert np.array_equal(rows_of(res)[2], np.broadcast_to(starts, (4, W, 2)))


# ---------------------------------------------------------------------------------------------------------
# 5. the native refusals
# ---------------------------------------------------------------------------------------------------------

def test_native_refusals_launch_nothing(device_ctx, monkeypatch):
    monkeypatch.delenv('FOKL_CALIBRATE_FREE_BYTES', raising=False)
    good = dynamics._prepare_calibrate(**case_b(), burnin=1, draws_kept=2, thin=1)
    device_ctx.calibrate(good)
    assert device_ctx.calibrate_report()['launches'] == 1

    def refused(match, **changes):
        with pytest.raises(_capi.FoklNativeError, match=match) as hit:
            device_ctx.calibrate({**good, **changes})
        assert hit.value.code == -2
        assert set(device_ctx.calibrate_report().values()) == {0}

    E, steps = good['E'], good['n_steps']
    # of a system and of observations, as fokl_assimilate_ensemble
    refused('h must be positive', h=0.0)
    refused('a state\'s box is empty', box=np.array([[0.5, 2.0], [1.0, 1.0]]))
    refused('a factor reads outside', fac_norm=np.full_like(good['fac_norm'], 99))
    refused('an observed column reads outside the states', obs_state=np.array([2], dtype=np.int32))
    refused('obs_hp = 0.5 / obs_sd\\^2 must be positive and finite', obs_hp=np.array([0.0]))
    bad_row = good['obs_row'].copy()
    bad_row[5] = 3
    refused('the observation table must hold the rows 0, 1, ...', obs_row=bad_row)
    refused('the observation table holds 6 rows, data 5', data=good['data'][:5])
    refused('data holds an infinite value', data=np.where(np.isnan(good['data']), np.inf, good['data']))
    refused('y0 is not finite', y0=np.full_like(good['y0'], np.nan))
    # of the unknowns
    none = np.zeros(0)
    refused('0 unknowns, the kernel is built for 1 to 16', d=0, unknown_src=np.zeros(0, dtype=np.int32), lo=none, hi=none,
            prior_mean=none, prior_prec=none, starts=np.zeros((W, 0)))
    refused('unknown 0 lies outside the 2 states and the 2 forcing columns', unknown_src=np.array([2, -1], dtype=np.int32))
    refused('unknown 1 lies outside the 2 states and the 2 forcing columns', unknown_src=np.array([1, -3], dtype=np.int32))
    refused('an unknown is named twice', unknown_src=np.array([1, 1], dtype=np.int32))
    refused('no model reads the parameter that is unknown 1', unknown_src=np.array([1, -3], dtype=np.int32),
            forcing=np.concatenate([good['forcing'], np.zeros((steps, 1))], axis=1))
    refused('norm_param\\[0\\] = -1 but the unknowns\' columns say 1', norm_param=np.full_like(good['norm_param'], -1))
    refused('its box is empty or not finite', hi=good['lo'].copy())
    refused('its box is empty or not finite', hi=np.array([np.inf, 10.0]))
    inside = good['starts'].copy()
    inside[70, 1] = good['hi'][1]
    refused('start 70 is not strictly inside the box at unknown 1', starts=inside)
    refused('a negative precision is refused', prior_prec=np.array([0.0, -1.0]))
    refused('the prior of unknown 0 needs a finite mean', prior_mean=np.array([np.nan, 0.0]))
    for key, value in (('thin', 0), ('draws_kept', 0), ('burnin', -1), ('jump_every', -1), ('burnin', (1 << 30) + 1)):
        refused('thin >= 1, 1 <= draws_kept <= 2\\^30, 0 <= burnin <= 2\\^30 and jump_every >= 0 are needed', **{key: value})
    # the LDS budget and the device's memory
    many = np.zeros((18200, E))
    many[:12] = good['coef']
    refused('the problem needs 160960 bytes of LDS \\(\\(1 \\+ 11 factors \\+ 4 normalised states \\+ 7 x 2 unknowns\\) x 64 x 8 \\+ '
            '18200 coefficients x 8\\), a wavefront has 147456', coef=many)
    monkeypatch.setenv('FOKL_CALIBRATE_FREE_BYTES', str(64 << 20))
    refused('bytes on the device and 64 MiB to spare .* the device has 67108864 free')
    monkeypatch.delenv('FOKL_CALIBRATE_FREE_BYTES')
    # and the context still works
    out = device_ctx.calibrate(good)
    assert device_ctx.calibrate_report()['launches'] == 1 and np.isfinite(out[1]).all()

"""acquire.acquire_system on the device against from-scratch arithmetic on the host.

Two small fitted Bernoulli models (test_acquire_system_host.models_case: 60 training rows, 40 pool rows, 30 draws, the
constraint model reads one of the objective's two inputs through another minmax).  The device is followed along its OWN
picks: at every pick the host forms f and the feasibility from ``basis_matrix`` per model, updates the incumbent with the
device's earlier picks and recomputes every row's criterion from scratch; the device's gain must match the host's value at
the device's index within 1e-9 relative (the bound tests/test_acquire_gpu.py uses for the same arithmetic) and be within
that bound of the host's maximum, so a near-tie decided differently by the order of a sum is not a failure.
"""
import numpy as np
import pytest

from test_acquire_system_host import LIMIT, XVARS, YVARS, models_case, scratch
from fokl_gpy_amd import acquire as aq
from fokl_gpy_amd import engine

pytestmark = pytest.mark.gpu

GATE = 1e-9


def follow_the_device(models, pool, res, criterion, sense):
    sign = 1.0 if sense == 'max' else -1.0
    F, ok = scratch(models, pool, sign)
    b = sign * res.incumbent
    for k in range(res.picks):
        crit = aq.gain_rows_system(F, ok, b, criterion)
        crit[res.index[:k]] = -np.inf
        i = int(res.index[k])
        assert crit[i] >= crit.max() * (1.0 - GATE), k
        assert abs(res.gain[k] - crit[i]) <= GATE * abs(crit[i]), k
        b = np.where(ok[i] & (F[i] > b), F[i] if criterion == 'ei' else np.inf, b)
    assert np.allclose(sign * res.incumbent_after, b, rtol=1e-12, atol=0.0)
    assert np.array_equal(res.joint, np.cumsum(res.gain)) and len(set(res.index.tolist())) == res.picks
    assert np.array_equal(res.feasible_draws, ok[res.index].sum(axis=1))
    assert np.array_equal(res.p_feasible, res.feasible_draws / res.draws)
    return F, ok


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('sense', aq.SENSES)
def test_pick_loop_along_the_devices_own_path(device_ctx, sense, criterion):
    models, pool, measured = models_case(3)                      # two draws have no feasible measured row
    backend = engine.HipBackend(device_ctx)
    sign = 1.0 if sense == 'max' else -1.0
    res = aq.acquire_system(models, XVARS, YVARS, 'yield', pool, constraints=LIMIT, picks=6, criterion=criterion, sense=sense,
                            keep='first', no_feasible=0.3, device=backend)
    assert res.gain[0] > 0.0 and res.draws == 30 and res.rows == 40 and res.row_tiles == 3
    assert np.array_equal(res.x, pool[res.index])                # the rows as passed, in true scale
    Fm, okm = scratch(models, measured, sign)
    assert 0 < (~okm.any(axis=0)).sum() < 30
    assert np.array_equal(res.measured_feasible, okm.sum(axis=0)) and res.measured_feasible.dtype == np.int64
    best = np.where(okm.any(axis=0), sign * np.where(okm, Fm, -np.inf).max(axis=0), 0.3)
    assert np.allclose(res.incumbent, best, rtol=1e-12, atol=0.0)
    F, ok = follow_the_device(models, pool, res, criterion, sense)
    first = aq.gain_rows_system(F, ok, sign * res.incumbent, criterion)
    assert res.first.shape == (40,) and np.max(np.abs(res.first - first)) <= 1e-12 * np.abs(F).max()
    assert res.first[res.index[0]] == res.gain[0] == res.first.max()
    rep = device_ctx.acquire_system_report()
    assert rep['instance'] == criterion and rep['lazy'] and rep['constraints'] == 1 and rep['picks'] == 6
    assert rep['lds_bytes'] == 8 * 16 * (8 + 4) and rep['tiles_evaluated'] == int(res.tiles_evaluated.sum())
    host = aq.acquire_system_host(models, XVARS, YVARS, 'yield', pool, constraints=LIMIT, picks=6, criterion=criterion,
                                  sense=sense, no_feasible=0.3)
    follow_the_device(models, pool, host, criterion, sense)     # the statement meets the same conditions
    assert np.allclose(res.incumbent, host.incumbent, rtol=1e-12, atol=0.0)
    assert np.array_equal(res.measured_feasible, host.measured_feasible)


def test_lazy_and_full_agree_and_measured_rows_may_be_given(device_ctx):
    models, pool, measured = models_case(3)
    backend = engine.HipBackend(device_ctx)
    kw = dict(constraints=LIMIT, picks=6, no_feasible=0.3, device=backend)
    lazy = aq.acquire_system(models, XVARS, YVARS, 'yield', pool, **kw)
    full = aq.acquire_system(models, XVARS, YVARS, 'yield', pool, lazy=False, **kw)
    given = aq.acquire_system(models, XVARS, YVARS, 'yield', pool, measured=measured, grid_cap=1, **kw)
    assert np.array_equal(lazy.index, full.index) and np.array_equal(lazy.index, given.index)
    for name in ('gain', 'joint', 'incumbent', 'incumbent_after', 'feasible_draws'):
        assert lazy[name].tobytes() == full[name].tobytes(), name
    assert np.allclose(given.incumbent, lazy.incumbent, rtol=1e-12, atol=0.0)
    assert np.all(full.tiles_evaluated == 3) and lazy.first is None and lazy.gain[1] > 0.0
    tight = aq.acquire_system(models, XVARS, YVARS, 'yield', pool, constraints={'impurity': (None, -0.35)}, picks=3,
                              criterion='pi', device=backend)
    assert np.any(tight.measured_feasible == 0)
    assert np.array_equal(tight.incumbent == -np.inf, tight.measured_feasible == 0)
    with pytest.raises(ValueError, match='of the 30 draws have no feasible measured row.*no_feasible='):
        aq.acquire_system(models, XVARS, YVARS, 'yield', pool, constraints={'impurity': (None, -0.35)}, picks=3, device=backend)

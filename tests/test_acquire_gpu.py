"""FoKL.acquire / fokl_acquire_select (csrc/fokl_acquire_device.inc) on the device against from-scratch arithmetic on the host.

Models are built as test_design_gpu builds them (``mtx`` directly, Bernoulli kernel, seeded uniform training inputs and
pools), with seeded draws around one coefficient vector.  The device is followed along its OWN picks: at every pick the
host forms f = X betas' in numpy, updates the incumbent with the device's earlier picks and recomputes every row's
criterion from scratch; the device's gain must match the host's value at the device's index within test_design_gpu.GATE
(1e-9 relative) and be within that gate of the host's maximum, so a near-tie decided differently by the order of a sum is
not a failure.
"""
import numpy as np
import pytest

from test_design_gpu import GATE, KERNEL, PHIS, columns, model_of, pool_of
from fokl_gpy_amd import acquire as aq

pytestmark = pytest.mark.gpu

NC = 29
DRAWS = 120


def fitted(device_ctx, nc=NC, E=DRAWS):
    """test_design_gpu's model with E draws: a coefficient vector and 30 % of spread around it."""
    model = model_of(device_ctx, nc)
    rng = np.random.default_rng(nc + E)
    model.betas = rng.standard_normal(nc) * (1.0 + 0.3 * rng.standard_normal((E, nc)))
    return model


def follow_the_device(model, pool, res, criterion, sense):
    sign = 1.0 if sense == 'max' else -1.0
    F = sign * (columns(pool, model.mtx) @ model.betas[-res.draws:].T)
    b = sign * res.incumbent
    worst_pick = worst_gain = 0.0
    for k in range(res.picks):                                    # no step is left out
        crit = aq.gain_rows(F, b, criterion)
        crit[res.index[:k]] = -np.inf
        i = int(res.index[k])
        assert crit[i] >= crit.max() * (1.0 - GATE), k
        assert abs(res.gain[k] - crit[i]) <= GATE * abs(crit[i]), k
        if crit.max() > 0.0:
            worst_pick = max(worst_pick, 1.0 - crit[i] / crit.max())
            worst_gain = max(worst_gain, abs(res.gain[k] - crit[i]) / abs(crit[i]))
        b = np.where(F[i] > b, F[i] if criterion == 'ei' else np.inf, b)
    assert np.allclose(sign * res.incumbent_after, b, rtol=1e-12, atol=0.0)
    assert np.array_equal(res.joint, np.cumsum(res.gain)) and np.array_equal(res.x, pool[res.index])
    assert len(set(res.index.tolist())) == res.picks
    return worst_pick, worst_gain


@pytest.mark.parametrize('criterion', aq.CRITERIA)
@pytest.mark.parametrize('sense', aq.SENSES)
@pytest.mark.parametrize('S', (17, 1029))
def test_pick_loop_along_the_devices_own_path(device_ctx, S, sense, criterion):
    model, pool = fitted(device_ctx), pool_of(S, S + 1)
    res = model.acquire(pool=pool, picks=8, criterion=criterion, sense=sense, keep='first')
    assert (res.gain[0] > 0.0 or S == 17) and res.draws == DRAWS and res.rows == S      # 17 rows may hold no improvement
    worst_pick, worst_gain = follow_the_device(model, pool, res, criterion, sense)
    print(f"S {S} {criterion} {sense}: gains {res.gain[0]:.3g} .. {res.gain[-1]:.3g}, worst shortfall of a pick {worst_pick:.3g}, "
          f"worst relative error of a gain {worst_gain:.3g}, tiles per pick {res.tiles_evaluated.tolist()}")
    # the map before the first pick: every term of a row's sum is off by a few ulp of |f| at most, 1e-12 of the scale
    sign = 1.0 if sense == 'max' else -1.0
    F = sign * (columns(pool, model.mtx) @ model.betas.T)
    first = aq.gain_rows(F, sign * res.incumbent, criterion)
    assert res.first.shape == (S,) and np.max(np.abs(res.first - first)) <= 1e-12 * np.abs(F).max()
    assert res.first[res.index[0]] == res.gain[0] == res.first.max()
    rep = device_ctx.acquire_report()
    assert rep['instance'] == criterion and rep['lazy'] and rep['picks'] == 8 and rep['launches'] == 2 + 4 * 7
    assert rep['lds_bytes'] == 8 * 16 * 32 and rep['tiles_evaluated'] == int(res.tiles_evaluated.sum())


@pytest.mark.parametrize('criterion', aq.CRITERIA)
def test_lazy_and_full_agree_and_the_host_statement_picks_alike(device_ctx, criterion):
    model, pool = fitted(device_ctx), pool_of(1029, 5)
    lazy = model.acquire(pool=pool, picks=8, criterion=criterion)
    full = model.acquire(pool=pool, picks=8, criterion=criterion, lazy=False)
    assert np.array_equal(lazy.index, full.index)
    for name in ('gain', 'joint', 'incumbent', 'incumbent_after'):
        assert lazy[name].tobytes() == full[name].tobytes(), name
    assert np.all(full.tiles_evaluated == 65) and lazy.tiles_evaluated[0] == 65 and np.all(lazy.tiles_evaluated <= 65)
    host = aq.acquire_host(model.betas, model.mtx, PHIS, KERNEL, model.inputs, pool, picks=8, criterion=criterion)
    follow_the_device(model, pool, host, criterion, 'max')        # the statement meets the same conditions
    assert np.allclose(lazy.incumbent, host.incumbent, rtol=1e-12, atol=0.0)


def test_the_training_incumbent_is_propagates_extreme_of_the_same_draws(device_ctx):
    model, pool = fitted(device_ctx), pool_of(200, 9)
    pop = model.propagate()
    assert np.array_equal(model.acquire(pool=pool, picks=1).incumbent, pop.max)
    assert np.array_equal(model.acquire(pool=pool, picks=1, sense='min').incumbent, pop.min)
    last = model.acquire(pool=pool, picks=1, draws=40)
    assert np.array_equal(last.incumbent, model.propagate(draws=40).max) and last.draws == 40
    post = dict(betas=np.concatenate([model.betas[:10], np.full((1, NC), np.nan)]), sigsqd=None)
    with pytest.raises(ValueError, match=r"1 of the 11 draws are NaN or infinite \(the rows of a resample's flagged chains"):
        model.acquire(post, pool=pool)
    res = model.acquire(post, pool=pool, picks=2, draws=np.arange(10), incumbent=0.0, criterion='pi')
    assert res.draws == 10 and np.all(res.incumbent == 0.0)
    with pytest.raises(ValueError, match="criterion='ei' needs a finite incumbent"):
        model.acquire(pool=pool, incumbent='none')
    none = model.acquire(pool=pool, picks=2, incumbent='none', criterion='pi')
    assert none.index.tolist() == [0, 1] and none.gain.tolist() == [1.0, 0.0]


def test_same_call_same_bytes_whatever_the_grid_and_nothing_drawn_at_random(device_ctx):
    model, pool = fitted(device_ctx), pool_of(1029, 11)
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    kw = dict(pool=pool, picks=10, criterion='ei', keep='first')
    a, b = model.acquire(**kw), model.acquire(**kw)
    default_grid = device_ctx.acquire_report()
    one = model.acquire(grid_cap=1, **kw)
    capped = device_ctx.acquire_report()
    assert np.array_equal(np.random.get_state()[1], state)
    assert default_grid['grid'] > 1 and capped['grid'] == capped['bound_grid'] == 1
    for name in ('index', 'gain', 'joint', 'incumbent', 'incumbent_after', 'first', 'tiles_evaluated'):
        assert a[name].tobytes() == b[name].tobytes(), name
        assert a[name].tobytes() == one[name].tobytes(), name


def test_clean_normalises_the_pool_and_returns_its_rows_as_passed(device_ctx):
    model = fitted(device_ctx)
    model.minmax = [[-1.0, 3.0]] * 4
    raw = -1.0 + 4.0 * pool_of(100, 13)
    res = model.acquire(pool=raw, clean=True, picks=3)
    same = model.acquire(pool=pool_of(100, 13), picks=3)
    assert np.array_equal(res.index, same.index) and np.array_equal(res.x, raw[res.index])
    assert np.allclose(res.x_normalised, same.x, rtol=0.0, atol=1e-15) and np.allclose(res.gain, same.gain, rtol=1e-9)

"""FoKL.design / fokl_design_select (csrc/fokl_design_device.inc) on the device against from-scratch arithmetic on the host.

Models are built directly from ``mtx`` (no search), Bernoulli kernel, training inputs and pools seeded continuous uniform.
Every reference is formed from scratch on the CPU -- inv(A0 + X_D' X_D) from the DEVICE's own picks, never the downdates --
and every case asserts cond(A0) <= 1e4 first, so that the project's fixed relative gate of 1e-9 means something: the
device's Gram and quadratic forms differ from numpy's by rounding (1e-16) times that condition number.

The pick loop is followed along the device's own path: at every step the device's pick must reach the from-scratch maximum
to 1e-9 relative (a near-tie decided by rounding is not an error) and its reported gain must match to 1e-9.  Identity
with design_host's picks is asked only of a pool whose top-two margin is asserted to be above 1e-6 at every step.
"""
import itertools

import numpy as np
import pytest

from helpers import upload
from fokl_gpy_amd import _capi, engine, FoKLRoutines, getKernels
from fokl_gpy_amd import design as dg
from fokl_gpy_amd.embedded import basis_matrix
from oracle import fokl_oracle as O

pytestmark = pytest.mark.gpu

KERNEL = 'Bernoulli Polynomials'
PHIS = getKernels.bernoulli()
INPUTS = 4
TRAIN_ROWS = 200
TAUSQD = 1.0
GATE = 1e-9
_CASES = {}


def model_mtx(nc):
    """nc - 1 terms in four inputs, orders up to 3, lowest total order first."""
    rows = sorted((r for r in itertools.product(range(4), repeat=INPUTS) if any(r)),
                  key=lambda r: (sum(r), sum(1 for v in r if v), r))
    return np.array(rows[:nc - 1]).reshape(nc - 1, INPUTS)


def columns(x, mtx):
    return basis_matrix(x, mtx, PHIS, KERNEL) if mtx.shape[0] else np.ones((x.shape[0], 1))


def case(nc):
    """(mtx, training inputs, A0, M of the training inputs) of the nc-column model; made once and never changed."""
    if nc not in _CASES:
        mtx = model_mtx(nc)
        train = np.random.default_rng(nc).random((TRAIN_ROWS, INPUTS))
        Xt = columns(train, mtx)
        G = Xt.T @ Xt
        A0 = G + np.eye(nc) / TAUSQD
        assert np.linalg.cond(A0) <= 1e4
        for a in (train, A0, G):
            a.setflags(write=False)
        _CASES[nc] = (mtx, train, A0, G / TRAIN_ROWS)
    return _CASES[nc]


def pool_of(S, seed):
    return np.random.default_rng(1000 + seed).random((S, INPUTS))


def model_of(device_ctx, nc):
    mtx, train, _, _ = case(nc)
    model = FoKLRoutines.FoKL(kernel=KERNEL, UserWarnings=False, ConsoleOutput=False)
    model.mtx, model.betas, model.inputs = mtx, np.zeros((4, nc)), train
    model._backend_override = engine.HipBackend(device_ctx)
    return model


def criterion_from_scratch(nc, X, picked, criterion, masked=True):
    """The criterion of every pool row after the picks ``picked``, from inv(A0 + X_D' X_D); picked rows -inf if ``masked``."""
    _, _, A0, M = case(nc)
    XD = X[np.asarray(picked, dtype=int)]
    C = np.linalg.inv(A0 + XD.T @ XD)
    v = np.einsum('si,ij,sj->s', X, C, X)
    crit = v
    if criterion == 'ivr':
        crit = np.einsum('si,ij,sj->s', X, C @ M @ C, X) / (1.0 + v)
    crit = crit.copy()
    if masked:
        crit[np.asarray(picked, dtype=int)] = -np.inf
    return crit, v


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('nc', (2, 5, 29, 102))
@pytest.mark.parametrize('S', (1, 15, 16, 17, 1029))
def test_first_pass_and_one_downdate(device_ctx, S, nc, criterion):
    """v of every row after one pick: the MFMA first pass (tile edges, column padding to 4, the 16-row blocks of the matrix)
    and one downdate, against x' inv(A0 + x* x*') x."""
    model, pool = model_of(device_ctx, nc), pool_of(S, S + nc)
    res = model.design(pool=pool, tausqd=TAUSQD, picks=1, criterion=criterion, replicates=True, keep='variance')
    X = columns(pool, model.mtx)
    crit0, _ = criterion_from_scratch(nc, X, [], criterion)
    i = int(res.index[0])
    print(f"S {S} nc {nc} {criterion}: pick {i}, gain {res.gain[0]:.17g} against {crit0.max():.17g}")
    assert crit0[i] >= crit0.max() * (1.0 - GATE)
    assert abs(res.gain[0] - crit0[i]) <= GATE * abs(crit0[i])
    _, v1 = criterion_from_scratch(nc, X, [i], criterion)
    err = np.max(np.abs(res.variance - v1) / np.abs(v1))
    print(f"   v after one downdate: max relative error {err:.3g}")
    assert res.variance.shape == (S,) and err <= GATE
    assert np.array_equal(res.x, pool[res.index]) and np.allclose(res.x_basis, X[res.index], rtol=1e-12, atol=1e-15)
    rep = device_ctx.design_report()
    assert rep['instance'] == criterion and rep['row_tiles'] == -(-S // 16) and 1 <= rep['grid'] <= rep['row_tiles']
    assert rep['lds_bytes'] == 8 * 16 * (-(-nc // 16) * 16) and rep['launches'] == 4


def follow_the_device(device_ctx, S, nc, picks, criterion, refresh_every):
    model, pool = model_of(device_ctx, nc), pool_of(S, 7 * S + picks)
    res = model.design(pool=pool, tausqd=TAUSQD, picks=picks, criterion=criterion, refresh_every=refresh_every)
    X = columns(pool, model.mtx)
    assert len(set(res.index.tolist())) == picks
    worst_pick = worst_gain = 0.0
    for k in range(picks):                                        # no step is left out
        crit, v = criterion_from_scratch(nc, X, res.index[:k], criterion)
        i = int(res.index[k])
        worst_pick = max(worst_pick, 1.0 - crit[i] / crit.max())
        worst_gain = max(worst_gain, abs(res.gain[k] - crit[i]) / abs(crit[i]))
        assert crit[i] >= crit.max() * (1.0 - GATE), k
        assert abs(res.gain[k] - crit[i]) <= GATE * abs(crit[i]), k
        assert abs(res.vstar[k] - v[i]) <= GATE * abs(v[i]), k
    print(f"S {S} nc {nc} picks {picks} {criterion} refresh {refresh_every}: worst shortfall of a pick {worst_pick:.3g}, "
          f"worst relative error of a gain {worst_gain:.3g}")
    _, _, A0, _ = case(nc)
    XD = X[res.index]
    assert abs(np.linalg.slogdet(A0 + XD.T @ XD)[1] - np.linalg.slogdet(A0)[1] - res.logdet_gain[-1]) <= 1e-9 * picks
    rep = device_ctx.design_report()
    assert rep['picks'] == picks and rep['refreshes'] == ((picks - 1) // refresh_every if refresh_every else 0)
    assert rep['launches'] == 1 + rep['refreshes'] + 2 * picks and rep['kernel_us'] > 0
    return res


@pytest.mark.parametrize('criterion', dg.CRITERIA)
@pytest.mark.parametrize('refresh_every', (0, 7))
def test_pick_loop_along_the_devices_own_path(device_ctx, criterion, refresh_every):
    follow_the_device(device_ctx, 1029, 29, 40, criterion, refresh_every)


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_pick_loop_until_the_pool_is_exhausted(device_ctx, criterion):
    res = follow_the_device(device_ctx, 17, 29, 17, criterion, 0)
    assert sorted(res.index.tolist()) == list(range(17))


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_well_separated_pool_gives_the_host_statements_picks(device_ctx, criterion):
    nc, picks = 5, 10
    model = model_of(device_ctx, nc)
    pool = np.random.default_rng(100).random((12, INPUTS))
    host = dg.design_host(model.mtx, PHIS, KERNEL, model.inputs, pool, picks=picks, criterion=criterion, inv_tausqd=1.0 / TAUSQD)
    X = columns(pool, model.mtx)
    for k in range(picks):                                        # separation, on the CPU, at every step
        top = np.sort(criterion_from_scratch(nc, X, host.index[:k], criterion)[0])[::-1]
        assert (top[0] - top[1]) > 1e-6 * top[0], k
    res = model.design(pool=pool, tausqd=TAUSQD, picks=picks, criterion=criterion)
    assert np.array_equal(res.index, host.index)
    assert np.allclose(res.gain, host.gain, rtol=GATE, atol=0.0)
    assert np.allclose(res.logdet_gain, host.logdet_gain, rtol=GATE, atol=0.0)
    if criterion == 'ivr':
        assert np.allclose(res.target_var, host.target_var, rtol=GATE, atol=0.0)


@pytest.mark.parametrize('criterion', dg.CRITERIA)
def test_ties_go_to_the_lowest_index(device_ctx, criterion):
    nc = 29
    model, pool = model_of(device_ctx, nc), pool_of(1029, 3)
    first = int(np.argmax(criterion_from_scratch(nc, columns(pool, model.mtx), [], criterion)[0]))
    pool[[3, first]] = pool[[first, 3]]                           # the best row to index 3 ...
    pool[700] = pool[3]                                           # ... and its exact copy to index 700
    res = model.design(pool=pool, tausqd=TAUSQD, picks=6, criterion=criterion)
    assert res.index[0] == 3 and 3 not in res.index[1:] and len(set(res.index.tolist())) == 6
    rep = model.design(pool=pool, tausqd=TAUSQD, picks=6, criterion=criterion, replicates=True)
    assert rep.index[0] == 3 and 700 not in rep.index             # identical rows tie at every step: the lower one wins
    weak = model.design(pool=pool[:17], tausqd=TAUSQD, picks=40, criterion=criterion, replicates=True)
    assert len(set(weak.index.tolist())) < 40                     # 40 picks from 17 rows: rows are repeated


def test_same_call_same_bytes_whatever_the_grid(device_ctx):
    model, pool = model_of(device_ctx, 29), pool_of(1029, 11)
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    kw = dict(pool=pool, tausqd=TAUSQD, picks=10, criterion='ivr', refresh_every=4, keep='variance')
    a, b = model.design(**kw), model.design(**kw)
    default_grids = device_ctx.design_report()
    one = model.design(grid_cap=1, **kw)
    capped = device_ctx.design_report()
    assert np.array_equal(np.random.get_state()[1], state)
    assert default_grids['step_grid'] > 1 and default_grids['grid'] > 1 and capped['step_grid'] == capped['grid'] == 1
    for name in ('index', 'gain', 'vstar', 'x_basis', 'logdet_gain', 'target_var', 'variance'):
        assert a[name].tobytes() == b[name].tobytes(), name
        assert a[name].tobytes() == one[name].tobytes(), name


def test_report_says_what_the_call_implies(device_ctx):
    model, pool = model_of(device_ctx, 5), pool_of(1029, 13)
    model.design(pool=pool, tausqd=TAUSQD, picks=9, criterion='variance', refresh_every=4, keep='variance')
    rep = device_ctx.design_report()
    assert rep['instance'] == 'variance' and rep['row_tiles'] == 65 and rep['picks'] == 9 and rep['refreshes'] == 2
    assert rep['launches'] == 3 + 2 * 9 + 1 and rep['lds_bytes'] == 8 * 16 * 16
    assert rep['kernel_us'] >= rep['quadform_us'] > 0
    post = dict(tausqd=np.array([0.5, 2.0, np.nan]), sigsqd=np.array([0.1, 0.3, np.nan]))
    res = model.design(post, pool=pool, picks=2, criterion='ivr')
    assert res.inv_tausqd == pytest.approx(1.25) and res.sigsqd_mean == pytest.approx(0.2)
    assert device_ctx.design_report()['instance'] == 'ivr'


def test_too_many_columns_are_refused_with_nothing_launched(device_ctx):
    upload(device_ctx, np.linspace(0.0, 1.0, 40).reshape(40, 1), np.zeros(40), O.KERNEL_BERNOULLI)
    slots = np.zeros(769, dtype=np.int32)                            # 769 times the ones column
    device_ctx.timing_enable(True)
    device_ctx.timing_reset()
    try:
        with pytest.raises(_capi.FoklNativeError, match='769 columns.*FOKL_DESIGN_MAX_COLUMNS = 768'):
            device_ctx.design_select(slots, np.eye(769), None, picks=1)
        assert device_ctx.timing_get(_capi.K_DESIGN)['launches'] == 0
    finally:
        device_ctx.timing_enable(False)
    rep = device_ctx.design_report()
    assert rep['instance'] == 'none' and rep['launches'] == 0 and rep['picks'] == 0
    with pytest.raises(_capi.FoklNativeError, match='41 picks from a pool of 40 rows need replicates'):
        device_ctx.design_select(slots[:1], np.eye(1), None, picks=41)
    with pytest.raises(ValueError, match='769 columns'):
        wide = np.array([r for r in itertools.product(range(10), repeat=3) if any(r)][:768])
        dg.design(wide, PHIS, KERNEL, np.zeros((3, 3)), np.zeros((3, 3)), picks=1, inv_tausqd=1.0,
                  device=engine.HipBackend(device_ctx))

"""The embedded-GP sampler on the device (fokl_embedded_hmc: one workgroup per chain) against its numpy statement
(embedded.full_sample_host / chain_host), value for value from the same counter-based random numbers."""
import os

import numpy as np
import pytest

from embedded_reference import term_scales
from helpers import GOLDEN
from fokl_gpy_amd import _capi, embedded, engine, getKernels

pytestmark = pytest.mark.gpu

EQUATIONS = ('identity', 'cstr', 'ratio')


def make_model(equation, K, T, N, kernel, seed=0):
    """A model of K GPs over two inputs with T terms and N rows whose equation is finite around q = 0.3 noise."""
    rng = np.random.default_rng(1000 * K + 10 * T + N + seed)
    x = rng.random((N, 2))
    cols = [0.5 + rng.random(N) for _ in range(3)]
    model = embedded.Embedded_GP_Model(*[embedded.GP() for _ in range(K)], kernel=kernel)
    model.inputs, model.data = x, rng.standard_normal(N)
    model.phis = getKernels.sp500() if kernel == 'Cubic Splines' else getKernels.bernoulli()
    G = lambda k: model.Processed_GPs[k % K]
    if equation == 'identity':
        eq = lambda: sum((G(k) for k in range(1, K)), G(0))
    elif equation == 'cstr':
        eq = lambda: -(np.exp(-G(0)) * cols[0] * cols[1] - np.exp(-G(1)) * cols[2])
    else:
        eq = lambda: np.log(np.square(G(0)) + 1.5) / (cols[0] + G(1) ** 2) + (cols[1] * G(2) + 30.0) ** 1.5 - np.sqrt(cols[2])
    model.set_equation(eq)
    orders = [(1 + t % 5, (t // 5) % 4) for t in range(T)]
    model.discmtx = np.array(orders[:T])
    return model


def launch(ctx, model, chains, draws, **kw):
    session = embedded._DeviceSession(model, model.tape, ctx)
    return session.sample(model.discmtx, chains, draws, kw.pop('leapfrog', 20), kw.pop('seed', 0), **kw)


@pytest.mark.parametrize('kernel', embedded.KERNELS)
@pytest.mark.parametrize('equation', EQUATIONS)
def test_potential_and_gradient(device_ctx, equation, kernel):
    for K, T, N in ((1, 1, 1), (2, 10, 63), (8, 31, 64), (2, 31, 257), (8, 10, 4000), (1, 10, 64)):
        model = make_model(equation, K, T, N, kernel)
        D = K * (T + 1) + 1
        q0 = 0.3 * np.random.default_rng(K + T + N).standard_normal((20, D))
        dev = launch(device_ctx, model, 20, 0, q0=q0, eps0=0.1, want_grad0=True)
        pot = model.host_potential()
        X = embedded.basis_matrix(model._inputs(), model.discmtx, model.phis, kernel)
        for c in range(20):
            U, g = pot(q0[c])
            # the size of the terms the sums are made of
            B = q0[c, :-1].reshape(K, T + 1)
            values = model.tape.forward(B @ X.T)
            e = model._data() - values[model.tape.result & 255]
            scale_U, scale_g = term_scales(q0[c], X, e, model.tape.backward(values))
            assert abs(dev['potential'][c, 0] - U) <= 1e-11 * scale_U, (K, T, N, c)
            assert np.all(np.abs(dev['grad0'][c] - g) <= 1e-11 * scale_g + 1e-300), (K, T, N, c)
            assert np.array_equal(dev['states'][c, 0], q0[c])


def test_one_transition_equals_the_statement(device_ctx):
    for equation, K, T, N in (('cstr', 2, 10, 257), ('ratio', 3, 5, 1000), ('identity', 1, 3, 64)):
        model = make_model(equation, K, T, N, 'Cubic Splines')
        D = K * (T + 1) + 1
        q0 = 0.3 * np.random.default_rng(5).standard_normal((6, D))
        dev = launch(device_ctx, model, 6, 1, q0=q0, eps0=1e-5, adapt=False, seed=11, want_proposal=True)
        pot = model.host_potential()
        for c in range(6):
            host = embedded.chain_host(pot, D, c, 1, 20, 11, q0[c], 1e-5, False)
            scale = max(1.0, abs(host['proposal'][-1]))
            assert np.max(np.abs(dev['proposal'][c, :-1] - host['proposal'][:-1])) < 1e-9
            assert abs(dev['proposal'][c, -1] - host['proposal'][-1]) < 1e-9 * scale
            assert dev['accepted'][c, 1] == host['accepted'][1]
            assert np.max(np.abs(dev['states'][c, 1] - host['states'][1])) < 1e-9


def test_chains_follow_the_statement_and_do_not_depend_on_the_grid(device_ctx):
    model = make_model('cstr', 2, 6, 500, 'Bernoulli Polynomials')
    D = 2 * 7 + 1
    q0 = np.tile(0.2 * np.random.default_rng(9).standard_normal(D), (64, 1))
    few = launch(device_ctx, model, 8, 60, q0=q0[:8], eps0=2e-3, adapt=False, seed=3)
    many = launch(device_ctx, model, 64, 60, q0=q0, eps0=2e-3, adapt=False, seed=3)
    for key in ('states', 'potential', 'accepted'):
        assert np.array_equal(few[key][3], many[key][3]), key                 # bitwise: chain 3 of 8 is chain 3 of 64
    assert not np.array_equal(many['states'][3], many['states'][4])
    pot = model.host_potential()
    compared = 0
    for c in range(4):
        host = embedded.chain_host(pot, D, c, 60, 20, 3, q0[c], 2e-3, False)
        if np.array_equal(host['accepted'], few['accepted'][c]):
            compared += 1
            assert np.max(np.abs(host['states'] - few['states'][c])) < 1e-7
            assert host['accepted'].sum() > 5
    assert compared >= 3


def test_adaptation_and_mass_update_inside_the_kernel(device_ctx):
    """A 600-draw chain on a conjugate problem: the step-size history, the inverse mass and the second step search."""
    rng = np.random.default_rng(4)
    N = 300
    model = embedded.Embedded_GP_Model(embedded.GP(), kernel='Bernoulli Polynomials')
    model.inputs, model.phis = rng.random((N, 1)), getKernels.bernoulli()
    model.data = 1.0 + 0.5 * model.inputs[:, 0] + 0.3 * rng.standard_normal(N)
    model.set_equation(lambda: model.Processed_GPs[0])
    model.discmtx = np.array([[1], [2]])
    dev = launch(device_ctx, model, 2, 600, seed=21)
    pot = model.host_potential()
    for c in range(2):
        host = embedded.chain_host(pot, 4, c, 600, 20, 21)
        assert dev['status'][c] == embedded.OK and dev['mass_updated'][c] and host['mass_updated']
        same = np.array_equal(host['accepted'], dev['accepted'][c])
        first = 600 if same else int(np.argmax(host['accepted'] != dev['accepted'][c]))
        assert first > 100                       # (a flip needs u within rounding of its threshold)
        windows = first // 50
        assert np.allclose(dev['eps_hist'][c, :windows], host['eps_hist'][:windows], rtol=1e-9, atol=0)
        if same:
            assert np.allclose(dev['inv_mass'][c], host['inv_mass'], rtol=1e-6)
            assert np.isclose(dev['eps_final'][c], host['eps_final'], rtol=1e-9)
        assert 0.2 < dev['accepted'][c, 300:].mean() <= 1.0


def test_refusals_from_python_and_natively(device_ctx):
    model = make_model('cstr', 2, 3, 100, 'Cubic Splines')
    session = embedded._DeviceSession(model, model.tape, device_ctx)
    slots = [_capi.SLOT_ONES] + session.pool.take(3)
    ops, cols, consts = model.tape.arrays()
    good = dict(n_gps=2, term_slots=slots, col_slots=session.col_slots, ops=ops, consts=consts, result=model.tape.result,
                chains=1, draws=0, leapfrog=20, seed=0)

    def refused(text, **change):
        with pytest.raises(_capi.FoklNativeError) as err:
            device_ctx.embedded_hmc(**{**good, **change})
        assert err.value.code == -2 and text in str(err.value), str(err.value)

    device_ctx.build_terms(np.array([[1, 0], [0, 1], [1, 1]], dtype=np.int32), slots[1:])
    device_ctx.embedded_hmc(**good)
    refused('GPs', n_gps=9)
    refused('columns', col_slots=list(range(2, 19)))
    refused('operations', ops=np.tile(ops[:1], (33, 1)))
    refused('parameters', n_gps=8, term_slots=[0] * 33)
    refused('chains', chains=5000)
    refused('chains', leapfrog=0)
    refused('opcode', ops=np.array([[11, 0, 0]], dtype=np.int32), result=2)
    refused('not computed before', ops=np.array([[0, 0, 2]], dtype=np.int32), result=2)
    refused('column', ops=np.array([[2, 0, (1 << 8) | 7]], dtype=np.int32), result=2)
    refused('constant', ops=np.array([[10, 0, (2 << 8) | 5]], dtype=np.int32), result=2)
    refused('exponent', ops=np.array([[10, 0, 1]], dtype=np.int32), result=2)
    refused('result', result=(1 << 8))
    refused('slot', term_slots=[0, 100000, 3, 4])
    # Python refuses before anything is launched
    big = embedded.Embedded_GP_Model(embedded.GP(), kernel='Bernoulli Polynomials')
    big.inputs, big.phis, big.data = np.random.default_rng(0).random((100, 2)), getKernels.bernoulli(), np.zeros(100)
    big.set_equation(lambda: big.Processed_GPs[0])
    big.discmtx = np.ones((256, 2), dtype=int)
    with pytest.raises(ValueError, match='parameters'):
        big.full_sample(10, device=device_ctx)
    big.discmtx = np.ones((3, 2), dtype=int)
    with pytest.raises(ValueError, match='chains'):
        big.full_sample(10, chains=5000, device=device_ctx)
    # 4 194 304 values: refused by both sides with a message that says why
    wide = embedded.Embedded_GP_Model(embedded.GP(), kernel='Bernoulli Polynomials')
    wide.inputs, wide.phis, wide.data = np.random.default_rng(0).random((70000, 1)), getKernels.bernoulli(), np.zeros(70000)
    wide.set_equation(lambda: wide.Processed_GPs[0])
    wide.discmtx = np.array([[1 + t % 20] for t in range(60)])
    with pytest.raises(ValueError, match='last-level cache'):
        wide.full_sample(10, device=device_ctx)
    wsession = embedded._DeviceSession(wide, wide.tape, device_ctx)
    with pytest.raises(_capi.FoklNativeError, match='last-level cache'):
        wsession.sample(wide.discmtx, 1, 0, 20, 0)


def cstr_model():
    d = np.load(os.path.join(GOLDEN, 'cstr_embedded.npz'))
    x = (d['Temperature_Inv'] - 1 / 600) / (1 / 300 - 1 / 600)
    model = embedded.Embedded_GP_Model(embedded.GP(), embedded.GP())
    model.inputs, model.phis, model.data = x[:, None], getKernels.sp500(), d['r_co2']
    CA, CB, CC = d['C_CO2'], d['C_Sites'], d['C_CO2_ADS']
    model.set_equation(lambda: -(np.exp(-model.Processed_GPs[0]) * CA * CB - np.exp(-model.Processed_GPs[1]) * CC))
    return model


def test_cstr_end_to_end_and_numpys_stream_is_left_alone(device_ctx):
    np.random.seed(123)
    before = np.random.get_state()
    model = cstr_model()
    samples, mtx, evs = model.full_routine(draws=1500, tolerance=0, chains=8, device=device_ctx)
    assert samples.shape == (8, 1501, 2 * (mtx.shape[0] + 1) + 1) and len(evs) >= 2
    assert np.all(model.diagnostics['status'] == embedded.OK)
    assert np.nanmax(model.diagnostics['rhat']) < 1.1, model.diagnostics['rhat']
    inv_T = 1.0 / np.linspace(300, 600, 50)
    x_new = ((inv_T - 1 / 600) / (1 / 300 - 1 / 600))[:, None]
    for k, slope in ((0, 100.0), (1, 200.0)):                       # the generating rate laws: k = exp(-slope / T)
        mean, bounds = model.evaluate(x_new, GP_number=k, draws=100, ReturnBounds=1, device=device_ctx)
        assert np.max(np.abs(np.exp(-mean) / np.exp(-slope * inv_T) - 1.0)) < 0.05
        assert np.all(bounds[:, 0] <= mean + 1e-12) and np.all(mean <= bounds[:, 1] + 1e-12)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]

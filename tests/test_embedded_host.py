"""Embedded GPs without a device: the tracer, the potential and its gradient, and the numpy statement of the sampler
(embedded.full_sample_host / full_routine_host) that the kernel is tested against."""
import numpy as np
import pytest

from fokl_gpy_amd import embedded, getKernels


def new_model(K, N, kernel='Bernoulli Polynomials', m=1, seed=0):
    rng = np.random.default_rng(seed)
    model = embedded.Embedded_GP_Model(*[embedded.GP() for _ in range(K)], kernel=kernel)
    model.inputs, model.data = rng.random((N, m)), rng.standard_normal(N)
    model.phis = getKernels.sp500() if kernel == 'Cubic Splines' else getKernels.bernoulli()
    return model, rng


def test_tracing_the_cstr_equation_and_a_shared_subexpression():
    model, rng = new_model(2, 50)
    CA, CB, CC = (0.5 + rng.random(50) for _ in range(3))
    tape = model.set_equation(lambda: -(np.exp(-model.Processed_GPs[0]) * CA * CB - np.exp(-model.Processed_GPs[1]) * CC))
    assert len(tape.columns) == 3 and tape.consts == [] and len(tape.ops) == 9
    assert [embedded.OP_NAMES[o[0]] for o in tape.ops] == ['negative', 'exp', 'multiply', 'multiply', 'negative', 'exp',
                                                           'multiply', 'subtract', 'negative']
    g = rng.standard_normal((2, 50))
    assert np.allclose(tape.evaluate(g), -(np.exp(-g[0]) * CA * CB - np.exp(-g[1]) * CC), rtol=1e-15)

    def nested():
        shared = np.exp(model.Processed_GPs[0] * 2.0)                      # written twice, recorded once
        again = np.exp(2.0 * model.Processed_GPs[0])
        return (shared + CA) / (again + CA) + np.sqrt(np.square(model.Processed_GPs[1]) + 3) ** 1.5 - 3 * np.log(again + 1.0)
    tape = model.set_equation(nested)
    names = [embedded.OP_NAMES[o[0]] for o in tape.ops]
    assert names.count('exp') == 1 and names.count('add') == 4 and len(tape.columns) == 1
    assert sorted(tape.consts) == [1.0, 1.5, 2.0, 3.0]
    e = np.exp(2 * g[0])
    assert np.allclose(tape.evaluate(g), (e + CA) / (e + CA) + np.sqrt(g[1] ** 2 + 3) ** 1.5 - 3 * np.log(e + 1), rtol=1e-14)
    for o, (code, a, b) in enumerate(tape.ops):                           # single assignment: operands precede their use
        for operand in ((a, b) if code <= embedded.DIV else (a,)):
            assert operand >> 8 != embedded.KIND_SLOT or (operand & 255) < 2 + o


@pytest.mark.parametrize('name, equation', [
    ('sin', lambda G, c: np.sin(G[0])), ('tanh', lambda G, c: np.tanh(G[0]) * c), ('less', lambda G, c: G[0] < 1.0),
    ('maximum', lambda G, c: np.maximum(G[0], 0.0)), ('shape', lambda G, c: G[0] * c[:10]),
    ('shape', lambda G, c: G[0] + np.ones((50, 2))), ('power', lambda G, c: 2.0 ** G[0]), ('power', lambda G, c: G[0] ** G[1]),
    ('power', lambda G, c: G[0] ** c), ('add', lambda G, c: np.add.reduce(G[0])), ('absolute', lambda G, c: abs(G[0])),
    ('does not depend', lambda G, c: c * 2.0), ('type str', lambda G, c: G[0] + 'a'),
    ('operation 33', lambda G, c: sum((np.exp(G[0] * float(k)) for k in range(2, 40)), G[1])),
    ('columns', lambda G, c: sum((G[0] * (c + k) for k in range(17)), G[1])),
])
def test_what_a_tape_cannot_hold_is_refused_by_name(name, equation):
    model, rng = new_model(2, 50)
    c = rng.random(50)
    with pytest.raises(ValueError, match=name):
        model.set_equation(lambda: equation(model.Processed_GPs, c))


def test_model_limits_are_refused():
    with pytest.raises(ValueError, match='GPs'):
        embedded.Embedded_GP_Model(*[embedded.GP()] * 9)
    with pytest.raises(ValueError, match='kernel'):
        embedded.Embedded_GP_Model(embedded.GP(), kernel='Matern')
    model, _ = new_model(1, 20, m=2)
    model.set_equation(lambda: model.Processed_GPs[0])
    model.discmtx = np.ones((256, 2), dtype=int)
    with pytest.raises(ValueError, match='parameters'):
        model.full_sample_host(5)
    model.discmtx = np.ones((3, 1), dtype=int)
    with pytest.raises(ValueError, match='columns'):
        model.full_sample_host(5)
    model.inputs = model.inputs * 3
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        model.set_equation(lambda: model.Processed_GPs[0])


@pytest.mark.parametrize('kernel', embedded.KERNELS)
@pytest.mark.parametrize('which', ['identity', 'cstr', 'ratio'])
def test_gradient_against_central_differences(which, kernel):
    model, rng = new_model(3, 200, kernel, m=2, seed=3)
    c = [0.5 + rng.random(200) for _ in range(3)]
    G = model.Processed_GPs
    if which == 'identity':
        eq = lambda: model.Processed_GPs[0] + model.Processed_GPs[1] + model.Processed_GPs[2]
    elif which == 'cstr':
        eq = lambda: -(np.exp(-model.Processed_GPs[0]) * c[0] * c[1] - np.exp(-model.Processed_GPs[1]) * c[2]) + model.Processed_GPs[2]
    else:
        eq = lambda: np.log(np.square(model.Processed_GPs[0]) + 1.5) / (c[0] + model.Processed_GPs[1] ** 2) + \
            (c[1] * model.Processed_GPs[2] + 5.0) ** 1.5 - 1.0 / np.sqrt(c[2])
    model.set_equation(eq)
    model.discmtx = np.array([[1, 0], [0, 2], [1, 1], [3, 0]])
    pot = model.host_potential()
    q = 0.3 * rng.standard_normal(3 * 5 + 1)
    U, grad = pot(q)
    assert np.isfinite(U) and np.isfinite(grad).all()
    for j in range(q.shape[0]):
        h = 1e-5 * max(1.0, abs(q[j]))
        step = np.zeros_like(q)
        step[j] = h
        fd = (pot(q + step)[0] - pot(q - step)[0]) / (2 * h)
        assert abs(fd - grad[j]) <= 1e-6 * max(np.abs(grad).max(), 1.0), (j, fd, grad[j])


def conjugate_model(N=300, seed=4):
    model, rng = new_model(1, N, seed=seed)
    model.data = 1.0 + 0.5 * model.inputs[:, 0] + 0.3 * rng.standard_normal(N)
    model.set_equation(lambda: model.Processed_GPs[0])
    model.discmtx = np.array([[1], [2]])
    return model


def test_identity_equation_recovers_the_ridge_solution_and_rhat():
    model = conjugate_model()
    before = np.random.get_state()
    samples, accepted, U = model.full_sample_host(2000, chains=4, seed=2)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert samples.shape == (4, 2001, 4) and accepted.shape == U.shape == (4, 2001)
    d = model.diagnostics
    assert np.all(d['status'] == embedded.OK) and d['mass_updated'].all() and np.all(d['acceptance_rate'] > 0.2)
    assert d['rhat'].shape == (4,) and np.all(d['rhat'] < 1.05), d['rhat']
    kept = samples[:, 1000:]
    X = embedded.basis_matrix(model._inputs(), model.discmtx, model.phis, model.kernel)
    sigma2 = np.exp(kept[..., -1]).mean()
    ridge = np.linalg.solve(X.T @ X + sigma2 / 1000 * np.eye(3), X.T @ model._data())
    flat = kept.reshape(-1, 4)
    # Monte Carlo standard error from the spread of the four chains' means (autocorrelation included)
    mcse = kept.mean(axis=1).std(axis=0, ddof=1) / np.sqrt(4) + 1e-3 * flat.std(axis=0)
    assert np.all(np.abs(flat[:, :3].mean(axis=0) - ridge) < 4 * mcse[:3] + 0.02 * flat[:, :3].std(axis=0))
    resid = model._data() - X @ ridge
    assert abs(flat[:, 3].mean() - np.log(resid @ resid / 300)) < 4 * mcse[3] + 0.05


def test_adaptation_bookkeeping_on_a_scripted_accept_sequence():
    assert [embedded.adapt_step(1.0, n) for n in (0, 14, 15, 29, 30, 31, 45, 46, 50)] == [0.5, 0.5, 0.8, 0.8, 1.0, 1.2, 1.2, 1.5, 1.5]
    model = conjugate_model(60)
    pot = model.host_potential()
    counts = [10, 20, 30, 40, 50, 0, 0, 0, 3, 1, 25, 50]             # accepted draws per window; 4 in draws 401 .. 500
    script = np.concatenate([np.arange(50) < n for n in counts])
    run = embedded.chain_host(pot, 4, 0, 600, leapfrog=2, seed=1, eps0=1e-3, accept_script=script)
    expected = 1e-3 * np.cumprod([embedded.adapt_step(1.0, n) for n in counts])
    assert np.allclose(run['eps_hist'], expected, rtol=1e-14) and not run['mass_updated'] and np.all(run['inv_mass'] == 1.0)
    assert np.array_equal(run['accepted'][1:], script.astype(np.int32)) and run['eps_final'] == run['eps_hist'][-1]
    counts[9] = 2                                                      # five moved: the mass update fires after draw 500
    script = np.concatenate([np.arange(50) < n for n in counts])
    run = embedded.chain_host(pot, 4, 0, 600, leapfrog=2, seed=1, eps0=1e-3, accept_script=script)
    assert run['mass_updated'] and np.allclose(run['inv_mass'], np.var(run['states'][401:501], axis=0, ddof=1))
    assert np.allclose(run['eps_hist'][:9], expected[:9]) and run['eps_hist'][9] != expected[9]
    assert np.allclose(run['eps_hist'][10:], run['eps_hist'][9] * np.cumprod([embedded.adapt_step(1.0, n) for n in counts[10:]]))


def test_the_capped_step_search_ends_with_no_step():
    model, rng = new_model(1, 40)
    model.set_equation(lambda: np.log(model.Processed_GPs[0] - 1e6))       # not finite at the start, nor anywhere near it
    samples, accepted, U = model.full_sample_host(20, chains=2)
    assert model.diagnostics['status_text'] == ['no step', 'no step']
    assert np.all(samples[:, 0] == 1.0) and np.isnan(samples[:, 1:]).all() and not accepted.any()
    assert np.isnan(model.diagnostics['step_size']).all()


def test_full_routine_host_finds_the_terms_of_a_known_truth():
    rng = np.random.default_rng(8)
    N = 150
    x = rng.random((N, 2))
    phis = getKernels.bernoulli()
    truth = np.array([[1, 0], [1, 1]])
    X = embedded.basis_matrix(x, truth, phis, 'Bernoulli Polynomials')
    c = 0.5 + rng.random(N)
    for tolerance in (0, 1):
        model = embedded.Embedded_GP_Model(embedded.GP(), kernel='Bernoulli Polynomials')
        model.inputs, model.phis = x, phis
        model.data = c * np.exp(X @ np.array([0.2, 1.5, -2.0])) + 0.02 * rng.standard_normal(N)
        model.set_equation(lambda: c * np.exp(model.Processed_GPs[0]))
        samples, mtx, evs = model.full_routine_host(1000, tolerance=tolerance, chains=2, seed=5)
        rows = {tuple(r) for r in mtx.tolist()}
        assert {(1, 0), (1, 1)} <= rows, mtx
        assert samples.shape == (2, 1001, mtx.shape[0] + 2) and np.array_equal(model.mtx, mtx)
        # the stop rule: the run ends at the first sub-stage that does not improve on the best so far (for tolerance 0 and
        # 1 alike: the reference's counter starts at 1), and the returned model is the best one
        assert len(evs) >= 2 and evs[-1] >= evs[:-1].min()
        assert all(evs[i] < evs[:i].min() for i in range(1, len(evs) - 1))
        best = int(np.argmin(evs))
        assert mtx.shape[0] == [2, 3, 5, 7, 9, 11, 13][best]

"""The systems tests/test_control_host.py and tests/test_control_gpu.py share (no tests here)."""
import numpy as np

from assimilate_cases import BERN, model


def mixed(E, steps, seed=11, h=0.05, spread=0.1):
    """d T/dt is a cubic-spline model of (T, c, u) with a two-way term T x u, d c/dt a Bernoulli model of (T, c, d) with a
    two-way term; u is the control, d a forcing column."""
    rng = np.random.default_rng(seed)
    first = model('s', [0.05, -0.6, 0.3, 0.4, 0.25], [[1, 0, 0], [0, 2, 0], [0, 0, 1], [1, 0, 2]],
                  [[-2.0, 2.0], [-2.0, 2.0], [0.0, 10.0]], E, rng, spread)
    second = model('b', [-0.02, 0.4, -0.5, 0.1, 0.2], [[1, 0, 0], [0, 1, 0], [2, 1, 0], [0, 0, 2]],
                   [[-2.5, 2.5], [-2.0, 2.0], [-1.0, 3.0]], E, rng, spread)
    d = 1.0 + 0.8 * np.sin(np.arange(steps + 3) / 2.0)
    return dict(models=[first, second], states=['T', 'c'], inputs=[['T', 'c', 'u'], ['T', 'c', 'd']], controls=['u'],
                forcing={'d': d}, y0=[0.3, -0.2], t=(0.0, (steps - 0.5) * h, h))


def linear(E, steps, n_controls=1, seed=13, h=0.1, spread=0.0):
    """Order-1 Bernoulli terms only (B1 is linear): with idle clamps the trajectory is affine in the controls.
    d x0/dt reads (x0, x1, u0), d x1/dt reads (x0, x1, u1 or u0)."""
    rng = np.random.default_rng(seed)
    second = 'u1' if n_controls == 2 else 'u0'
    a = model('b', [0.1, -0.8, 0.3, 1.2], np.eye(3, dtype=int), [[-4.0, 4.0], [-4.0, 4.0], [-1.0, 1.0]], E, rng, spread)
    b = model('b', [-0.05, 0.4, -0.6, 0.7], np.eye(3, dtype=int), [[-4.0, 4.0], [-4.0, 4.0], [-1.0, 1.0]], E, rng, spread)
    return dict(models=[a, b], states=['x0', 'x1'], inputs=[['x0', 'x1', 'u0'], ['x0', 'x1', second]],
                controls=['u0', 'u1'][:n_controls], y0=[0.2, -0.1], t=(0.0, (steps - 0.5) * h, h))


def product(E, steps, seed=17, h=0.05, spread=0.1):
    """Two states with a product term x0 x1 and a product x1 u, Bernoulli."""
    rng = np.random.default_rng(seed)
    a = model('b', [0.05, -0.5, 0.6, 0.8], [[1, 0, 0], [1, 1, 0], [0, 0, 1]], [[-2.0, 2.0], [-2.0, 2.0], [0.0, 4.0]], E, rng, spread)
    b = model('b', [-0.1, 0.3, -0.7, 0.5], [[1, 0, 0], [0, 2, 0], [0, 1, 2]], [[-2.0, 2.0], [-2.0, 2.0], [0.0, 4.0]], E, rng, spread)
    return dict(models=[a, b], states=['x0', 'x1'], inputs=[['x0', 'x1', 'u'], ['x0', 'x1', 'u']], controls=['u'],
                y0=[0.4, -0.3], t=(0.0, (steps - 0.5) * h, h))


def chain(n_states, E, steps, seed=19, h=0.05):
    """n_states models, state k reading (x_k, x_(k+1), u), kernels alternating, one term per column and their product."""
    rng = np.random.default_rng(seed)
    names = [f'x{k}' for k in range(n_states)]
    models, inputs = [], []
    for k in range(n_states):
        cols = [names[k]] + ([names[(k + 1) % n_states]] if n_states > 1 else []) + ['u']
        m = len(cols)
        mtx = np.concatenate([np.diag(rng.choice([1, 2, 3], size=m)), np.ones((1, m), dtype=int)])
        minmax = [[0.0, 10.0] if name == 'u' else [-1.0 - 0.125 * k, 1.0 + 0.25 * k] for name in cols]
        models.append(model('bs'[k % 2], 0.3 * rng.standard_normal(m + 2), mtx, minmax, E, rng))
        inputs.append(cols)
    return dict(models=models, states=names, inputs=inputs, controls=['u'], y0=rng.uniform(-0.4, 0.4, n_states),
                t=(0.0, (steps - 0.5) * h, h))


__all__ = ['BERN', 'mixed', 'linear', 'product', 'chain']

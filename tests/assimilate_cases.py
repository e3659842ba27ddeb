"""The systems tests/test_assimilate_host.py and tests/test_assimilate_gpu.py share (no tests here)."""
import os
from fractions import Fraction

import numpy as np

from helpers import GOLDEN
from fokl_gpy_amd import getKernels

BERN = getKernels.bernoulli()
SPLINES = getKernels.table_to_phis(np.load(os.path.join(GOLDEN, 'spline_phis.npz'))['table'])
KERNELS = {'b': ('Bernoulli Polynomials', BERN), 's': ('Cubic Splines', SPLINES)}


def model(kind, mean, mtx, minmax, E, rng, spread=0.1):
    mean = np.asarray(mean, dtype=np.float64)
    kernel, phis = KERNELS[kind]
    return dict(betas=mean * (1 + spread * rng.standard_normal((E, mean.shape[0]))), mtx=np.asarray(mtx, dtype=int), phis=phis,
                minmax=minmax, kernel=kernel)


def two_state(E, steps, seed=5, h=0.05):
    """d T/dt is a cubic-spline model of (T, c, u), d c/dt a Bernoulli model of (T, c); u is forcing."""
    rng = np.random.default_rng(seed)
    first = model('s', [0.05, -0.6, 0.3, 0.2], [[1, 0, 0], [0, 2, 0], [1, 0, 1]], [[-2.0, 2.0], [-2.0, 2.0], [0.0, 10.0]], E, rng)
    second = model('b', [-0.02, 0.4, -0.5, 0.1], [[1, 0], [0, 1], [2, 1]], [[-2.5, 2.5], [-2.0, 2.0]], E, rng)
    u = 5.0 + 4.0 * np.sin(np.arange(steps + 3) / 3.0)
    return dict(models=[first, second], states=['T', 'c'], inputs=[['T', 'c', 'u'], ['T', 'c']], forcing={'u': u},
                y0=[0.3, -0.2], t=(0.0, (steps - 0.5) * h, h))


def one_term_models(n_states, E, seed=7):
    """n_states models of one order-1 Bernoulli term each, state k reading state k."""
    rng = np.random.default_rng(seed)
    names = [f'x{k}' for k in range(n_states)]
    models = [model('b', [0.1 - 0.03 * k, -0.4], [[1]], [[-1.0 - 0.125 * k, 1.0 + 0.25 * k]], E, rng) for k in range(n_states)]
    return dict(models=models, states=names, inputs=[[name] for name in names], y0=np.linspace(-0.3, 0.4, n_states))


def wide_system(E, seed=9, n_states=4, n_terms=92):
    """n_states Bernoulli models of n_terms terms each over all the states: more coefficients than ``simulate`` holds per
    member, few enough for ``assimilate``, which holds them once."""
    rng = np.random.default_rng(seed)
    names = [f'x{k}' for k in range(n_states)]
    models = []
    for k in range(n_states):
        mtx = rng.integers(0, 4, size=(n_terms, n_states))
        mtx[np.arange(n_terms), rng.integers(0, n_states, n_terms)] += 1          # no empty row
        mean = np.concatenate([[0.02 * (k - 1.5)], 0.02 * rng.standard_normal(n_terms)])
        models.append(model('b', mean, mtx, [[-1.0, 1.0 + 0.125 * j] for j in range(n_states)], E, rng))
    return dict(models=models, states=names, inputs=[names] * n_states, y0=np.linspace(-0.2, 0.3, n_states))


def linear_model(E):
    """tests/test_simulate_host.py's linear system, dy/dt = a + b y with a = 1, b = -0.5 on [0, 4], as E equal rows; also
    the RK4 step y <- A y + c in closed form, from the very doubles the model holds."""
    lo, hi, h = 0.0, 4.0, 0.0625
    c0, c1 = (float(v) for v in BERN[0])
    beta1 = -2.0 / c1
    beta0 = 1.0 - beta1 * c0
    F = Fraction
    b = F(beta1) * F(c1) / (F(hi) - F(lo))
    a = F(beta0) + F(beta1) * (F(c0) - F(c1) * F(lo) / (F(hi) - F(lo)))
    z = b * F(h)
    R = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
    one = dict(betas=np.tile([[beta0, beta1]], (E, 1)), mtx=np.array([[1]]), phis=BERN, minmax=[[lo, hi]],
               kernel='Bernoulli Polynomials')
    return one, h, float(R), float((R - 1) * a / b)

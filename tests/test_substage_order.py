"""The order in which the native sub-stage loop (csrc/fokl_run.cpp) sends a sub-stage's model out, read from the clock stamps
it reports (fit_stats['substage_order']): K1 of the coming sub-stage in front of the wait for the model's eigenpairs; once
they are there the chain first, K3 behind it, the coming sub-stage's Gram rows behind K3.  The order changes no result: the
fit equals the Python loop's and its own repetition bit for bit, and a residual launch that fails in the middle (an outcome
exists by then, a residual pass may be in flight, columns are built ahead) leaves the backend fit for the next fit."""
import contextlib
import os
import warnings

import numpy as np
import pytest

from helpers import OracleBackend
from fokl_gpy_amd import FoKLRoutines
from oracle import fokl_oracle as O


def _problem():
    rng = np.random.default_rng(11)
    x = rng.random((20000, 3))
    y = np.sin(4 * x[:, 0]) + x[:, 1] * x[:, 2] + 0.3 * x[:, 2] ** 2 + 0.05 * rng.standard_normal(x.shape[0])
    return x, y


@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fit(loop, backend=None):
    """-> (model, betas, mtx, evs, end state of numpy's stream); backend None: the device"""
    x, y = _problem()
    with _env(FOKL_SUBSTAGE_LOOP=loop, FOKL_SEARCH='native'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = FoKLRoutines.FoKL(kernel='Bernoulli Polynomials', burnin=50, draws=50, UserWarnings=False, ConsoleOutput=False)
        if backend is not None:
            model._backend_override = backend
        np.random.seed(2024)
        betas, mtx, evs = model.fit(x, y, clean=True)
    st = np.random.get_state()
    return model, betas, mtx, evs, (st[1].copy(), st[2], st[3], st[4])


def _same_bits(a, b):
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[4][0], b[4][0]) and a[4][1:] == b[4][1:]


def _check_order(model):
    assert model.fit_stats.get('substage_loop') == 'native'
    order = model.fit_stats['substage_order']
    assert len(order) == model.fit_stats['substages'] and len(order) >= 3
    for row in order:
        # (the stop rule ends this search long before the patterns run out: every sub-stage has a coming one)
        assert row['k1_ahead'] is not None and row['ahead_gram_launched'] is not None
        assert row['k1_ahead'] <= row['g2_wait_begun'] <= row['g2_arrived']
        assert row['g2_arrived'] <= row['chain_submitted'] <= row['k3_launched'] <= row['ahead_gram_launched']
        # (the first tests' orders: from a G2 that was there before the sub-stage began, else behind the chain's start)
        placed = row['orders_placed']
        assert placed is None or placed <= row['g2_wait_begun'] or placed >= row['chain_submitted']
    firsts = [row['g2_wait_begun'] for row in order]
    assert firsts == sorted(firsts)


_HOST = {}


def _host_fits():
    if not _HOST:
        _HOST['native'] = _fit('native', OracleBackend())
        _HOST['again'] = _fit('native', OracleBackend())
        _HOST['python'] = _fit('python', OracleBackend())
    return _HOST


def test_the_chain_starts_before_the_launches_and_k1_before_the_wait():
    _check_order(_host_fits()['native'][0])


def test_the_native_loop_equals_the_python_loop_bit_for_bit():
    fits = _host_fits()
    assert fits['python'][0].fit_stats.get('substage_loop') != 'native'
    _same_bits(fits['native'], fits['python'])
    a, b = fits['native'][0], fits['python'][0]
    assert [(t['cols'], t['built'], t['kill']) for t in a.fit_trace] == [(t['cols'], t['built'], t['kill']) for t in b.fit_trace]
    assert np.array_equal([t['ev'] for t in a.fit_trace], [t['ev'] for t in b.fit_trace])


def test_a_second_run_equals_the_first_bit_for_bit():
    fits = _host_fits()
    _same_bits(fits['native'], fits['again'])


class MatrixFreeStandIn(OracleBackend):
    """The stand-in with a matrix-free residual pass (K3 from the terms, not from stored columns), which the native loop then
    takes for every two-way Bernoulli model; fail_at: that call of it raises."""

    def __init__(self, fail_at=None):
        super().__init__()
        self.fail_at = fail_at
        self.terms_calls = 0

    def resid_terms_supported(self, terms):
        return bool(np.all(np.count_nonzero(terms, axis=1) <= 2))

    def bic_resid_terms_launch(self, terms, betahat):
        self.terms_calls += 1
        if self.terms_calls == self.fail_at:
            raise RuntimeError('residual launch refused')
        X = O.build_columns_c(self.xsm, self.phind, self.phis, self.kernel, np.atleast_2d(terms))
        r = self.cols[1] - betahat[0] - X @ np.reshape(betahat[1:], -1)
        return float(np.sum(r)), float(np.sum(r * r))


def test_a_failing_residual_launch_leaves_the_backend_fit_for_the_next_fit():
    first = MatrixFreeStandIn()
    clean = _fit('native', first)
    assert clean[0].fit_stats['resid_matrix_free'] == first.terms_calls >= 4
    backend = MatrixFreeStandIn(fail_at=3)
    with pytest.raises(RuntimeError, match='residual launch refused'):
        _fit('native', backend)
    assert backend.terms_calls == 3
    after = _fit('native', backend)                          # the same backend: nothing of the failed search is in its way
    assert backend.terms_calls > 3
    _same_bits(clean, after)
    _check_order(after[0])


@pytest.mark.gpu
def test_the_order_and_the_bits_on_the_device():
    native = _fit('native')
    _check_order(native[0])
    _same_bits(native, _fit('python'))

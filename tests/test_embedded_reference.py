"""The extended-precision reference the device's edge tests compare against (tests/embedded_reference.py) is guarded here,
without a device: a central difference of its own U against its forward-mode gradient on EVERY tape those tests use, and
the statement (float64, reverse mode) against it."""
import numpy as np
import pytest

import embedded_reference as R
from fokl_gpy_amd import embedded


def every_tape():
    """(tape, rows, coefficients per GP) of tests/test_embedded_edges_gpu.py"""
    cases = [(R.chain_tape(K, n_ops), N, P) for K, n_ops in ((3, 31), (3, 32), (8, 26), (8, 27)) for N, P in ((65, 2), (129, 11))]
    cases += [(R.chain_tape(1, 9), 130, 256), (R.chain_tape(3, 32), 130, 85)]
    for tape in R.semantic_tapes():
        cases += [(tape, 130, 3), (tape.padded(), 130, 3)]
    cases.append((R.RawTape('no operation, two GPs, the result is GP 1', 2).done(R.S(1)), 130, 3))
    return cases


def test_longdouble_is_wider_than_double():
    assert np.finfo(R.L).eps < 1e-18


def test_the_reference_agrees_with_its_own_central_difference_on_every_tape():
    """h = 1e-6: truncation ~1e-12; the bound is 1e-8 of the gradient's largest component (reference_self_check)."""
    for tape, N, P in every_tape():
        problem = R.Problem(N, P)
        D = tape.n_gps * P + 1
        q = 0.3 * np.random.default_rng(D).standard_normal(D)
        if D > 100:                                     # the widest vectors: every 9th coefficient and ln sigma^2
            keep = np.append(np.arange(0, D - 1, 9), D - 1)
            X = problem.X
            U, grad, _, _ = R.reference_potential(q, X, tape, problem.columns, problem.data)
            worst = 0.0
            for j in keep:
                step = np.zeros(D, dtype=R.L)
                step[j] = R.L(1e-6)
                fd = (R.reference_potential(q.astype(R.L) + step, X, tape, problem.columns, problem.data)[0] -
                      R.reference_potential(q.astype(R.L) - step, X, tape, problem.columns, problem.data)[0]) / (2 * R.L(1e-6))
                worst = max(worst, float(abs(fd - grad[j])))
            error = worst / float(np.max(np.abs(grad)))
        else:
            error = R.reference_self_check(q, problem.X, tape, problem.columns, problem.data)
        assert error <= 1e-8, (tape.name, error)


def test_the_statement_agrees_with_the_reference_on_every_tape():
    """float64 and a reverse sweep against longdouble and tangents, at the bound the device is held to."""
    for tape, N, P in every_tape():
        problem = R.Problem(N, P)
        D = tape.n_gps * P + 1
        q = 0.3 * np.random.default_rng(D).standard_normal(D)
        U, grad, e, drdg = R.reference_potential(q, problem.X, tape, problem.columns, problem.data)
        host_U, host_grad = embedded.potential(q, problem.X, tape.host_tape(problem.columns), problem.data)
        scale_U, scale_g = R.term_scales(q, problem.X, e, drdg)
        assert abs(host_U - float(U)) <= 1e-11 * scale_U, tape.name
        assert np.all(np.abs(host_grad - grad.astype(np.float64)) <= 1e-11 * scale_g + 1e-300), tape.name


def test_dead_operations_and_an_unread_gp_have_no_derivative():
    problem = R.Problem(130, 3)
    q = 0.3 * np.random.default_rng(1).standard_normal(10)
    for tape in R.semantic_tapes():
        short = R.reference_potential(q, problem.X, tape, problem.columns, problem.data)
        padded = R.reference_potential(q, problem.X, tape.padded(), problem.columns, problem.data)
        assert short[0] == padded[0] and np.array_equal(short[1], padded[1]), tape.name
        if tape.name == 'a GP that no operation reads':
            assert np.array_equal(short[1][3:6].astype(np.float64), (q[3:6].astype(R.L) / 1000).astype(np.float64))

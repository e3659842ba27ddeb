"""hmc_chain_kernel at its edges: both launch plans (256 and 128 threads) at the slot count where they switch, every
(opcode, operand kind, position) of the tape interpreter against an extended-precision forward-mode reference
(tests/embedded_reference.py), the step search on its own, the loop edges and the chains that find no step.

Every decision a comparison depends on (an accept, a doubling or halving of the step search) is shown to be at least 1e-6
from its threshold in the HOST run, inside the test; the device's sums differ from the host's by rounding only."""
import numpy as np
import pytest

import embedded_reference as R
from fokl_gpy_amd import embedded

pytestmark = pytest.mark.gpu

LN2 = np.log(2.0)
ROWS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
COEFS = (1, 2, 11)


def starts(chains, D, seed):
    return 0.3 * np.random.default_rng(seed).standard_normal((chains, D))


def assert_plan(ctx, tape, threads):
    """the instantiation a launch of this tape runs, and its LDS request against the layout recomputed here"""
    n_ops = len(tape.ops)
    plan = ctx.embedded_plan(tape.n_gps, n_ops)
    assert plan['threads'] == threads, (tape.name, plan)
    assert plan['lds_bytes'] == R.lds_bytes(tape.n_gps + n_ops, n_ops, threads) <= R.LDS_BUDGET, (tape.name, plan)


@pytest.mark.parametrize('K,n_ops,threads', [(3, 31, 256), (3, 32, 128), (8, 26, 256), (8, 27, 128)])
def test_both_plans_at_the_slot_count_where_they_switch(device_ctx, K, n_ops, threads):
    tape = R.chain_tape(K, n_ops)
    assert tape.n_slots == R.SWITCH_SLOTS + (threads == R.NARROW)
    assert_plan(device_ctx, tape, threads)
    assert R.lds_bytes(tape.n_slots, n_ops, R.WIDE) > R.LDS_BUDGET or threads == R.WIDE      # 128 only where 256 does not fit
    for N in ROWS:
        for P in COEFS:
            problem = R.Problem(N, P)
            q0 = starts(3, K * P + 1, K + P + N)
            dev = problem.launch(device_ctx, tape, q0, eps0=0.1, want_grad0=True)
            R.assert_device_matches_reference(dev, q0, problem, tape, (tape.name, N, P))


@pytest.mark.parametrize('K,P,n_ops,threads', [(1, 256, 9, 256), (3, 85, 32, 128)])
def test_the_widest_parameter_vector_of_each_plan(device_ctx, K, P, n_ops, threads):
    tape = R.chain_tape(K, n_ops)
    assert_plan(device_ctx, tape, threads)
    problem = R.Problem(130, P, kernel='Cubic Splines' if K == 1 else 'Bernoulli Polynomials')
    q0 = starts(3, K * P + 1, P)
    assert q0.shape[1] in (256, 257)
    dev = problem.launch(device_ctx, tape, q0, eps0=0.1, want_grad0=True)
    R.assert_device_matches_reference(dev, q0, problem, tape, tape.name)


@pytest.mark.parametrize('threads', [256, 128])
def test_every_opcode_operand_kind_and_position(device_ctx, threads):
    """Short tapes run under 256 threads; behind each, dead operations up to 35 slots bring it under 128."""
    problem = R.Problem(130, 3)
    q0 = starts(3, 3 * 3 + 1, 7)
    tapes = R.semantic_tapes()
    assert len({t.name for t in tapes}) == len(tapes)
    for tape in tapes:
        tape = tape if threads == R.WIDE else tape.padded()
        assert_plan(device_ctx, tape, threads)
        dev = problem.launch(device_ctx, tape, q0, eps0=0.1, want_grad0=True)
        R.assert_device_matches_reference(dev, q0, problem, tape, tape.name)
    if threads == R.WIDE:
        tape = R.RawTape('no operation, two GPs, the result is GP 1', 2).done(R.S(1))
        assert_plan(device_ctx, tape, R.WIDE)
        q2 = starts(3, 2 * 3 + 1, 8)
        dev = problem.launch(device_ctx, tape, q2, eps0=0.1, want_grad0=True)
        R.assert_device_matches_reference(dev, q2, problem, tape, tape.name)
        assert np.array_equal(dev['grad0'][:, :3], q2[:, :3] / 1000.0)             # GP 0: the prior's gradient alone


def narrow_model(device_ctx, K, T, N, kernel='Bernoulli Polynomials'):
    model = R.traced_model('wide', K, T, N, kernel)
    assert device_ctx.embedded_plan(K, len(model.tape.ops))['threads'] == R.NARROW
    return model, K * (T + 1) + 1


def test_one_transition_equals_the_statement_under_128_threads(device_ctx):
    for K, T, N in ((8, 5, 257), (3, 3, 129)):
        model, D = narrow_model(device_ctx, K, T, N, 'Cubic Splines')
        q0 = starts(6, D, 5)
        dev = R.launch_model(device_ctx, model, 6, 1, q0=q0, eps0=1e-5, adapt=False, seed=11, want_proposal=True)
        pot = model.host_potential()
        for c in range(6):
            host = embedded.chain_host(pot, D, c, 1, 20, 11, q0[c], 1e-5, False)
            assert R.accept_margins(pot, host, c, 20, 11, 1e-5).min() >= 1e-6
            scale = max(1.0, abs(host['proposal'][-1]))
            assert np.max(np.abs(dev['proposal'][c, :-1] - host['proposal'][:-1])) < 1e-9
            assert abs(dev['proposal'][c, -1] - host['proposal'][-1]) < 1e-9 * scale
            assert dev['accepted'][c, 1] == host['accepted'][1]
            assert np.max(np.abs(dev['states'][c, 1] - host['states'][1])) < 1e-9


def test_chains_under_128_threads_follow_the_statement_and_do_not_depend_on_the_grid(device_ctx):
    model, D = narrow_model(device_ctx, 8, 3, 300)
    q0 = np.tile(0.2 * np.random.default_rng(9).standard_normal(D), (64, 1))
    few = R.launch_model(device_ctx, model, 8, 60, q0=q0[:8], eps0=1e-2, adapt=False, seed=3)
    many = R.launch_model(device_ctx, model, 64, 60, q0=q0, eps0=1e-2, adapt=False, seed=3)
    for key in ('states', 'potential', 'accepted'):
        assert np.array_equal(few[key][3], many[key][3]), key                 # bitwise: chain 3 of 8 is chain 3 of 64
    assert not np.array_equal(many['states'][3], many['states'][4])
    pot = model.host_potential()
    compared = 0
    for c in range(4):
        host = embedded.chain_host(pot, D, c, 60, 20, 3, q0[c], 1e-2, False)
        assert R.accept_margins(pot, host, c, 20, 3, 1e-2).min() >= 1e-6         # the seed's decisions are not marginal
        if np.array_equal(host['accepted'], few['accepted'][c]):
            compared += 1
            assert np.max(np.abs(host['states'] - few['states'][c])) < 1e-7
            assert host['accepted'].sum() > 5
    assert compared >= 3


@pytest.mark.parametrize('leapfrog', [1, 2])
def test_the_last_leapfrog_step_is_the_only_or_the_second(device_ctx, leapfrog):
    """leapfrog = 1: the only step is the last one and gets the half kick.  The last kick reaches nothing but the final
    kinetic energy, so it shows in the accept decisions alone: at this step every one of the 20 chains accepts, and a full
    kick in place of the half one would reject 14 of them."""
    model = R.traced_model('cstr', 2, 4, 257)
    D, chains, eps = 2 * 5 + 1, 20, 1e-2
    q0 = starts(chains, D, 5)
    dev = R.launch_model(device_ctx, model, chains, 1, q0=q0, eps0=eps, adapt=False, seed=11, leapfrog=leapfrog,
                         want_proposal=True)
    pot = model.host_potential()
    for c in range(chains):
        host = embedded.chain_host(pot, D, c, 1, leapfrog, 11, q0[c], eps, False)
        assert R.accept_margins(pot, host, c, leapfrog, 11, eps).min() >= 1e-6
        scale = max(1.0, abs(host['proposal'][-1]))
        assert np.max(np.abs(dev['proposal'][c, :-1] - host['proposal'][:-1])) < 1e-9
        assert abs(dev['proposal'][c, -1] - host['proposal'][-1]) < 1e-9 * scale
        assert dev['accepted'][c, 1] == host['accepted'][1] == 1
        assert np.max(np.abs(dev['states'][c, 1] - host['states'][1])) < 1e-9
        assert abs(dev['potential'][c, 1] - host['potential'][1]) < 1e-9 * scale


@pytest.mark.parametrize('eps0,factors', [(2e-3, {1.5}), (0.1, {1.2, 1.5}), (0.15, {0.5})])
@pytest.mark.parametrize('draws', [49, 50, 51])
def test_draws_around_the_first_window(device_ctx, draws, eps0, factors):
    """49, 50 and 51 draws: no window, one window that ends the chain, one window and a draw with the adapted step; the
    three first steps have every draw accepted, most of them, and none."""
    model = R.traced_model('cstr', 2, 3, 200)
    D, chains, leapfrog = 2 * 4 + 1, 4, 5
    q0 = np.tile(0.2 * np.random.default_rng(9).standard_normal(D), (chains, 1))
    dev = R.launch_model(device_ctx, model, chains, draws, q0=q0, eps0=eps0, adapt=True, seed=3, leapfrog=leapfrog)
    assert dev['eps_hist'].shape == (chains, draws // 50)
    assert np.all(dev['status'] == embedded.OK) and not dev['mass_updated'].any()
    pot = model.host_potential()
    seen = set()
    for c in range(chains):
        host = embedded.chain_host(pot, D, c, draws, leapfrog, 3, q0[c], eps0, True)
        steps = np.full(draws, eps0)
        if draws > 50:
            steps[50:] = host['eps_hist'][0]
        assert R.accept_margins(pot, host, c, leapfrog, 3, steps).min() >= 1e-6
        assert np.array_equal(dev['accepted'][c], host['accepted'])
        assert np.max(np.abs(dev['states'][c] - host['states'])) < 1e-7
        after = embedded.adapt_step(eps0, host['accepted'][1:51].sum()) if draws >= 50 else eps0
        if draws >= 50:
            assert dev['eps_hist'][c, 0] == host['eps_hist'][0] == after
            seen.add(round(after / eps0, 6))
        assert dev['eps_final'][c] == host['eps_final'] == after
    assert draws < 50 or seen == factors


def search_problems():
    """(name, model, q0 [chains, D], what the host run must show): a flat potential (one row, a wide noise variance: the
    step doubles), a stiff one (600 rows, sigma^2 = exp(-6): it halves), and rate terms under that variance, whose first
    trial points overflow (the step is halved until they are finite, then further)."""
    flat = R.traced_model('identity', 1, 1, 1, data=lambda x, rng: np.zeros(1))
    q_flat = 1e-3 * np.random.default_rng(1).standard_normal((4, 3))
    q_flat[:, -1] = 3.0
    stiff = R.traced_model('identity', 1, 2, 600)
    q_stiff = starts(4, 4, 2)
    q_stiff[:, -1] = -6.0
    rates = R.traced_model('cstr', 2, 3, 600)
    q_rates = starts(4, 9, 2)
    q_rates[:, -1] = -6.0
    return (('flat', flat, q_flat, lambda eps, nonfinite: np.all(eps >= 2.0) and not nonfinite.any()),
            ('stiff', stiff, q_stiff, lambda eps, nonfinite: np.all(eps <= 2.0 ** -6) and not nonfinite.any()),
            ('overflow', rates, q_rates, lambda eps, nonfinite: np.all(eps <= 2.0 ** -6) and (nonfinite >= 2).sum() >= 2))


@pytest.mark.parametrize('which', [0, 1, 2])
def test_the_step_search_alone(device_ctx, which):
    """draws = 0 and eps0 = 0: eps_final is the search's result, a power of two -- the host's, bit for bit."""
    name, model, q0, expected = search_problems()[which]
    pot = model.host_potential()
    traces = [R.step_search_trace(pot, q0[c], 5, c) for c in range(q0.shape[0])]
    for eps, logs, nonfinite, largest in traces:
        assert eps > 0.0 and np.log2(eps) == np.round(np.log2(eps))
        assert np.min(np.abs(logs + LN2)) >= 1e-6                                   # no decision is marginal
        assert largest < 1e150                                                      # and no finite trial is near overflow
    assert expected(np.array([t[0] for t in traces]), np.array([t[2] for t in traces])), name
    dev = R.launch_model(device_ctx, model, q0.shape[0], 0, q0=q0, eps0=0.0, seed=5)
    assert np.all(dev['status'] == embedded.OK)
    assert np.array_equal(dev['eps_final'], np.array([t[0] for t in traces])), (name, dev['eps_final'])
    assert dev['states'].shape == (q0.shape[0], 1, q0.shape[1]) and np.array_equal(dev['states'][:, 0], q0)


def test_chains_without_a_step_end_as_the_statement_says_and_leave_their_neighbours_alone(device_ctx):
    """log(G0) with a constant GP of +2 (finite) or -2 (never finite): the step search of a bad start halves 61 times and
    gives up.  NaN arithmetic is ordinary arithmetic."""
    model = R.traced_model('log', 1, 2, 100)
    D, draws = 4, 60
    good, bad = np.array([2.0, 0.0, 0.0, 0.0]), np.array([-2.0, 0.0, 0.0, 0.0])
    mixed = np.array([good, bad, good, bad, good, bad])
    kw = dict(seed=7, want_proposal=True, want_grad0=True)
    dev = R.launch_model(device_ctx, model, 6, draws, q0=mixed, **kw)
    alone = R.launch_model(device_ctx, model, 6, draws, q0=np.tile(good, (6, 1)), **kw)
    pot = model.host_potential()
    for c in (1, 3, 5):
        host = embedded.chain_host(pot, D, c, draws, 20, 7, mixed[c])
        assert host['status'] == embedded.NO_STEP and dev['status'][c] == embedded.NO_STEP
        assert np.array_equal(dev['states'][c, 0], mixed[c])
        for key in ('states', 'potential', 'eps_hist', 'proposal', 'accepted', 'inv_mass'):
            assert np.array_equal(dev[key][c], host[key], equal_nan=True), (key, c)
        assert np.isnan(dev['states'][c, 1:]).all() and np.isnan(dev['potential'][c, 1:]).all()
        assert np.isnan(dev['eps_hist'][c]).all() and dev['eps_hist'].shape == (6, 1) and np.isnan(dev['proposal'][c]).all()
        assert np.isnan(dev['eps_final'][c]) and np.isnan(host['eps_final'])
        assert not dev['accepted'][c].any() and np.all(dev['inv_mass'][c] == 1.0) and not dev['mass_updated'][c]
    for c in (0, 2, 4):
        host = embedded.chain_host(pot, D, c, draws, 20, 7, mixed[c])
        assert host['status'] == embedded.OK and dev['status'][c] == embedded.OK
        for key in dev:
            assert dev[key][c].tobytes() == alone[key][c].tobytes(), (key, c)     # bitwise: the neighbours changed nothing
        assert np.isfinite(dev['states'][c]).all() and np.isfinite(dev['eps_final'][c])
    assert dev['accepted'][0].sum() > 5                                            # a good chain moves

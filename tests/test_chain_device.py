"""
G3 on the device (include/fokl_hip.h: fokl_dchain_*): the finishing of the polar normals and the Gibbs recursion of
FR:1519-1548 on the GPU against the host chain (fokl_gibbs_chain_from_tape, itself pinned bit for bit to the
reference's loop and numpy's stream in tests/test_sampler_host.py) on the same noise tapes.

Tolerances: with FOKL_DCHAIN_RECURSION=exact a tape whose normals were finished on the host goes through the device
recursion BIT FOR BIT (same IEEE operations in the same order, the quadratic forms summed in the host's order); with the
finishing on the device the normals differ from libm's in the last bit of log(), and the default recursion folds its
reciprocals (three long operations on the critical path instead of nine), each fold a rounding or two away from the
host's: both reach the draws at the 1e-16 .. 1e-15 level.  Round 6's recursion forms bstar as
b + (dtd - sum d qty^2 + sigma^2 sum v^2) / 2 -- two of its three sums off the critical path -- where the host forms
b + (w'Lw - 2 w'qty + dtd + w'w / tau^2) / 2: the same cancellation against dtd reached through different roundings, a
digit's worth on models whose fit is nearly exact.  Bounded here by TOL = 1e-12 of the column scale over the full 2000
iterations of a fit's chain (the reference's draws are held to 1e-9, tests/test_config_goldens.py).

The segmented recursion (gibbs_chain_segments_kernel: eight pieces on eight wavefronts, 64 warm-up iterations each, the cut
checked to 1e-14, a chain that fails the check run again in one piece) has a reference stricter than the host chain: the
SAME statement on one wavefront (FOKL_DCHAIN_RECURSION=serial when the engine is created).  A chain that took the fallback
must equal it bit for bit -- draws, means, end state -- and says so in ``DeviceChainJob.bad_cut`` and the engine's ``recuts``
counter; a chain whose cut held agrees with it to the check's tolerance.  The host twin (fokl_gibbs_chain_segments_host,
tests/test_chain_segments_host.py) must take the same decision on the same chain.
"""
import os

import numpy as np
import pytest

from helpers import slow_chain_case
from fokl_gpy_amd import _capi

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope='module')
def engine():
    """The default engine: the recursion with its reciprocals folded (three long operations on the critical path)."""
    eng = _capi.DeviceChainEngine(int(os.environ.get('FOKL_DEVICE', '0')), slots=8)
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def exact_engine():
    """FOKL_DCHAIN_RECURSION=exact: the host chain's operations in the host chain's order."""
    saved = os.environ.get('FOKL_DCHAIN_RECURSION')
    os.environ['FOKL_DCHAIN_RECURSION'] = 'exact'
    try:
        eng = _capi.DeviceChainEngine(int(os.environ.get('FOKL_DEVICE', '0')), slots=8)
    finally:
        if saved is None:
            del os.environ['FOKL_DCHAIN_RECURSION']
        else:
            os.environ['FOKL_DCHAIN_RECURSION'] = saved
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def serial_engine():
    """FOKL_DCHAIN_RECURSION=serial: the default (fast) statement on one wavefront from start to end -- what the segmented
    kernel's fallback must reproduce bit for bit."""
    saved = os.environ.get('FOKL_DCHAIN_RECURSION')
    os.environ['FOKL_DCHAIN_RECURSION'] = 'serial'
    try:
        eng = _capi.DeviceChainEngine(int(os.environ.get('FOKL_DEVICE', '0')), slots=8)
    finally:
        if saved is None:
            del os.environ['FOKL_DCHAIN_RECURSION']
        else:
            os.environ['FOKL_DCHAIN_RECURSION'] = saved
    yield eng
    eng.close()


def model(p1, rng):
    lamb = np.sort(rng.random(p1) * 1e5 + 1e-2)
    lamb[0] = 3e-3
    qty = rng.standard_normal(p1) * np.sqrt(lamb) * 3
    return lamb, qty


def host_tape(p1, draws, seed, exact=True):
    np.random.seed(seed)
    stream = _capi.LegacyStream()
    return _capi.noise_tape(p1, draws, 500.0 + p1 / 2, 4 + (p1 - 1) / 2, stream)


@pytest.mark.parametrize('which', ['fast', 'exact'])
@pytest.mark.parametrize('p1', [1, 2, 7, 17, 60, 64, 65, 129, 200, 586])
def test_device_chain_equals_the_host_chain_on_the_same_tape(engine, exact_engine, which, p1, monkeypatch):
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    engine = engine if which == 'fast' else exact_engine
    rng = np.random.default_rng(p1)
    draws = 300 if p1 > 200 else 2000
    lamb, qty = model(p1, rng)
    tape = host_tape(p1, draws, 10 + p1)
    args = (lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9)
    want, flag = _capi.gibbs_chain_from_tape(*args, tape)
    half0 = draws // 2
    w, mean_w, negative = _capi.gibbs_chain_device(engine, *args, tape, stat_first=half0)
    assert not negative and not flag
    scale = np.max(np.abs(want), axis=0)
    assert np.max(np.abs(w - want) / scale) < TOL
    assert np.max(np.abs(mean_w - want[half0:].mean(axis=0)) / scale) < TOL


@pytest.mark.parametrize('p1', [3, 60, 150])
def test_device_recursion_is_bitwise_the_host_recursion_on_finished_normals(exact_engine, p1, monkeypatch):
    """Finishing done by the host (exact log): what is left for the device is the recursion -- division, square root,
    products and the three sums in the host's order -- and the draws come out bit for bit."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    rng = np.random.default_rng(100 + p1)
    draws = 500
    lamb, qty = model(p1, rng)
    tape = host_tape(p1, draws, 77 + p1)
    args = (lamb, qty, 40.0, 1.5, 2e4, 0.2, 1.1)
    _capi.finish_tape_blocks(tape)
    want, _ = _capi.gibbs_chain_from_finished_tape(*args, tape)
    tape.finishing_requested = True
    job = exact_engine.submit(*args, tape, stat_first=0, follow=False)
    try:
        job.wait()
        w = job.fetch_w()
        sig, tau = job.last_state
    finally:
        job.release()
    assert np.array_equal(w, want)
    assert np.isfinite(sig) and np.isfinite(tau)


def test_negative_bstar_is_flagged_and_goes_nan_like_the_host(engine, monkeypatch):
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    rng = np.random.default_rng(5)
    lamb, qty = model(6, rng)
    tape = host_tape(6, 50, 3)
    args = (lamb, qty, -1e9, 2.0, 10.0, 0.3, 0.9)                     # b far below zero: bstar < 0 at once
    want, flag = _capi.gibbs_chain_from_tape(*args, tape)
    w, mean_w, negative = _capi.gibbs_chain_device(engine, *args, tape)
    assert flag and negative
    assert np.array_equal(np.isnan(w), np.isnan(want)) and np.isnan(w[1:]).all()
    # (the first row is formed before anything goes NaN: the fast recursion's Newton-refined reciprocal square root is within
    # a rounding or two of the host's 1 / x and sqrt)
    assert np.allclose(w[0], want[0], rtol=1e-14, atol=0)


def test_chains_follow_tapes_that_are_still_on_record_and_slots_are_recycled(engine):
    """Jobs are submitted while the pool's noise thread is still recording the tapes (the dispatcher waits for each
    tape's progress flag); more jobs than slots go through as slots are released; a full engine says so."""
    rng = np.random.default_rng(9)
    np.random.seed(4)
    s_pool, s_ref = _capi.LegacyStream(), _capi.LegacyStream()
    pool = _capi.HostPool(s_pool, chain_threads=1, finish_threads=0, spectral_threads=0)
    draws, jobs = 400, []
    sizes = [40, 61, 8, 130, 60, 60, 59, 58, 57, 12, 300, 5]
    try:
        for p in sizes:
            lamb, qty = model(p, rng)
            tape = _capi.NoiseTape(p, draws)
            noise = pool.submit_noise(tape, 500.0 + p / 2, 4 + (p - 1) / 2)
            args = (lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9)
            while True:
                try:
                    job = engine.submit(*args, tape, stat_first=draws // 2)
                    break
                except _capi.FoklNativeError as exc:                    # all 8 slots alive: release the oldest
                    assert exc.code == -3
                    old = jobs.pop(0)
                    check(old, draws, s_ref)
            jobs.append((job, noise, args, p))
        while jobs:
            check(jobs.pop(0), draws, s_ref)
    finally:
        pool.close()
    assert engine.stats()['issued'] >= len(sizes)


def check(entry, draws, s_ref):
    job, noise, args, p = entry
    mean_w, flag = job.wait()
    noise.wait()
    w = job.fetch_w()
    job.release()
    want = _capi.gibbs_chain(args[0], args[1], 500.0 + p / 2, 4 + (p - 1) / 2, *args[2:], draws, s_ref)
    scale = np.max(np.abs(want), axis=0)
    assert flag[0] == 0 and np.max(np.abs(w - want) / scale) < TOL
    assert np.max(np.abs(mean_w - want[draws // 2:].mean(axis=0)) / scale) < TOL


@pytest.mark.parametrize('draws', [1, 2, 7, 8, 9, 17, 129])
def test_short_chains_and_ring_boundaries(engine, exact_engine, draws, monkeypatch):
    """Fewer iterations than the prefetch ring holds, one more than it holds, one more than a staged block of gammas:
    the clamped row indices of the ring and the gamma blocks must not leak into the results."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    rng = np.random.default_rng(draws)
    for p1 in (3, 70):
        lamb, qty = model(p1, rng)
        tape = host_tape(p1, draws, 5 * draws + p1)
        args = (lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9)
        want, _ = _capi.gibbs_chain_from_tape(*args, tape)
        for eng in (engine, exact_engine):
            w, mean_w, negative = _capi.gibbs_chain_device(eng, *args, tape, stat_first=draws // 2)
            scale = np.max(np.abs(want), axis=0)
            assert not negative and np.max(np.abs(w - want) / scale) < TOL
            assert np.max(np.abs(mean_w - want[draws // 2:].mean(axis=0)) / scale) < TOL


def test_largest_model_and_beyond(engine, monkeypatch):
    """768 columns is what one wavefront holds (12 eigen-directions per lane); beyond that the engine says so and the
    search keeps such chains on the host threads (engine.ForwardSelection.device_chain_columns)."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    rng = np.random.default_rng(768)
    lamb, qty = model(768, rng)
    tape = host_tape(768, 40, 768)
    args = (lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9)
    want, _ = _capi.gibbs_chain_from_tape(*args, tape)
    w, _, negative = _capi.gibbs_chain_device(engine, *args, tape)
    assert not negative and np.max(np.abs(w - want) / np.max(np.abs(want), axis=0)) < TOL
    lamb, qty = model(769, rng)
    with pytest.raises(_capi.FoklNativeError) as err:
        engine.submit(lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9, host_tape(769, 10, 1), follow=False)
    assert err.value.code == -2 and '768' in str(err.value)


def test_tapes_in_ordinary_memory_are_staged(engine, monkeypatch):
    """A tape in page-locked memory (fokl_host_alloc) is read by the device in place; one in ordinary memory goes through
    copy calls and a device staging buffer: same draws either way."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    rng = np.random.default_rng(11)
    p1, draws = 45, 300
    lamb, qty = model(p1, rng)
    args = (lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9)
    np.random.seed(5)
    s1, s2 = _capi.LegacyStream(), _capi.LegacyStream()
    plain = _capi.noise_tape(p1, draws, 500.0, 26.0, s1)
    need = _capi.NoiseTape.doubles_needed(p1, draws) + 8
    pinned = _capi.record_noise_tape(_capi.NoiseTape(p1, draws, _capi.pinned_empty(need)), 500.0, 26.0, s2)
    before = engine.stats()['staged']
    w_plain, _, _ = _capi.gibbs_chain_device(engine, *args, plain)
    assert engine.stats()['staged'] == before + 1
    w_pinned, _, _ = _capi.gibbs_chain_device(engine, *args, pinned)
    assert engine.stats()['staged'] == before + 1
    assert np.array_equal(w_plain, w_pinned)


@pytest.mark.parametrize('p1,pos', [(1, 0), (2, 1), (7, 623), (60, 2), (61, 311), (129, 624), (586, 5)])
def test_rows_expanded_on_the_device_equal_the_tape_expanded_on_the_host(p1, pos, monkeypatch):
    """Round 4: a tape as 32-byte rows (fokl_stream_walk).  The engine regenerates the stream's segments from the raw
    pre-states the host's bulk threads leave in its ring (MT19937 recurrence, tempering, numpy's doubles: exact) and
    expands the rows there -- accepted attempts re-decided from x1^2 + x2^2 with the host's roundings -- so the chain it
    runs is the host chain on the host-expanded tape up to log()."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    eng = _capi.DeviceChainEngine(int(os.environ.get('FOKL_DEVICE', '0')), slots=8)
    try:
        np.random.seed(100 + p1)
        st = np.random.get_state()
        stream = _capi.LegacyStream(('MT19937', st[1], pos, 0, 0.0))
        se = _capi.StreamEngine(stream, 2, prestates=eng.prestate_ring())
        eng.bind(se._h)
        rng = np.random.default_rng(p1)
        draws = 300 if p1 > 200 else 2000
        astar, atau_star = 5e5 + p1 / 2, 4 + (p1 - 1) / 2
        args = (900.0, 2.0, 5e5, 0.3, 0.9)
        jobs, wants, holds = [], [], []
        for rep in range(3):                                  # three tapes back to back: later ones start mid-segment
            lamb, qty = model(p1, rng)
            tape = _capi.NoiseTape(p1, draws, raw=_capi.pinned_empty(_capi.NoiseTape.doubles_needed(p1, draws)))
            first = se.tell().position
            holds.append(se.walk(tape, astar, atau_star))
            span = np.array([holds[-1], se.tell().position], dtype=np.uint64)
            assert span[0] <= first
            jobs.append(eng.submit_rows(lamb, qty, *args, astar, atau_star, tape, span, stat_first=draws // 2))
            host = _capi.NoiseTape(p1, draws)
            host.rows[:] = tape.rows
            se.expand(host, astar, atau_star)
            host.progress[0] = draws
            wants.append(_capi.gibbs_chain_from_tape(lamb, qty, *args, host)[0])
        for job, want in zip(jobs, wants):
            mean_w, flag = job.wait()
            w = job.fetch_w()
            scale = np.max(np.abs(want), axis=0)
            assert not flag[0]
            assert np.max(np.abs(w - want) / scale) < TOL
            assert np.max(np.abs(mean_w - want[draws // 2:].mean(axis=0)) / scale) < TOL
            job.release()
        assert eng.stream_stats()['rows_jobs'] == 3 and eng.stream_stats()['segments_made'] >= 1
        for hold in holds:
            se.release(hold)
        eng.bind(None)
        se.close()
    finally:
        eng.close()


@pytest.mark.parametrize('p1', [586, 768])
def test_sixteen_wide_chains_at_once_at_the_full_chain_length(p1, monkeypatch):
    """the size classes above four elements per lane (T = 12: up to 768 columns) and tapes in page-locked buffers
    of exactly the size they need had no clean batched run on record (tools/chain_device_probe.py died at 586 columns).
    Sixteen chains of 2000 iterations in flight together, from tapes recorded into exact-size page-locked buffers (the
    one-thread recorder and its whole-vector stores included) and from rows expanded on the device: every one equals the
    host chain on the same tape."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    draws, chains = 2000, 16
    eng = _capi.DeviceChainEngine(int(os.environ.get('FOKL_DEVICE', '0')), slots=2 * chains)
    try:
        rng = np.random.default_rng(p1)
        args = (900.0, 2.0, 5e5, 0.3, 0.9)
        astar, atau_star = 5e5 + p1 / 2, 4 + (p1 - 1) / 2
        np.random.seed(p1)
        old_stream = _capi.LegacyStream()
        se = _capi.StreamEngine(_capi.LegacyStream(), 3, prestates=eng.prestate_ring())
        eng.bind(se._h)
        jobs, holds = [], []
        for c in range(chains):
            lamb, qty = model(p1, rng)
            raw = _capi.pinned_empty(_capi.NoiseTape.doubles_needed(p1, draws))
            tape = _capi.NoiseTape(p1, draws, raw=raw)
            if c % 2 == 0:
                # the round-3 path: the one-thread recorder into the page-locked buffer, gathered over the bus
                _capi.record_noise_tape(tape, astar, atau_star, old_stream)
                job = eng.submit(lamb, qty, *args, tape, stat_first=draws // 2, follow=False)
                want = _capi.gibbs_chain_from_tape(lamb, qty, *args, tape)[0]
            else:
                # the round-4 path: rows, expanded on the device
                holds.append(se.walk(tape, astar, atau_star))
                span = np.array([holds[-1], se.tell().position], dtype=np.uint64)
                job = eng.submit_rows(lamb, qty, *args, astar, atau_star, tape, span, stat_first=draws // 2)
                host = _capi.NoiseTape(p1, draws)
                host.rows[:] = tape.rows
                se.expand(host, astar, atau_star)
                host.progress[0] = draws
                want = _capi.gibbs_chain_from_tape(lamb, qty, *args, host)[0]
            jobs.append((job, want))
        for job, want in jobs:
            mean_w, flag = job.wait()
            w = job.fetch_w()
            scale = np.max(np.abs(want), axis=0)
            assert not flag[0]
            assert np.max(np.abs(w - want) / scale) < TOL
            assert np.max(np.abs(mean_w - want[draws // 2:].mean(axis=0)) / scale) < TOL
            job.release()
        for hold in holds:
            se.release(hold)
        eng.bind(None)
        se.close()
    finally:
        eng.close()


# ---- the segmented recursion at its seams and in its fallback -------------------------------------------------------------

def collect(job):
    """Everything a chain leaves behind, then its slot back."""
    try:
        mean_w, flag = job.wait()
        return dict(w=job.fetch_w(), mean=np.array(mean_w), flag=bool(flag[0]), state=job.last_state, bad_cut=job.bad_cut,
                    rows=job.rows_averaged)
    finally:
        job.release()


def run_all(eng, lamb, qty, args, tape, stat_firsts):
    """One job per stat_first, all submitted before any is waited for (they share a launch)."""
    jobs = [eng.submit(lamb, qty, *args, tape, stat_first=first, follow=False) for first in stat_firsts]
    return [collect(job) for job in jobs]


def finished(tape):
    """The normals completed on the host (as the host twin sees them): the device runs the recursion alone."""
    tape.finishing_requested = True
    return tape


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def scaled(got, want, scale):
    return np.max(np.abs(got - want) / scale)


def seams(draws):
    piece = -(-draws // _capi.CHAIN_SEGMENTS)
    return piece, [0, 1, piece - 1, piece, piece + 1, draws - 1, draws, draws + 5]


@pytest.mark.parametrize('p1', [20, 100, 200, 586])
def test_a_finite_chain_that_fails_its_cut_is_the_one_wavefront_recursion_bit_for_bit(engine, serial_engine, p1):
    """The fallback on FINITE chains (helpers.slow_chain_case: a gamma shape of p1 / 2 + 4 carries sigma^2 almost undamped):
    every piece runs, the check fails on finite states, wavefront 0 runs the chain again from start to end over rows the
    pieces already stored, and the sums of wavefronts 1-7, their flags and the end state are the re-run's, not the pieces'.
    stat_first on a seam between two pieces and away from one."""
    draws = 300 if p1 > 200 else 2000
    piece = -(-draws // _capi.CHAIN_SEGMENTS)
    firsts = [4 * piece, 4 * piece + 37, 0]
    lamb, qty, args, tape = slow_chain_case(p1, draws)
    want, want_flag = _capi.gibbs_chain_from_finished_tape(lamb, qty, *args, tape)
    assert not want_flag and np.isfinite(want).all()
    assert _capi.gibbs_chain_segments_host(lamb, qty, *args, tape)[2]             # the host twin takes the same decision
    finished(tape)
    before, serial_before = engine.stats()['recuts'], serial_engine.stats()['recuts']
    got = run_all(engine, lamb, qty, args, tape, firsts)
    ref = run_all(serial_engine, lamb, qty, args, tape, firsts)
    assert engine.stats()['recuts'] == before + len(firsts)                       # exactly one per chain
    assert serial_engine.stats()['recuts'] == serial_before
    scale = np.max(np.abs(want), axis=0)
    for first, g, r in zip(firsts, got, ref):
        assert g['bad_cut'] and not r['bad_cut']
        assert not g['flag'] and not r['flag']
        assert np.isfinite(g['w']).all()
        assert same_bits(g['w'], r['w'])
        assert same_bits(g['mean'], r['mean']) and g['rows'] == r['rows'] == draws - first
        assert g['state'] == r['state'] and np.isfinite(g['state']).all()
        assert scaled(g['w'], want, scale) < TOL
        assert scaled(g['mean'], want[first:].mean(axis=0), scale) < TOL


GOOD_CUTS = [('model', 1), ('model', 64), ('model', 65), ('model', 129), ('model', 586), ('forgets', 20), ('forgets', 100),
             ('forgets', 130)]


@pytest.mark.parametrize('kind,p1', GOOD_CUTS)
def test_a_cut_that_holds_is_not_run_again_and_agrees_to_the_checks_tolerance(engine, serial_engine, kind, p1, monkeypatch):
    """Chains that forget their state within the warm-up (the fit's own kind, and slow_chain_case under a gamma shape of
    p1 / 2 + 400): no fallback, not counted, draws and end state those of the one-wavefront recursion to 1e-12."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    draws = 300 if p1 > 200 else 2000
    if kind == 'model':
        lamb, qty = model(p1, np.random.default_rng(p1))
        tape = host_tape(p1, draws, 10 + p1)
        args = (900.0, 2.0, 5e5, 0.3, 0.9)
        want, want_flag = _capi.gibbs_chain_from_tape(lamb, qty, *args, tape)
    else:
        lamb, qty, args, tape = slow_chain_case(p1, draws, extra=400.0)
        want, want_flag = _capi.gibbs_chain_from_finished_tape(lamb, qty, *args, tape)
        assert not _capi.gibbs_chain_segments_host(lamb, qty, *args, tape)[2]     # the host twin's cut holds too
        finished(tape)
    assert not want_flag
    piece = -(-draws // _capi.CHAIN_SEGMENTS)
    firsts = [4 * piece, 4 * piece + 37]
    before = engine.stats()['recuts']
    got = run_all(engine, lamb, qty, args, tape, firsts)
    ref = run_all(serial_engine, lamb, qty, args, tape, firsts)
    assert engine.stats()['recuts'] == before
    scale = np.max(np.abs(want), axis=0)
    for first, g, r in zip(firsts, got, ref):
        assert not g['bad_cut'] and not r['bad_cut'] and not g['flag'] and not r['flag']
        assert scaled(g['w'], r['w'], scale) < TOL and scaled(g['w'], want, scale) < TOL
        assert scaled(g['mean'], r['mean'], scale) < TOL
        assert scaled(g['mean'], want[first:].mean(axis=0), scale) < TOL
        assert g['rows'] == draws - first
        assert np.max(np.abs(np.array(g['state']) / np.array(r['state']) - 1)) < 1e-12


@pytest.mark.parametrize('draws', [255, 256, 257, 2001, 4096])
def test_cut_boundaries_and_where_the_statistics_start(engine, serial_engine, draws, monkeypatch):
    """Either side of the 4 x warm-up switch between one piece and eight, a ragged last piece, pieces whose gamma staging
    starts at a different phase on every wavefront (k_begin = s * piece - 64, staged 32 at a time), and the first row of the
    statistics on, beside and beyond every kind of seam -- beyond the last row there is nothing to average: means 0.0."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    piece, firsts = seams(draws)
    for p1 in (3, 70, 129):
        lamb, qty = model(p1, np.random.default_rng(1000 * draws + p1))
        tape = host_tape(p1, draws, 3 * draws + p1)
        args = (900.0, 2.0, 5e5, 0.3, 0.9)
        want, want_flag = _capi.gibbs_chain_from_tape(lamb, qty, *args, tape)
        assert not want_flag
        before = engine.stats()['recuts']
        got = run_all(engine, lamb, qty, args, tape, firsts)
        ref = run_all(serial_engine, lamb, qty, args, tape, firsts if draws < 4 * _capi.CHAIN_WARM else firsts[:1])
        assert engine.stats()['recuts'] == before
        scale = np.max(np.abs(want), axis=0)
        assert scaled(ref[0]['w'], want, scale) < TOL
        for n, (first, g) in enumerate(zip(firsts, got)):
            assert not g['bad_cut'] and not g['flag']
            assert same_bits(g['w'], got[0]['w'])                                  # the draws do not depend on stat_first
            assert scaled(g['w'], ref[0]['w'], scale) < TOL and scaled(g['w'], want, scale) < TOL
            rows = max(draws - first, 0)
            assert g['rows'] == rows
            if rows == 0:
                assert same_bits(g['mean'], np.zeros(p1))
            else:
                assert scaled(g['mean'], ref[0]['w'][first:].mean(axis=0), scale) < TOL
                assert scaled(g['mean'], want[first:].mean(axis=0), scale) < TOL
            assert np.max(np.abs(np.array(g['state']) / np.array(ref[0]['state']) - 1)) < 1e-12
            if draws < 4 * _capi.CHAIN_WARM:                                       # one piece, no cut: the same bits
                r = ref[n]
                assert same_bits(g['w'], r['w']) and same_bits(g['mean'], r['mean']) and g['state'] == r['state']


@pytest.mark.parametrize('p1', [6, 130])
def test_a_flagged_chain_at_full_length_comes_back_through_the_fallback(engine, serial_engine, p1, monkeypatch):
    """bstar < 0 at once (b far below zero) in a chain long enough to be cut: every piece goes NaN, the check fails through
    the NaN comparison, the one-piece re-run flags again and the flag comes back through the workgroup's any_flag; at 130
    columns wavefronts 1-7 write the means of the columns from 64 on.
    (A chain whose FIRST negative bstar falls behind row 256: test_a_chain_that_flags_late_...)"""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    draws = 2000
    lamb, qty = model(p1, np.random.default_rng(5 + p1))
    tape = host_tape(p1, draws, 3 + p1)
    args = (-1e9, 2.0, 10.0, 0.3, 0.9)
    want, want_flag = _capi.gibbs_chain_from_tape(lamb, qty, *args, tape)
    assert want_flag and np.isnan(want[1:]).all()
    firsts = [0, 1000, 1037]
    before = engine.stats()['recuts']
    got = run_all(engine, lamb, qty, args, tape, firsts)
    ref = run_all(serial_engine, lamb, qty, args, tape, firsts)
    assert engine.stats()['recuts'] == before + len(firsts)
    for first, g, r in zip(firsts, got, ref):
        assert g['flag'] and r['flag'] and g['bad_cut'] and not r['bad_cut']
        assert np.array_equal(np.isnan(g['w']), np.isnan(want))
        assert same_bits(g['w'][0], r['w'][0]) and np.allclose(g['w'][0], want[0], rtol=1e-14, atol=0)
        assert np.isnan(g['mean']).all() and np.isnan(r['mean']).all() and g['rows'] == r['rows'] == draws - first
        assert np.isnan(g['state']).all() and np.isnan(r['state']).all()


def late_flag_case(seed, draws=2000):
    """Eigenvalues comparable to 1 / tausqd, dtd barely above sum qty^2 / lamb and b < 0 half way between the two floors of
    bstar (tau^2 large / tau^2 = tausqd0): sum d qty^2 moves with tau^2, and bstar first falls below zero hundreds of rows
    into the chain (found by a scan over seeds on the host; most chains of this kind flag in their first rows or never)."""
    p1 = 20
    np.random.seed(seed)
    tape = _capi.noise_tape(p1, draws, p1 / 2 + 4.0, p1 / 2 + 3.0, _capi.LegacyStream())
    _capi.finish_tape_blocks(tape)
    rng = np.random.default_rng(seed)
    lamb = np.sort(rng.random(p1) * 1.5 + 0.5)
    qty = rng.standard_normal(p1) * np.sqrt(lamb) * 3
    at_start, at_large = np.sum(qty ** 2 / (lamb + 1 / 0.9)), np.sum(qty ** 2 / lamb)
    dtd = at_large * 1.02
    b = -0.5 * ((dtd - at_large) + 0.5 * (at_large - at_start))
    return lamb, qty, (b, 2.0, dtd, 0.3, 0.9), tape


@pytest.mark.parametrize('seed', [0, 6, 19])
def test_a_chain_that_flags_late_is_finite_up_to_there_and_flagged_like_the_one_wavefront_recursion(engine, serial_engine, seed):
    """The first negative bstar in piece 1 or 2 of eight: the pieces in front are clean, the re-run must carry the chain to
    that row with the one-wavefront recursion's bits, flag there, and leave NaN behind it -- rows the pieces had stored
    finite values in."""
    draws = 2000
    lamb, qty, args, tape = late_flag_case(seed, draws)
    want, want_flag = _capi.gibbs_chain_from_finished_tape(lamb, qty, *args, tape)
    first_nan = int(np.argmax(np.isnan(want).any(axis=1)))
    assert want_flag and first_nan > 4 * _capi.CHAIN_WARM and np.isnan(want[first_nan:]).all()
    assert _capi.gibbs_chain_segments_host(lamb, qty, *args, tape)[1:] == (True, True)
    finished(tape)
    firsts = [0, first_nan + 3]
    got = run_all(engine, lamb, qty, args, tape, firsts)
    ref = run_all(serial_engine, lamb, qty, args, tape, firsts)
    scale = np.max(np.abs(want[:first_nan]), axis=0)
    for g, r in zip(got, ref):
        assert g['flag'] and r['flag'] and g['bad_cut'] and not r['bad_cut']
        assert np.array_equal(np.isnan(g['w']), np.isnan(want))
        assert same_bits(g['w'], r['w'])
        assert scaled(g['w'][:first_nan], want[:first_nan], scale) < TOL
        assert np.isnan(g['mean']).all() and np.isnan(g['state']).all() and np.isnan(r['state']).all()


def test_a_recycled_slot_shows_nothing_of_the_chain_before(serial_engine, monkeypatch):
    """One slot, hence one statistics area: a chain that took the fallback (indicator 1, means of 130 columns written by three
    wavefronts), then a flagged one, then a chain of the same size whose cut holds -- whose indicator, flag, means and end
    state must be its own.  (An ordinary sequential check of what the epilogue writes.)"""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    eng = _capi.DeviceChainEngine(int(os.environ.get('FOKL_DEVICE', '0')), slots=1)
    try:
        p1, draws, first = 130, 2000, 1000
        lamb, qty, args, tape = slow_chain_case(p1, draws)
        slow = run_all(eng, lamb, qty, args, finished(tape), [first])[0]
        assert slow['bad_cut'] and not slow['flag'] and eng.stats()['recuts'] == 1
        lamb2, qty2 = model(p1, np.random.default_rng(77))
        tape2 = host_tape(p1, draws, 78)
        nan = run_all(eng, lamb2, qty2, (-1e9, 2.0, 10.0, 0.3, 0.9), tape2, [first])[0]
        assert nan['bad_cut'] and nan['flag'] and np.isnan(nan['mean']).all() and eng.stats()['recuts'] == 2
        args2 = (900.0, 2.0, 5e5, 0.3, 0.9)
        want, _ = _capi.gibbs_chain_from_tape(lamb2, qty2, *args2, tape2)
        good = run_all(eng, lamb2, qty2, args2, tape2, [first])[0]
        ref = run_all(serial_engine, lamb2, qty2, args2, tape2, [first])[0]
        assert not good['bad_cut'] and not good['flag'] and good['rows'] == draws - first and eng.stats()['recuts'] == 2
        scale = np.max(np.abs(want), axis=0)
        assert scaled(good['w'], want, scale) < TOL and scaled(good['mean'], want[first:].mean(axis=0), scale) < TOL
        assert scaled(good['mean'], ref['mean'], scale) < TOL
        assert np.max(np.abs(np.array(good['state']) / np.array(ref['state']) - 1)) < 1e-12
        # ... and the fallback again behind a good chain
        again = run_all(eng, lamb, qty, args, tape, [first])[0]
        assert again['bad_cut'] and same_bits(again['w'], slow['w']) and same_bits(again['mean'], slow['mean'])
        assert again['state'] == slow['state'] and eng.stats()['recuts'] == 3
    finally:
        eng.close()


def test_fallback_and_good_chains_mixed_in_one_batch(monkeypatch):
    """Sixteen jobs queued before any is waited for, fallback and good chains alternating over the size classes of 1, 2, 4
    and 12 elements per lane: neighbours in a launch, on the streams and in the slots do not touch each other -- each job is
    its own single-job result bit for bit."""
    monkeypatch.setenv('FOKL_FINISH_LOG', 'exact')
    draws = 400
    eng = _capi.DeviceChainEngine(int(os.environ.get('FOKL_DEVICE', '0')), slots=16)
    try:
        cases = []
        for rep in range(2):
            for p1 in (20, 100, 200, 586):
                lamb, qty, args, tape = slow_chain_case(p1, draws)
                cases.append((True, lamb, qty, args, finished(tape), 150 + 37 * rep))
                lamb, qty = model(p1, np.random.default_rng(40 + p1 + rep))
                cases.append((False, lamb, qty, (900.0, 2.0, 5e5, 0.3, 0.9), host_tape(p1, draws, 50 + p1 + rep), 200 * rep))
        jobs = [eng.submit(lamb, qty, *args, tape, stat_first=first, follow=False) for _, lamb, qty, args, tape, first in cases]
        together = [collect(job) for job in jobs]
        assert eng.stats()['recuts'] == 8
        for (slow, lamb, qty, args, tape, first), g in zip(cases, together):
            alone = run_all(eng, lamb, qty, args, tape, [first])[0]
            assert g['bad_cut'] == alone['bad_cut'] == slow and not g['flag']
            assert same_bits(g['w'], alone['w']) and same_bits(g['mean'], alone['mean'])
            assert g['state'] == alone['state'] and g['rows'] == alone['rows'] == draws - first
        assert eng.stats()['recuts'] == 16
    finally:
        eng.close()

"""A host chain's recursion in verified segments (fokl_gibbs_chain_segments_host, csrc/fokl_chain_lanes.inc) against the
one-piece recursion, and the statistics formed behind a sub-stage model's chain.  No GPU needed."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT, slow_chain_case as slow_case
from fokl_gpy_amd import _capi

SIZES = (1, 7, 8, 9, 64, 100, 145)
DRAWS = (255, 256, 2000, 2001)
ARGS = (900.0, 2.0, 5e5, 0.3, 0.9)                                       # b, btau, dtd, sigsqd0, tausqd0


def _case(p1, draws, seed=5, astar=None, atau_star=None):
    np.random.seed(seed + p1)
    stream = _capi.LegacyStream()
    tape = _capi.noise_tape(p1, draws, 5e5 + p1 / 2 if astar is None else astar,
                            3 + p1 / 2 if atau_star is None else atau_star, stream)
    _capi.finish_tape_blocks(tape)
    rng = np.random.default_rng(seed * 1000 + p1)
    lamb = np.sort(rng.random(p1) * 1e5 + 10)
    qty = rng.standard_normal(p1) * 100
    return lamb, qty, tape


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture
def mapping(monkeypatch):
    def choose(recursion=None, mapping=None):
        for name, value in (('FOKL_HCHAIN_RECURSION', recursion), ('FOKL_HCHAIN_MAPPING', mapping)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, value)
    choose()
    return choose


@pytest.mark.parametrize('p1', SIZES)
def test_segments_against_the_one_piece_recursion(p1, mapping):
    for draws in DRAWS:
        lamb, qty, tape = _case(p1, draws)
        b, btau, dtd, s0, t0 = ARGS
        want, want_flag = _capi.gibbs_chain_from_finished_tape(lamb, qty, b, btau, dtd, s0, t0, tape)
        # (a) FOKL_HCHAIN_RECURSION=serial is the old entry point
        mapping(recursion='serial')
        w, flag, bad_cut = _capi.gibbs_chain_segments_host(lamb, qty, b, btau, dtd, s0, t0, tape)
        assert _same_bits(w, want) and flag == want_flag and not bad_cut
        # (b) in segments: the draws and the state of every iteration inside 1e-12, the flag equal
        mapping(mapping='lanes')
        w, flag, bad_cut, sigs, taus = _capi.gibbs_chain_segments_host(lamb, qty, b, btau, dtd, s0, t0, tape, states=True)
        mapping(recursion='serial')
        _, _, _, want_sigs, want_taus = _capi.gibbs_chain_segments_host(lamb, qty, b, btau, dtd, s0, t0, tape, states=True)
        assert flag == want_flag and not bad_cut
        assert np.max(np.abs(w - want) / np.max(np.abs(want), axis=0)) < 1e-12
        assert np.max(np.abs(sigs / want_sigs - 1)) < 1e-12 and np.max(np.abs(taus / want_taus - 1)) < 1e-12
        # (c) pieces across lanes == pieces one after the other through the one-piece recursion's own iteration
        mapping(mapping='pieces')
        w2, flag2, bad2, sigs2, taus2 = _capi.gibbs_chain_segments_host(lamb, qty, b, btau, dtd, s0, t0, tape, states=True)
        assert _same_bits(w, w2) and _same_bits(sigs, sigs2) and _same_bits(taus, taus2) and flag2 == flag and not bad2
        # (e) too short to be cut: one piece, the one-piece recursion's bits
        if draws < 4 * _capi.CHAIN_WARM:
            assert _same_bits(w, want)
        # (f) the same input twice: the same bits
        mapping(mapping='lanes')
        again = _capi.gibbs_chain_segments_host(lamb, qty, b, btau, dtd, s0, t0, tape)
        assert _same_bits(again[0], w)


def test_other_cuts_and_warm_ups(mapping):
    lamb, qty, tape = _case(37, 1000)
    want, _ = _capi.gibbs_chain_from_finished_tape(lamb, qty, *ARGS, tape)
    for segments, warm in ((1, 64), (2, 64), (3, 10), (5, 100), (8, 0), (8, 250), (8, 251)):
        by_mapping = []
        for name in ('lanes', 'pieces'):
            mapping(mapping=name)
            w, flag, bad_cut = _capi.gibbs_chain_segments_host(lamb, qty, *ARGS, tape, segments=segments, warm=warm)
            by_mapping.append(w)
            assert not flag
            if bad_cut or segments == 1 or 1000 < 4 * warm:              # (no warm-up at all cannot pass the check)
                assert _same_bits(w, want)
            else:
                assert np.max(np.abs(w - want) / np.max(np.abs(want), axis=0)) < 1e-12
        assert _same_bits(*by_mapping)
    assert _capi.gibbs_chain_segments_host(lamb, qty, *ARGS, tape, segments=8, warm=0)[2]      # bad_cut: nothing forgotten
    with pytest.raises(_capi.FoklNativeError):
        _capi.gibbs_chain_segments_host(lamb, qty, *ARGS, tape, segments=9)


@pytest.mark.parametrize('name', ['lanes', 'pieces'])
def test_a_chain_that_does_not_forget_runs_in_one_piece(name, mapping):
    """(d) A gamma shape barely above p1 / 2 carries sigma^2 from one iteration to the next almost undamped: the pieces do not
    meet at FINITE states, bad_cut is reported and the result is the one-piece recursion's, bit for bit.  (Not a flagged
    chain: every draw is finite.  That case is test_a_flagged_chain_returns_what_it_always_did.)"""
    for p1 in (20, 100, 200):
        lamb, qty, args, tape = slow_case(p1)
        want, want_flag = _capi.gibbs_chain_from_finished_tape(lamb, qty, *args, tape)
        assert not want_flag and np.isfinite(want).all()
        mapping(mapping=name)
        w, flag, bad_cut = _capi.gibbs_chain_segments_host(lamb, qty, *args, tape)
        assert bad_cut and not flag and np.isfinite(w).all() and _same_bits(w, want)
        # the same model under a gamma shape that forgets: the cut holds, the draws are the one-piece recursion's to 1e-12
        if p1 <= 130:
            lamb, qty, args, tape = slow_case(p1, extra=400.0)
            want, _ = _capi.gibbs_chain_from_finished_tape(lamb, qty, *args, tape)
            w, flag, bad_cut = _capi.gibbs_chain_segments_host(lamb, qty, *args, tape)
            assert not bad_cut and not flag
            assert np.max(np.abs(w - want) / np.max(np.abs(want), axis=0)) < 1e-12


@pytest.mark.parametrize('name', ['lanes', 'pieces'])
def test_a_flagged_chain_returns_what_it_always_did(name, mapping):
    """(d) bstar < 0 (b far below zero) in the first piece: NaN rows and the flag exactly as the one-piece recursion leaves them."""
    lamb, qty, tape = _case(20, 2000)
    args = (-1e12, 2.0, 5e5, 0.3, 0.9)
    want, want_flag = _capi.gibbs_chain_from_finished_tape(lamb, qty, *args, tape)
    assert want_flag and np.isnan(want).any()
    mapping(mapping=name)
    w, flag, bad_cut = _capi.gibbs_chain_segments_host(lamb, qty, *args, tape)
    assert bad_cut and flag and _same_bits(w, want)


_DIGEST = """
import hashlib, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_chain_segments_host import _case, ARGS
from fokl_gpy_amd import _capi
h = hashlib.sha256()
for p1 in (7, 8, 9, 64, 145):
    for draws in (256, 2001):
        lamb, qty, tape = _case(p1, draws)
        w, flag, bad_cut, sigs, taus = _capi.gibbs_chain_segments_host(lamb, qty, *ARGS, tape, states=True)
        assert not bad_cut
        h.update(w.tobytes()); h.update(sigs.tobytes()); h.update(taus.tobytes())
print(h.hexdigest())
"""


def test_portable_avx2_and_avx512_statements_agree_bit_for_bit():
    """(c) The statement is chosen once per process (FOKL_CHAIN_ISA): one process each.  On a CPU without AVX2 / AVX-512 the
    request falls back to what the CPU has, and the digests agree trivially."""
    digests = {}
    for isa in ('base', 'avx2', 'avx512'):
        env = dict(os.environ, FOKL_CHAIN_ISA=isa, FOKL_HCHAIN_MAPPING='lanes')
        env.pop('FOKL_HCHAIN_RECURSION', None)
        res = subprocess.run([sys.executable, '-c', _DIGEST.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))],
                             capture_output=True, text=True, env=env, timeout=600)
        assert res.returncode == 0, res.stderr
        digests[isa] = res.stdout.strip().splitlines()[-1]
    assert len(set(digests.values())) == 1, digests


@pytest.mark.parametrize('finish_threads', [0, 2])
def test_pool_chains_run_in_segments_behind_the_finish_threads(finish_threads, mapping):
    """Through the pool, following the block flags of a tape that is still being finished: the one-piece recursion's draws
    inside 1e-12, counted as segmented when the tape is finished for the chain and long enough to cut."""
    np.random.seed(33)
    rng = np.random.default_rng(4)
    stream = _capi.LegacyStream()
    pool = _capi.HostPool(stream, chain_threads=2, finish_threads=finish_threads, spectral_threads=0)
    jobs = []
    for p1, draws in ((9, 2000), (70, 2000), (145, 1001), (33, 255)):
        lamb, qty = np.linspace(1.0, 1e4, p1), rng.standard_normal(p1) * 30
        tape = _capi.NoiseTape(p1, draws)
        noise = pool.submit_noise(tape, 4e3 + p1 / 2, 4 + p1 / 2, finish=True)
        jobs.append((lamb, qty, tape, noise, pool.submit_chain(lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9, tape)))
    for lamb, qty, tape, noise, chain in jobs:
        w, flag = chain.wait()
        noise.wait()
        want, _ = _capi.gibbs_chain_from_finished_tape(lamb, qty, 900.0, 2.0, 5e5, 0.3, 0.9, tape) \
            if tape.finishing_requested else (None, None)
        if want is not None:
            assert flag[0] == 0 and np.max(np.abs(w - want) / np.max(np.abs(want), axis=0)) < 1e-12
    busy = pool.busy_seconds()
    assert busy['host_chains_segmented'] == (3 if finish_threads else 0) and busy['host_chain_recuts'] == 0
    pool.close()

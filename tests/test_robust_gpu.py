"""fokl_robust_pass / _step / _chains (csrc/fokl_robust_device.inc) on the device against their statement robust.pass_host /
step_host / robust_host, over the edges of the row chunks and the 16-column blocks; determinism; refusals; and
FoKL.resample_robust end to end behind a fit.

Two references for the pass:
  * exact -- columns, y and weights are small integers and nu = inf, so every sum of G is an exact integer in any order:
    ``np.array_equal`` against numpy's integer Gram.  This pins the chunk edges, the padding rows and columns, which wavefront
    owns which block pair, the y block, the mirrored triangles and the reduce over the workgroups' partials.
  * drawn -- continuous columns and nu = 4 against pass_host: the attempts equal except in rows where an accept test was
    decided by the last bit; lam elsewhere relative to the row's lam; G against numpy's Gram formed from the DEVICE's own
    lam, relative to sqrt(G_ii G_jj).
Device against statement the two maths libraries differ in the last bits of log / cos, and a P-wide Cholesky lifts them.
Measured over every case below before anything was asserted (each test prints its figures; DESIGN section 3, robust), the
largest differences are
    lam     1.51e-15 of the row's lam (n = 4 099; below 1e-15 up to 65 rows: the worst of more rows)
    G       4.03e-15 of sqrt(G_ii G_jj) (n = 4 099, one column; the order of the sum over the rows, sqrt(n) ulp)
    step    3.68e-17 of the largest coefficient (P + 1 = 64; sigsqd and tausqd bit-equal, no coordinate off by more than an ulp)
    chains  6.27e-13 of the scale over 1, 2 and 5 iterations of 1 and 3 chains (lam_i after five iterations: a last-place
            difference in beta passes through r_i^2 / sigsqd of the gross errors)
with equal attempt counts in every row and every chain; every bound is ten times its measurement, all far below the project's
draw tolerance of 1e-9.
"""
import warnings

import numpy as np
import pytest

from helpers import load_case
from test_score_gpu import stage
from fokl_gpy_amd import FoKLRoutines, _capi, robust as RB
from fokl_gpy_amd.embedded import basis_matrix

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 63, 64, 65, 1000, 4099)
WIDTHS = (1, 2, 15, 16, 17, 63, 64, 127)                                  # P + 1
# every n at two widths, every width at three n
SHAPES = sorted({(n, nc) for n in ROWS for nc in (16, 127)} | {(n, nc) for n in (17, 65, 4099) for nc in WIDTHS})
SEED = 13
MEASURED_LAM, MEASURED_GRAM, MEASURED_STEP, MEASURED_CHAIN = 1.51e-15, 4.03e-15, 3.68e-17, 6.27e-13
TOL_LAM, TOL_GRAM, TOL_STEP, TOL_CHAIN = (10 * m for m in (MEASURED_LAM, MEASURED_GRAM, MEASURED_STEP, MEASURED_CHAIN))


def integer_case(n, nc, seed=0):
    rng = np.random.default_rng(seed)
    cols = rng.integers(-3, 4, size=(n, nc - 1)).astype(np.float64)
    y = rng.integers(-20, 21, size=n).astype(np.float64)
    w = rng.integers(1, 5, size=n).astype(np.float64)
    return cols, y, w


def continuous_case(n, nc, seed=1):
    """Columns of unit scale, y = X beta + noise with a few gross errors -> cols, y, w, a beta near the least-squares point."""
    rng = np.random.default_rng(seed)
    cols = rng.uniform(-1.0, 1.0, size=(n, nc - 1))
    X = np.concatenate([np.ones((n, 1)), cols], axis=1)
    truth = rng.standard_normal(nc) / np.sqrt(nc)
    y = X @ truth + 0.1 * rng.standard_normal(n)
    y[::17] += 1.0
    w = rng.uniform(0.5, 2.0, size=n)
    return cols, y, w, truth + 0.01 * rng.standard_normal(nc) / np.sqrt(nc)


def integer_gram(X, y, w):
    Z = np.concatenate([X, y[:, None]], axis=1).astype(np.int64)
    return (Z.T @ (Z * w.astype(np.int64)[:, None])).astype(np.float64)


@pytest.mark.parametrize('n,nc', SHAPES + [(16500, 3)])
def test_exact_pass(device_ctx, n, nc):
    """(16 500 rows: more chunks than workgroups, so a workgroup walks two chunks.)"""
    cols, y, w = integer_case(n, nc)
    slots, X = stage(device_ctx, cols, y)
    G, lam, att = device_ctx.robust_pass(slots, w, None, 1.0, np.inf, SEED, 0, 3)
    assert np.array_equal(G, integer_gram(X, y, w)), (n, nc)
    assert np.array_equal(lam, np.ones(n)) and not att.any()
    rep = device_ctx.robust_report()
    chunks = -(-n // 64)
    per_group = -(-chunks // 256)
    blocks = -(-(nc + 1) // 16)
    assert rep['grid'] == (-(-chunks // per_group), 1) and rep['columns'] == nc + 1 and rep['blocks'] == blocks
    assert rep['partial_doubles'] == 256 * blocks * (blocks + 1) // 2 and rep['iterations'] == 1 and rep['attempts'] == 0
    assert rep['lds_bytes'] == 8 * (16 * blocks * 66 + 320 + 32 * blocks) and rep['pass_ms'] > 0.0
    # without weights, and at iteration 0 of a finite nu: lam = 1 all the same
    G1 = device_ctx.robust_pass(slots, None, np.zeros(nc), 1.0, 4.0, SEED, 0, 0, want_rows=False)[0]
    assert np.array_equal(G1, integer_gram(X, y, np.ones(n)))


@pytest.mark.parametrize('n,nc', SHAPES)
def test_drawn_pass(device_ctx, n, nc):
    cols, y, w, beta = continuous_case(n, nc)
    slots, X = stage(device_ctx, cols, y)
    Z = np.concatenate([X, y[:, None]], axis=1)
    worst_lam = worst_gram = 0.0
    parted = 0
    for iteration in (1, 7):
        for chain in (0, 2):
            G, lam, att = device_ctx.robust_pass(slots, w, beta, 0.01, 4.0, SEED, chain, iteration)
            G_h, lam_h, att_h = RB.pass_host(X, y, w, beta, 0.01, 4.0, SEED, chain, iteration)
            same = att == att_h
            parted += int((~same).sum())
            assert (~same).sum() <= n // 100
            assert np.all(att >= 1) and device_ctx.robust_report()['attempts'] == int(att.sum())
            gap = np.abs(lam[same] - lam_h[same]) / lam_h[same]
            worst_lam = max(worst_lam, float(gap.max()) if gap.size else 0.0)
            expect = Z.T @ (Z * (w * lam)[:, None])
            d = np.sqrt(np.diag(expect))
            worst_gram = max(worst_gram, float(np.max(np.abs(G - expect) / np.outer(d, d))))
            assert np.array_equal(G, G.T)
            again = device_ctx.robust_pass(slots, w, beta, 0.01, 4.0, SEED, chain, iteration)
            assert np.array_equal(again[0], G) and np.array_equal(again[1], lam) and np.array_equal(again[2], att)
        assert not np.array_equal(lam, device_ctx.robust_pass(slots, w, beta, 0.01, 4.0, SEED, 0, iteration)[1]) or n == 0
    print(f"n = {n}, P + 1 = {nc}: lam {worst_lam:.3e} of the row's lam, G {worst_gram:.3e} of sqrt(G_ii G_jj); {parted} rows "
          f"parted by an accept test")
    assert worst_lam <= TOL_LAM and worst_gram <= TOL_GRAM


def hyper(n, nc):
    return RB.hyper_of(4.0, 0.05, 4.0, 1.0, n, nc - 1)


@pytest.mark.parametrize('nc', [1, 17, 64, 127])
def test_step(device_ctx, nc):
    n = 1000
    cols, y, w, beta = continuous_case(n, nc)
    slots, X = stage(device_ctx, cols, y)
    worst = 0.0
    for iteration, chain, nu in ((0, 0, 4.0), (1, 2, 4.0), (7, 1, 4.0)):
        G = device_ctx.robust_pass(slots, w, beta, 0.01, nu, SEED, chain, iteration, want_rows=False)[0]
        for sig, tau in ((0.01, 0.5), (0.3, 1e-3)):
            got = device_ctx.robust_step(G, sig, tau, hyper(n, nc), SEED, chain, iteration)
            rep = device_ctx.robust_report()
            assert rep['grid'] == (0, 1) and rep['step_lds_bytes'] == 8 * ((nc + 1) * ((nc + 1) | 1) + 7 * 128 + 8) and rep['step_ms'] > 0
            want = RB.step_host(G, sig, tau, hyper(n, nc), SEED, chain, iteration)
            assert got[3] == want[3] == RB.FLAG_NONE
            gaps = [np.max(np.abs(got[0] - want[0])) / np.max(np.abs(want[0])), abs(got[1] / want[1] - 1), abs(got[2] / want[2] - 1)]
            worst = max(worst, float(max(gaps)))
            assert np.array_equal(device_ctx.robust_step(G, sig, tau, hyper(n, nc), SEED, chain, iteration)[0], got[0])
    print(f"P + 1 = {nc}: step {worst:.3e} of the scale")
    assert worst <= TOL_STEP
    # the flags: bstar < 0 through b, a pivot that is not positive
    bad = dict(hyper(n, nc), b=-1e9)
    assert device_ctx.robust_step(G, 0.01, 0.5, bad, SEED, 0, 1)[3] == RB.step_host(G, 0.01, 0.5, bad, SEED, 0, 1)[3] == RB.FLAG_BSTAR_NEGATIVE
    G = G.copy()
    G[0, 0] = -1e9
    got, want = device_ctx.robust_step(G, 0.01, 0.5, hyper(n, nc), SEED, 0, 1), RB.step_host(G, 0.01, 0.5, hyper(n, nc), SEED, 0, 1)
    assert got[3] == want[3] == RB.FLAG_PIVOT and np.isnan(got[0]).all() and np.isnan(got[1])


CHAIN_N, CHAIN_NC = 1000, 17
_CASE = {}


def chain_case(device_ctx):
    """One dataset, its statement runs and its shift, shared by the chain tests."""
    if not _CASE:
        cols, y, w, beta = continuous_case(CHAIN_N, CHAIN_NC, seed=3)
        X = np.concatenate([np.ones((CHAIN_N, 1)), cols], axis=1)
        _CASE.update(cols=cols, y=y, w=w, X=X, shift=beta, hyper=hyper(CHAIN_N, CHAIN_NC), host={})
    slots, _ = stage(device_ctx, _CASE['cols'], _CASE['y'])
    return slots, _CASE


def starts(chains):
    return 0.01 * (1.0 + 0.1 * np.arange(chains)), 0.5 * (1.0 + 0.2 * np.arange(chains))


def host_run(case, chains, iterations):
    key = (chains, iterations)
    if key not in case['host']:
        sig0, tau0 = starts(chains)
        case['host'][key] = RB.robust_host(case['X'], case['y'], case['w'], 4.0, case['hyper'], case['shift'], sig0, tau0, 0,
                                           iterations, 1, SEED)
    return case['host'][key]


def test_chains_against_the_statement(device_ctx):
    slots, case = chain_case(device_ctx)
    worst, cut_short, compared = 0.0, 0, 0
    for chains in (1, 3):
        sig0, tau0 = starts(chains)
        for iterations in (1, 2, 5):
            host = host_run(case, chains, iterations)
            dev = device_ctx.robust_chains(slots, case['w'], 4.0, case['hyper'], case['shift'], sig0, tau0, 0, iterations, 1, SEED)
            rep = device_ctx.robust_report()
            assert rep['grid'] == (16, chains) and rep['iterations'] == iterations and rep['kept'] == iterations
            assert rep['attempts'] == int(dev['counts'][:, 2].sum()) and rep['flagged'] == 0 and rep['timed_iterations'] == iterations
            assert rep['pass_ms'] > 0 and rep['reduce_ms'] > 0 and rep['step_ms'] > 0 and rep['total_ms'] > 0
            scale = np.max(np.abs(host['betas']), axis=(0, 1))
            for c in range(chains):
                compared += 1
                same = dev['attempts'][c] == host['attempts'][c]
                upto = iterations if same.all() else int(np.argmin(same)) + 1      # the row that parted used the same state
                cut_short += upto < iterations
                gaps = [np.max(np.abs(dev['betas'][c, :upto] - host['betas'][c, :upto]) / scale),
                        np.max(np.abs(dev['sigsqd'][c, :upto] / host['sigsqd'][c, :upto] - 1)),
                        np.max(np.abs(dev['tausqd'][c, :upto] / host['tausqd'][c, :upto] - 1))]
                if upto == iterations:
                    assert np.array_equal(dev['counts'][c], host['counts'][c])
                    gaps.append(np.max(np.abs(dev['sums'][c] - host['sums'][c]) / np.maximum(np.abs(host['sums'][c]), 1e-3)))
                    gaps.append(np.max(np.abs(dev['lam_sum'][c] - host['lam_sum'][c]) / host['lam_sum'][c]))
                worst = max(worst, float(max(gaps)))
    print(f"chains: {worst:.3e} of the scale; {cut_short} of {compared} chains cut short by an attempt count")
    assert worst <= TOL_CHAIN and cut_short <= 1


def test_chains_bookkeeping_and_determinism(device_ctx):
    slots, case = chain_case(device_ctx)
    sig0, tau0 = starts(3)
    args = (slots, case['w'], 4.0, case['hyper'], case['shift'])
    base = device_ctx.robust_chains(*args, sig0, tau0, 2, 9, 1, SEED)
    again = device_ctx.robust_chains(*args, sig0, tau0, 2, 9, 1, SEED)
    for key in base:
        assert np.array_equal(base[key], again[key]), key
    alone = device_ctx.robust_chains(*args, sig0[2:], tau0[2:], 2, 9, 1, SEED, chain_ids=[2])
    for key in base:
        assert np.array_equal(base[key][2:], alone[key]), key
    assert not np.array_equal(base['betas'][0], base['betas'][1])
    thinned = device_ctx.robust_chains(*args, sig0, tau0, 2, 9, 3, SEED)
    assert thinned['betas'].shape == (3, 3, CHAIN_NC) and device_ctx.robust_report()['kept'] == 3
    for key in ('betas', 'sigsqd', 'tausqd', 'attempts'):
        assert np.array_equal(thinned[key], base[key][:, ::3]), key
    for key in ('sums', 'counts', 'lam_sum'):
        assert np.array_equal(thinned[key], base[key]), key
    none = device_ctx.robust_chains(*args, sig0, tau0, 2, 9, 1, SEED, rows=False)
    assert none['betas'] is None and none['attempts'] is None
    for key in ('sums', 'counts', 'lam_sum'):
        assert np.array_equal(none[key], base[key]), key
    # the sums are the rows': first half (4), second half (4), the odd last
    dev = base['betas'] - case['shift']
    for seg, rows in enumerate((slice(0, 4), slice(4, 8), slice(8, 9))):
        assert np.allclose(base['sums'][:, seg, 0, :CHAIN_NC], dev[:, rows].sum(axis=1), rtol=1e-12, atol=1e-15)
        assert np.allclose(base['sums'][:, seg, 1, CHAIN_NC], (base['sigsqd'][:, rows] ** 2).sum(axis=1), rtol=1e-12)


def test_weight_sums_are_the_passes_lam(device_ctx):
    slots, case = chain_case(device_ctx)
    sig0, tau0 = starts(2)
    run = device_ctx.robust_chains(slots, case['w'], 4.0, case['hyper'], case['shift'], sig0, tau0, 0, 4, 1, SEED)
    for c in range(2):
        total = np.ones(CHAIN_N)                                                   # iteration 0: lam = 1
        for k in range(1, 4):
            total = total + device_ctx.robust_pass(slots, case['w'], run['betas'][c, k - 1], run['sigsqd'][c, k - 1], 4.0, SEED, c, k)[1]
        assert np.array_equal(run['lam_sum'][c], total)
    late = device_ctx.robust_chains(slots, case['w'], 4.0, case['hyper'], case['shift'], sig0, tau0, 2, 2, 1, SEED)
    lam2 = device_ctx.robust_pass(slots, case['w'], run['betas'][1, 1], run['sigsqd'][1, 1], 4.0, SEED, 1, 2)[1]
    lam3 = device_ctx.robust_pass(slots, case['w'], run['betas'][1, 2], run['sigsqd'][1, 2], 4.0, SEED, 1, 3)[1]
    assert np.array_equal(late['lam_sum'][1], lam2 + lam3) and np.array_equal(late['betas'], run['betas'][:, 2:])


def test_gaussian_noise_runs_one_pass(device_ctx):
    slots, case = chain_case(device_ctx)
    sig0, tau0 = starts(2)
    device_ctx.timing_enable(True)
    device_ctx.timing_reset()
    dev = device_ctx.robust_chains(slots, case['w'], np.inf, case['hyper'], case['shift'], sig0, tau0, 1, 4, 1, SEED)
    assert device_ctx.timing_get(_capi.K_ROBUST)['launches'] == 3 + 4
    device_ctx.timing_reset()
    device_ctx.robust_chains(slots, case['w'], 4.0, case['hyper'], case['shift'], sig0, tau0, 1, 4, 1, SEED)
    assert device_ctx.timing_get(_capi.K_ROBUST)['launches'] == 3 * 5
    device_ctx.timing_enable(False)
    host = RB.robust_host(case['X'], case['y'], case['w'], np.inf, case['hyper'], case['shift'], sig0, tau0, 1, 4, 1, SEED)
    assert np.array_equal(dev['lam_sum'], np.full((2, CHAIN_N), 4.0)) and np.array_equal(dev['counts'], host['counts'])
    assert np.max(np.abs(dev['betas'] - host['betas']) / np.max(np.abs(host['betas']))) <= TOL_CHAIN


def test_a_flagged_chain_is_alone(device_ctx):
    slots, case = chain_case(device_ctx)
    h = dict(case['hyper'], b=-0.45 * float(case['w'] @ (case['y'] ** 2)))
    sig0, tau0 = np.full(3, 0.01), np.array([1e-12, 1e6, 1e-12])
    dev = device_ctx.robust_chains(slots, case['w'], 4.0, h, case['shift'], sig0, tau0, 0, 3, 1, SEED)
    host = RB.robust_host(case['X'], case['y'], case['w'], 4.0, h, case['shift'], sig0, tau0, 0, 3, 1, SEED)
    assert np.array_equal(dev['counts'][:, :2], host['counts'][:, :2]) and dev['counts'][1, 0] == 0
    assert np.all(dev['counts'][:, 1] == RB.FLAG_BSTAR_NEGATIVE) and device_ctx.robust_report()['flagged'] == 3
    assert np.isnan(dev['sigsqd'][1]).all() and np.isnan(dev['betas'][1, 1:]).all() and np.isfinite(dev['betas'][[0, 2], 0]).all()
    tau0[1] = 1e-12
    twin = device_ctx.robust_chains(slots, case['w'], 4.0, h, case['shift'], sig0, tau0, 0, 3, 1, SEED)
    for key in dev:
        assert np.array_equal(twin[key][[0, 2]], dev[key][[0, 2]], equal_nan=True), key
    # a row that meets the attempt cap is NaN, and so is its chain; nothing hangs
    capped = device_ctx.robust_chains(slots, case['w'], 4.0, case['hyper'], case['shift'], sig0[:1], [0.5], 0, 2, 1, SEED, attempt_cap=1)
    host = RB.robust_host(case['X'], case['y'], case['w'], 4.0, case['hyper'], case['shift'], sig0[:1], [0.5], 0, 2, 1, SEED, attempt_cap=1)
    assert np.array_equal(capped['counts'][:, :2], host['counts'][:, :2]) and capped['counts'][0, 1] == RB.FLAG_ATTEMPT_CAP
    assert capped['counts'][0, 0] == 1 and np.isnan(capped['betas'][0, 1]).all() and np.isfinite(capped['betas'][0, 0]).all()


def test_native_refusals_launch_nothing(device_ctx, monkeypatch):
    ctx = device_ctx
    slots, case = chain_case(ctx)
    sig0, tau0 = starts(1)
    args = (slots, case['w'], 4.0, case['hyper'], case['shift'], sig0, tau0, 0, 2, 1, SEED)
    before = ctx.robust_chains(*args)
    ctx.timing_enable(True)
    ctx.timing_reset()
    wide_slots = np.array([_capi.SLOT_ONES] + [2] * 127, dtype=np.int32)
    refused = [
        (lambda: ctx.robust_pass(wide_slots, None, None, 1.0, np.inf, 0, 0, 0), 'at most 127'),
        (lambda: ctx.robust_chains(wide_slots, None, 4.0, case['hyper'], np.zeros(128), sig0, tau0, 0, 2, 1, 0), 'at most 127'),
        (lambda: ctx.robust_step(np.eye(129), 0.1, 0.1, case['hyper'], 0, 0, 0), 'at most 127'),
        (lambda: ctx.robust_pass(np.array([0, 99999], dtype=np.int32), None, None, 1.0, np.inf, 0, 0, 0), 'slot 99999 outside'),
        (lambda: ctx.robust_chains(np.array([0, -1], dtype=np.int32), None, 4.0, case['hyper'], np.zeros(2), sig0, tau0, 0, 2, 1, 0), 'slot -1 outside'),
        (lambda: ctx.robust_pass(slots, case['w'][:-1], None, 1.0, np.inf, 0, 0, 0), '999 weights for 1000 rows'),
        (lambda: ctx.robust_chains(slots, np.ones(1001), 4.0, case['hyper'], case['shift'], sig0, tau0, 0, 2, 1, 0), '1001 weights for 1000 rows'),
        (lambda: ctx.robust_pass(slots, None, case['shift'], 0.1, 0.5, 0, 0, 1), 'nu < 1'),
        (lambda: ctx.robust_chains(slots, None, np.nan, case['hyper'], case['shift'], sig0, tau0, 0, 2, 1, 0), 'nu < 1 or NaN'),
        (lambda: ctx.robust_chains(slots, None, 4.0, dict(case['hyper'], atau_star=0.5), case['shift'], sig0, tau0, 0, 2, 1, 0), 'shapes >= 1'),
        (lambda: ctx.robust_pass(slots, None, None, 0.1, 4.0, 0, 0, 1), 'needs beta'),
    ]
    for call, text in refused:
        with pytest.raises(_capi.FoklNativeError, match=text) as exc:
            call()
        assert exc.value.code == -2
        assert ctx.robust_report()['iterations'] == 0 and ctx.robust_report()['grid'] == (0, 0)
    monkeypatch.setenv('FOKL_ROBUST_FREE_BYTES', str(65 << 20))                 # 64 MiB are to stay spare
    with pytest.raises(_capi.FoklNativeError, match='bytes of rows.*partial Grams.*free'):
        ctx.robust_chains(slots, case['w'], 4.0, case['hyper'], case['shift'], np.full(64, 0.01), np.full(64, 0.5), 0, 2, 1, SEED)
    with pytest.raises(_capi.FoklNativeError, match='partial Grams.*free'):
        ctx.robust_pass(np.array([0] + list(range(2, 18)) * 7, dtype=np.int32), None, None, 1.0, np.inf, 0, 0, 0)
    monkeypatch.delenv('FOKL_ROBUST_FREE_BYTES')
    assert ctx.timing_get(_capi.K_ROBUST)['launches'] == 0
    ctx.timing_enable(False)
    assert np.array_equal(ctx.read_slot(2), case['cols'][:, 0]) and np.array_equal(ctx.read_slot(_capi.SLOT_Y), case['y'])
    after = ctx.robust_chains(*args)
    for key in before:
        assert np.array_equal(before[key], after[key]), key


def test_resample_robust_behind_a_fit(device_ctx):
    g, hy, kname, kid, phis = load_case('bern_m8_capped')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = FoKLRoutines.FoKL(kernel=kname, phis=phis, UserWarnings=False, ConsoleOutput=False, **hy)
        np.random.seed(int(g['seed']))
        betas, mtx, evs = model.fit(g['raw_inputs'], g['raw_data'], clean=True)
        X = basis_matrix(np.asarray(model.inputs), mtx, phis, kname)
        data = np.asarray(model.data, dtype=np.float64).reshape(-1)
        n = data.shape[0]
        sd = float(np.sqrt(np.mean((data - X @ np.asarray(betas).mean(axis=0)) ** 2)))
        rng = np.random.default_rng(0)
        rows = rng.choice(n, max(n // 50, 1), replace=False)
        shifted = data.copy()
        shifted[rows] += 20.0 * sd * rng.choice([-1.0, 1.0], rows.shape[0])
        state = np.random.get_state()
        res = model.resample_robust(data=shifted, chains=2, draws=300, burnin=100)
        gauss = model.resample(data=shifted, chains=2, draws=300, burnin=100)
        after = np.random.get_state()
        assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        sd_t, sd_g = float(np.sqrt(res.sigsqd.mean())), float(np.sqrt(gauss.sigsqd.mean()))
        rep = FoKLRoutines.device_backend().ctx.robust_report()
        print(f"n = {n}, P + 1 = {mtx.shape[0] + 1}: residual sd {sd:.5f}; robust {sd_t:.5f}, gaussian {sd_g:.5f}; shifted rows' "
              f"weight_mean at most {res.weight_mean[rows].max():.4f}, the others at least {np.delete(res.weight_mean, rows).min():.4f}; "
              f"400 iterations in {rep['total_ms']:.1f} ms")
        assert res.betas.shape == (600, mtx.shape[0] + 1) and res.nu == 4.0 and res.noise == 'student' and not res.flagged.any()
        assert rep['iterations'] == 400 and rep['grid'][1] == 2 and rep['kept'] == 300
        assert abs(sd_t - sd) <= 0.15 * sd
        assert sd_g > 2.0 * sd
        assert res.weight_mean[rows].max() < np.delete(res.weight_mean, rows).min()
        assert max(res.rhat['betas'].max(), res.rhat['sigsqd']) < 1.1
        mean = model.evaluate(betas=res.betas, draws=res.betas.shape[0])
        mean = mean[0] if isinstance(mean, tuple) else mean
        assert np.max(np.abs(mean[:40] - (res.betas @ X[:40].T).mean(axis=0))) < 1e-9
        assert model.propagate(betas=res.betas).mean.shape == (600,)
        for call in (model.score, model.predictive):
            with pytest.raises(ValueError, match='Gaussian likelihood'):
                call(res)

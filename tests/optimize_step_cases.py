"""What tests/test_optimize_step_host.py, tests/test_optimize_step_gpu.py and tests/test_optimize_system_step_gpu.py share
(no tests here): the models and systems one iteration of the optimisers is traced on, the references the traced values
are compared with, and the recomputation of every decision of a traced iteration from the traced values.

Three references, each for what it can decide without a margin:

EXACT.  An integer coefficient table (orders 1 to 4), integer betas in -3 .. 3 and starts on k / 8: every factor, product
and sum of F, noise, g and H is a dyadic rational that fits a double, so the order of the sums does not matter and the
device must equal ``optimize._model_parts`` bit for bit.  That the reference itself is exact is shown on the CPU against
``fractions.Fraction`` arithmetic (``fraction_parts``) at every point the device tests use.

RATIONAL.  The real Bernoulli table at the device's own traced points.  A double is a rational and so is every operation
of the evaluation: ``fraction_parts`` gives the exact F, g and H of those doubles.  The tolerance is the standard running
bound |computed - exact| <= gamma_N M, gamma_N = N u / (1 - N u), u = 2**-53, where M is the same expression with every
coefficient, factor and term replaced by its magnitude (formed exactly, in Fractions) and N counts the roundings on the
longest path from an input to the result (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3 and 5):
    Horner of order p          2 p    a multiplication and an addition per step; a coefficient that ends in phi' or phi''
                                      passes at most p steps of the three coupled recurrences all the same (the final
                                      doubling of phi'' is exact)
    a mapped input a + b z     2 p + 3  the point itself carries 2 roundings, which p powers multiply: 2 p; phi' b is
                                      one more, phi'' (b b) two, so 3 at most
    the product of a term      k + 1  k - 1 multiplications of its k factors (one of them a derivative, or two), one by
                                      the coefficient; for the system one more, the weight times the coefficient
    the sum over T terms       T + 1  every term and the constant pass at most T additions; + 1 for the system's sum of
                                      the weighted model gradient into g
so N = 2 p + k + T + 2 for a model (p its largest order, k its widest term, T its terms) and 4 p + k + T + 6 for a
mapped model of a system.  N is derived, not tuned; the tests print the largest observed error / bound.

DECISIONS.  Whatever an iteration decides -- the projected gradient and the stop test, the active set, the factor, the
direction, every Armijo test, the point it moves to, the multiplier / penalty update -- is recomputed by the host
statement's own operations in the statement's order FROM THE DEVICE'S TRACED NUMBERS (``check_decisions``).  Division and
square root are correctly rounded on both sides and nothing is fused, so the device must agree bit for bit.
"""
from fractions import Fraction

import numpy as np

from fokl_gpy_amd import getKernels
from fokl_gpy_amd import optimize as opt

PHIS = getKernels.bernoulli()
TABLE = getKernels.pack_phis(PHIS, getKernels.KERNEL_BERNOULLI)[0]
# orders 1 to 4, width 5, constant first; integers in -3 .. 3, the leading one non-zero
INT_TABLE = np.array([[1.0, 2.0, 0.0, 0.0, 0.0],
                      [-1.0, 3.0, -2.0, 0.0, 0.0],
                      [2.0, -3.0, 1.0, 3.0, 0.0],
                      [-2.0, 1.0, -1.0, 2.0, -3.0]])
UNIT = 2.0 ** -53
TRIALS = opt.MAX_HALVINGS + 1


def gamma(N):
    return Fraction(N) * Fraction(UNIT) / (1 - Fraction(N) * Fraction(UNIT))


def tri(i, j):
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


# ---------------------------------------------------------------------------------------------------------
# the exact models
# ---------------------------------------------------------------------------------------------------------

def row_of(m, **orders):
    row = np.zeros(m, dtype=np.int32)
    for name, order in orders.items():
        row[int(name[1:])] = order
    return row


def exact_model(name):
    """mtx of 'one' (m = 1, one term), 'six' (6 inputs: main effects of orders 1 to 3, 8 pairs and 8 triples with orders
    1 to 4, three 4-factor terms, one 5-factor term, a row of zeros) and 'sixteen' (m = 16: the FIRST term reads variable
    15, two orders of it sit in different terms, pairs (15, 14) and (15, 0), the triple (0, 7, 15), a 4-factor term with
    15; its 136 Hessian entries put a solve's LDS above 64 KB)."""
    if name == 'one':
        return np.array([[3]], dtype=np.int32)
    if name == 'six':
        rng = np.random.default_rng(6)
        m = 6
        rows = [row_of(m, **{f'x{j}': order}) for j in range(m) for order in (1, 2, 3)]
        for width, count in ((2, 8), (3, 8)):
            for _ in range(count):
                row = np.zeros(m, dtype=np.int32)
                row[rng.choice(m, width, replace=False)] = rng.integers(1, 5, width)
                rows.append(row)
        rows += [row_of(m, x0=1, x1=2, x3=1, x5=2), row_of(m, x1=1, x2=1, x4=2, x5=1), row_of(m, x0=2, x2=1, x3=1, x4=1),
                 row_of(m, x0=1, x1=1, x2=1, x4=1, x5=2), np.zeros(m, dtype=np.int32)]
        return np.array(rows, dtype=np.int32)
    m = 16
    rows = [row_of(m, x15=1), row_of(m, x15=3), row_of(m, x15=2, x14=1), row_of(m, x15=1, x0=2), row_of(m, x0=1, x7=2, x15=3),
            row_of(m, x2=1, x5=1, x9=2, x15=2), row_of(m, x0=1), row_of(m, x0=3, x1=1)]
    rows += [row_of(m, **{f'x{j}': 1 + j % 3}) for j in range(1, 15)]
    rows += [row_of(m, **{f'x{j}': 2, f'x{j + 5}': 1}) for j in range(1, 7)]
    return np.array(rows, dtype=np.int32)


def exact_problem(name, E, S, seed=0):
    """Integer betas [E, terms + 1] that differ per draw, starts [S, m] on k / 8 that differ per lane, and the box: [0, 1],
    in the larger models with coordinate 2 fixed at 1 / 2 (the starts are clipped to it, as the kernel clips them)."""
    mtx = exact_model(name)
    m = mtx.shape[1]
    rng = np.random.default_rng(1000 * E + S + seed)
    betas = rng.integers(-3, 4, (E, mtx.shape[0] + 1)).astype(np.float64)
    s, j = np.meshgrid(np.arange(S), np.arange(m), indexing='ij')
    starts = ((s * (2 * j + 1) + j * j + s // 9 + 3 * seed) % 9) / 8.0
    starts[:, 0] = ((s[:, 0] + seed) % 4 // 2 * 8 + (s[:, 0] % 2) * (s[:, 0] % 9)) % 9 / 8.0   # often on a face
    starts[:, m - 1] = np.where(s[:, 0] % 3 == 0, 0.0, np.where(s[:, 0] % 3 == 1, 1.0, starts[:, m - 1]))
    if m == 1:
        starts[:, 0] = (4 * s[:, 0] % 9) / 8.0                         # all nine points, a face every fourth or fifth lane
    lo, hi = np.zeros(m), np.ones(m)
    if m > 2:
        lo[2] = hi[2] = 0.5
    return mtx, betas, np.ascontiguousarray(starts), lo, hi


def first_points(betas, starts, lo, hi):
    """The iterate every solve starts from, [E * S, m], and its draw's coefficients [E * S, terms + 1]: draws are the
    slow axis, as in the kernel."""
    E, S = betas.shape[0], starts.shape[0]
    x0 = np.minimum(np.maximum(starts, lo), hi)
    return np.ascontiguousarray(np.broadcast_to(x0, (E,) + x0.shape).reshape(E * S, -1)), np.repeat(betas, S, axis=0)


# ---------------------------------------------------------------------------------------------------------
# the rational reference
# ---------------------------------------------------------------------------------------------------------

def fraction_parts(mtx, table, z, coef, scale=1.0, weight=None, maps=None, level=2):
    """``optimize._model_parts`` for ONE point z [n] and one coefficient row in exact rational arithmetic.  Returns a dict:
    e, noise (the sum of the exact terms' magnitudes), g [n], H [n (n + 1) / 2] -- Fractions -- and Me, Mg, MH: the same
    expressions with every coefficient, power of the point, factor and term replaced by its magnitude."""
    F = Fraction
    n_terms, n = mtx.shape
    z = [F(float(v)) for v in z]
    weight = scale if weight is None else weight
    scale, weight = F(float(scale)), F(float(weight))
    cache = {}

    def factor(j, order):
        if (j, order) not in cache:
            c = [F(float(v)) for v in table[order - 1][:order + 1]]
            a, b = (F(0), F(1)) if maps is None else (F(float(maps[0][j])), F(float(maps[1][j])))
            y, ya = a + b * z[j], abs(a) + abs(b) * abs(z[j])
            poly = lambda cs, at, d: sum((cs[k] * F(int(np.prod(np.arange(k - d + 1, k + 1)))) * at ** (k - d)
                                          for k in range(d, order + 1)), F(0))
            ca = [abs(v) for v in c]
            cache[(j, order)] = ((poly(c, y, 0), b * poly(c, y, 1), b * b * poly(c, y, 2)),
                                 (poly(ca, ya, 0), abs(b) * poly(ca, ya, 1), b * b * poly(ca, ya, 2)))
        return cache[(j, order)]

    e = scale * F(float(coef[0]))
    noise = Me = abs(e)
    g, Mg = [F(0)] * n, [F(0)] * n
    H, MH = [F(0)] * (n * (n + 1) // 2), [F(0)] * (n * (n + 1) // 2)
    for t in range(n_terms):
        used = [(j, factor(j, int(mtx[t, j]))) for j in range(n) if mtx[t, j]]
        w, wh = scale * F(float(coef[t + 1])), weight * F(float(coef[t + 1]))

        def product(which, derived):
            """(value, magnitude) of the product of the term's factors, those in `derived` by their derivative's order"""
            value, size = F(1), F(1)
            for i, (_, (exact, mags)) in enumerate(used):
                d = derived.get(i, 0)
                value, size = value * exact[d], size * mags[d]
            return value, size

        value, size = product(used, {})
        e, noise, Me = e + w * value, noise + abs(w * value), Me + abs(w) * size
        if level < 2:
            continue
        for a, (ja, _) in enumerate(used):
            value, size = product(used, {a: 1})
            g[ja], Mg[ja] = g[ja] + w * value, Mg[ja] + abs(w) * size
            value, size = product(used, {a: 2})
            H[tri(ja, ja)], MH[tri(ja, ja)] = H[tri(ja, ja)] + wh * value, MH[tri(ja, ja)] + abs(wh) * size
            for b in range(a):
                jb = used[b][0]
                value, size = product(used, {a: 1, b: 1})
                H[tri(ja, jb)], MH[tri(ja, jb)] = H[tri(ja, jb)] + wh * value, MH[tri(ja, jb)] + abs(wh) * size
    return dict(e=e, noise=noise, g=g, H=H, Me=Me, Mg=Mg, MH=MH)


def roundings(mtx, mapped=False):
    """N of the module docstring for this model."""
    p, k, T = int(mtx.max(initial=1)), int((mtx > 0).sum(axis=1).max(initial=1)), mtx.shape[0]
    return 4 * p + k + T + 6 if mapped else 2 * p + k + T + 2


def is_exact(value, exact):
    """Every double of `value` IS the Fraction next to it."""
    value, exact = np.ravel(value), list(exact) if isinstance(exact, (list, tuple)) else [exact]
    return len(value) == len(exact) and all(np.isfinite(v) and Fraction(float(v)) == q for v, q in zip(value, exact))


def worst_ratio(value, exact, size, N):
    """max |value - exact| / (gamma_N size) over the entries (0 where the bound and the error are both 0)."""
    worst = Fraction(0)
    for v, q, s in zip(np.ravel(value), exact if isinstance(exact, list) else [exact], size if isinstance(size, list) else [size]):
        assert np.isfinite(v)
        err = abs(Fraction(float(v)) - q)
        if err:
            assert s > 0, "an error where the bound is zero"
            worst = max(worst, err / (gamma(N) * s))
    return float(worst)


# ---------------------------------------------------------------------------------------------------------
# the decisions of a traced iteration, recomputed from the traced values
# ---------------------------------------------------------------------------------------------------------

def flat(trace):
    """The trace with the solves on one axis: [E * S, ...]."""
    return {key: value.reshape((-1,) + value.shape[2:]) for key, value in trace.items()}


def same(a, b):
    """Bit for bit, NaN where NaN (and +0 == -0: the sign of a zero decides nothing here)."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def check_decisions(tr, lo, hi, tol, k, max_iter, steepest_in, label='', settled=None, update=None):
    """Every decision of the traced iteration k from its traced values, bit for bit.  tr: a flat trace; steepest_in [B]
    what the iteration before carried over (zeros at k = 0).  For the system, ``settled`` [B] replaces pg <= tol in the
    stop test and ``update`` [B] are the solves whose iteration is an update: they do not step.  Returns the counts the
    callers assert occurrences on."""
    run = tr['running']
    B, m = tr['x_in'].shape
    lo_c, hi_c = lo[:, None], hi[:, None]
    xt, g = tr['x_in'][run].T, tr['g'][run].T
    with np.errstate(invalid='ignore', over='ignore'):
        pg = np.max(np.abs(np.minimum(np.maximum(xt - g, lo_c), hi_c) - xt), axis=0)
        finite = np.isfinite(tr['F'][run]) & np.isfinite(g).all(axis=0)
    assert same(tr['pg'][run][finite], pg[finite]), label             # (fmax drops a NaN, numpy's max keeps it)
    assert np.array_equal(tr['active'][run], opt._active_set(xt, g, lo_c, hi_c).T), label
    done = (pg <= tol) if settled is None else settled[run]
    want = np.where(~finite, opt.NON_FINITE, np.where(done, opt.CONVERGED, opt.ITERATION_LIMIT if k == max_iter else -1))
    assert np.array_equal(tr['status_tests'][run], want), (label, tr['status_tests'][run], want)
    # a solve that had stopped keeps its point (-9: its wavefront had ended, nothing was written)
    written = ~run & (tr['status'] != -9)
    assert np.all(tr['status'][written] >= 0) and same(tr['x_out'][written], tr['x_in'][written]), label

    step = run & (tr['status_tests'] == -1)
    if update is not None:
        step = step & ~update
    reached = ~np.isnan(tr['alpha'])                                  # the wavefront went on to the step
    assert np.array_equal(tr['stepping'][reached], step[reached]), label
    step = step & reached
    counts = dict(running=int(run.sum()), stepping=int(step.sum()))
    if not step.any():
        return counts
    x = tr['x_in'][step].copy()
    g, H = tr['g'][step].T.copy(), tr['H'][step].T.copy()
    F, noise = tr['F'][step], tr['noise'][step]
    active, d, use = opt._step_direction(x, g, H, lo, hi, steepest_in[step])
    assert np.array_equal(active.T, tr['active'][step]), label
    assert same(H.T, tr['factor'][step]), (label, 'factor', np.max(np.abs(H.T - tr['factor'][step])))
    assert same(d.T, tr['d'][step]), (label, 'direction')
    assert np.array_equal(use, tr['use_steepest'][step]), label
    # the search: every traced Ft under the Armijo test with slope and moved recomputed from g, x_in and d
    Ft, trials = tr['Ft'][step], tr['trials'][step]
    assert np.all((trials >= 1) & (trials <= TRIALS)), label
    count, searching, alpha, x_out = recount(x, F, noise, g, d, lo, hi, Ft)
    assert np.array_equal(count, trials), (label, count, trials)
    assert all(np.isnan(row[c:]).all() for row, c in zip(Ft, count)), label   # no trial point beyond the accepted one
    assert same(alpha, tr['alpha'][step]) and np.array_equal(searching, tr['failed'][step]), label
    assert same(x_out, tr['x_out'][step]), label
    assert np.array_equal(tr['steepest'][step], searching & ~use), label
    assert np.array_equal(tr['status'][step], np.where(searching & use, opt.STALLED, -1)), label
    moved = np.max(np.abs(x_out - x), axis=1)
    counts.update(first=int((count == 1).sum()), middle=int(((count >= 5) & (count <= 29) & ~searching).sum()),
                  last=int(((count == TRIALS) & ~searching).sum()), failed=int(searching.sum()),
                  stalled=int((searching & use).sum()), steepest=int(use.sum()), moved=int((moved > 0).sum()))
    return counts


def recount(x, F, noise, g, d, lo, hi, Ft):
    """The arc search of every solve from the values Ft [B, 31] its trial points had: the number of trial points (the
    first h that passes, 31 when none does), which solves found none, alpha, and the point each ends at."""
    lo_c, hi_c = lo[:, None], hi[:, None]
    alpha = np.ones(x.shape[0])
    searching = np.ones(x.shape[0], dtype=bool)
    x_out = x.copy()
    count = np.zeros(x.shape[0], dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for h in range(TRIALS):
            if not searching.any():
                break
            trial = np.minimum(np.maximum(x.T + alpha * d, lo_c), hi_c)
            ok = opt._armijo(Ft[:, h], F, noise, g, trial - x.T)
            count[searching] += 1
            take = searching & ok
            x_out[take] = trial.T[take]
            searching = searching & ~ok
            alpha = np.where(searching, alpha * 0.5, alpha)
    return count, searching, alpha, x_out


def host_walk(mtx, table, betas, starts, lo, hi, sign, max_iter, tol):
    """``optimize.solve_host`` with every iteration's record kept: a list over k of dicts (running, x_in, F, noise, g, H,
    status after the tests, trial values [B, 31], trials, failed, use_steepest, x_out), the solves flat."""
    tt = opt.TermTable(np.ascontiguousarray(mtx, dtype=np.int32))
    x, coef = first_points(betas, starts, lo, hi)
    B, m = x.shape
    status = np.full(B, -1)
    steepest = np.zeros(B, dtype=bool)
    lo_c, hi_c = lo[:, None], hi[:, None]
    walk = []
    for it in range(max_iter + 1):
        running = status < 0
        if not running.any():
            break
        F, noise, g, H = opt._evaluate(tt, table, x, coef, sign, 2)
        with np.errstate(invalid='ignore', over='ignore'):
            pg = np.max(np.abs(np.minimum(np.maximum(x.T - g, lo_c), hi_c) - x.T), axis=0)
            finite = np.isfinite(F) & np.isfinite(g).all(axis=0)
        status = np.where(running & ~finite, opt.NON_FINITE, status)
        status = np.where((status < 0) & (pg <= tol), opt.CONVERGED, status)
        if it == max_iter:
            status = np.where(status < 0, opt.ITERATION_LIMIT, status)
        rec = dict(running=running, x_in=x.copy(), F=F, noise=noise, g=g.T.copy(), H=H.T.copy(), pg=pg,
                   status_tests=status.copy(), steepest_in=steepest.copy())
        walk.append(rec)
        stepping = status < 0
        if not stepping.any():
            rec.update(status=status.copy(), x_out=x.copy())
            break
        values = np.full((B, TRIALS), np.nan)
        calls = [0]

        def merit_at(trial):
            values[:, calls[0]] = opt._evaluate(tt, table, trial, coef, sign, 0)[0]
            calls[0] += 1
            return values[:, calls[0] - 1]

        x_in = x.copy()
        _, d, use = opt._step_direction(x, g, H, lo, hi, steepest)
        failed = opt._arc_search(x, F, noise, g, d, lo, hi, stepping, merit_at)
        trials = recount(x_in, F, noise, g, d, lo, hi, values)[0]
        values[np.arange(TRIALS)[None, :] >= trials[:, None]] = np.nan   # what a solve evaluated while it was searching
        values[~stepping], trials = np.nan, np.where(stepping, trials, 0)
        status = np.where(failed & use, opt.STALLED, status)
        steepest = failed & ~use
        rec.update(d=d.T.copy(), use_steepest=use, failed=failed, Ft=values, trials=trials, status=status.copy(),
                   x_out=x.copy(), stepping=stepping)
    return walk


SIZES = ((1, 1), (1, 63), (1, 65), (3, 64), (5, 32), (2, 100))


def rules_seen(x, g, active, lo, hi):
    """Which of the four rules of the active set occur at coordinate 0 and at coordinate m - 1, and whether a fixed
    coordinate does: a set of (coordinate, rule).  x, active [B, m], g [B, m]."""
    seen = set()
    m = x.shape[1]
    for j in sorted({0, m - 1}):
        on_lo, on_hi = x[:, j] <= lo[j], x[:, j] >= hi[j]
        for rule, which in (('lower, g > 0: active', on_lo & (g[:, j] > 0) & active[:, j]),
                            ('lower, g < 0: free', on_lo & (g[:, j] < 0) & ~active[:, j]),
                            ('upper, g < 0: active', on_hi & (g[:, j] < 0) & active[:, j]),
                            ('upper, g > 0: free', on_hi & (g[:, j] > 0) & ~active[:, j])):
            if lo[j] < hi[j] and which.any():
                seen.add((j, rule))
    if np.any((lo == hi) & active.all(axis=0)):
        seen.add('fixed')
    return seen


def all_rules(m, fixed):
    rules = ('lower, g > 0: active', 'lower, g < 0: free', 'upper, g < 0: active', 'upper, g > 0: free')
    return {(j, rule) for j in {0, m - 1} for rule in rules} | ({'fixed'} if fixed else set())


# ---------------------------------------------------------------------------------------------------------
# designed cases: the factorisation and the search
# ---------------------------------------------------------------------------------------------------------

# order o is x**o for o = 1, 2, 3: a model of main effects is a plain polynomial and its Hessian is what its coefficients
# say; "order 4" is (x - 1)**2, whose Horner value and slope are exactly 0 at x = 1
POWERS = np.array([[0.0, 1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0, 0.0], [1.0, -2.0, 1.0, 0.0, 0.0]])
# terms: x0, x0^2, x0^3, x1, x1^2, x0 x1, (x0 - 1)^2
POWER_MTX = np.array([[1, 0], [2, 0], [3, 0], [0, 1], [0, 2], [1, 1], [4, 0]], dtype=np.int32)


def power_betas(c=0.0, x0=0.0, x0x0=0.0, x0x0x0=0.0, x1=0.0, x1x1=0.0, x0x1=0.0, well=0.0):
    return [c, x0, x0x0, x0x0x0, x1, x1x1, x0x1, well]


def factor_cases():
    """Minimisations (sign +1) of c + b . x + x' A x / 2 whose Hessian at the start is A exactly: name -> (betas, start,
    lo, hi, H [3] the lower triangle).  One draw and one start each; the solve of case i is (draw i, start i)."""
    quad = lambda h00, h10, h11, b0=1.0, b1=1.0: power_betas(x0=b0, x1=b1, x0x0=h00 / 2, x0x1=h10, x1x1=h11 / 2)
    box = ([-4.0, -4.0], [4.0, 4.0])
    cases = {
        'positive definite': (quad(4.0, 1.0, 3.0), [0.5, 0.25], *box, [4.0, 1.0, 3.0]),
        'negative pivot': (quad(-2.0, 1.0, 1.0), [0.5, 0.25], *box, [-2.0, 1.0, 1.0]),
        'zero pivot': (quad(4.0, 2.0, 1.0), [0.5, 0.25], *box, [4.0, 2.0, 1.0]),
        'pivot on the floor': (quad(1.0, 0.0, 1e-8), [0.5, 0.25], *box, [1.0, 0.0, 1e-8]),
        # coordinate 1 sits on its lower bound with g > 0: active, and its diagonal of 1e6 must not raise the floor --
        # with it the floor were 1e-2 and the pivot 1e-3 of coordinate 0 replaced: a direction ten times shorter
        'huge diagonal on an active coordinate': (quad(1e-3, 0.0, 1e6, b0=-1e-4, b1=1.0), [0.0, 0.0], [-4.0, 0.0],
                                                  [4.0, 4.0], [1e-3, 0.0, 1e6]),
        'reach below 1': (quad(4.0, 0.0, 4.0, b0=0.0, b1=0.0), [0.5, 0.25], *box, [4.0, 0.0, 4.0]),
        'reach equal to 1': (quad(4.0, 0.0, 4.0, b0=0.0, b1=0.0), [1.0, 0.5], *box, [4.0, 0.0, 4.0]),
        'reach above 1': (quad(4.0, 0.0, 4.0, b0=0.0, b1=0.0), [3.0, 1.0], *box, [4.0, 0.0, 4.0]),
    }
    return cases


# order 1 is 1e200 x: the cross term's second derivative overflows while value and gradient stay finite at x = 1e-200
OVERFLOW_TABLE = np.array([[0.0, 1e200, 0.0], [0.0, 0.0, 1.0]])
OVERFLOW = dict(mtx=np.array([[1, 1], [2, 0], [0, 2]], dtype=np.int32), betas=np.array([[0.0, 1.0, 1.0, 1.0]]),
                starts=np.array([[1e-200, 1e-200]]), lo=np.zeros(2), hi=np.ones(2))


def search_cases():
    """Minimisations whose first arc search ends as named: name -> (betas, start).  Box [0, 2] x [0, 1], tol = 0.
    A (x^3 - eps x) from x = 0: the Hessian is 0 there, the floor pivot makes the Newton direction long, it is scaled to
    1, and a trial point at distance s decreases the value enough only if s^2 <= eps (1 - 1e-4); every number involved is
    a power of two."""
    cubic = lambda A, eps: power_betas(x0=-A * eps, x0x0x0=A)
    return {
        'first': (power_betas(x0=-1.0, x0x0=1.0, x1=-0.5, x1x1=1.0), [1.0, 0.75]),
        'twelfth': (cubic(2.0 ** 40, 2.0 ** -21), [0.0, 0.5]),
        'thirty-first': (cubic(2.0 ** 40, 2.0 ** -59), [0.0, 0.5]),
        'none, then steepest descent': (cubic(2.0 ** 40, 2.0 ** -63), [0.0, 0.5]),
        'none twice: stalled': (cubic(2.0 ** 64, 2.0 ** -63), [0.0, 0.5]),
        # x0^2 - (2 + 2^-51) x0 + (x0 - 1)^2 at x0 = 1: g = -2^-51 exactly and H = 4, the Newton step 2^-53 is half an ulp
        # of 1 and 1 + 2^-53 rounds to 1: no trial point of the Newton direction moves although each passes the decrease
        # test; the steepest-descent step 2^-51 of the next iteration does
        'not moved': (power_betas(x0=-(2.0 + 2.0 ** -51), x0x0=1.0, well=1.0), [1.0, 0.5]),
        # (x0 - 9)^2 + (x1 - 1/2)^2 from (1.5, 0.25): the scaled direction (1, 1/30) leaves the box in x0 only
        'clipped in one coordinate': (power_betas(x0=-18.0, x0x0=1.0, x1=-1.0, x1x1=1.0), [1.5, 0.25]),
    }


def search_problem():
    cases = search_cases()
    betas = np.array([b for b, _ in cases.values()])
    starts = np.array([s for _, s in cases.values()])
    return list(cases), betas, starts, np.zeros(2), np.array([2.0, 1.0])


# ---------------------------------------------------------------------------------------------------------
# the rational check of evaluated values
# ---------------------------------------------------------------------------------------------------------

TWENTY = np.array([[1, 0], [0, 20], [20, 1], [1, 20], [20, 0], [0, 1]], dtype=np.int32)   # orders 1 and 20 of 2 inputs
TWENTY_MEAN = np.array([0.2, 0.7, -1.1, 0.9, -0.8, 1.3, -0.4])


def rational_ratios(mtx, table, x, coef, sign, F, noise, g, H):
    """Largest |computed - exact| / (gamma_N M) of F, noise, g and H at ONE point (g [m], H [m (m + 1) / 2]) against the
    exact rational values of the same doubles; N = ``roundings(mtx)``."""
    N = roundings(mtx)
    ref = fraction_parts(mtx, table, x, coef, sign)
    return dict(F=worst_ratio(F, ref['e'], ref['Me'], N), noise=worst_ratio(noise, ref['noise'], ref['Me'], N),
                g=worst_ratio(g, ref['g'], ref['Mg'], N), H=worst_ratio(H, ref['H'], ref['MH'], N))


def rational_value_ratio(mtx, table, x, coef, sign, Ft):
    ref = fraction_parts(mtx, table, x, coef, sign, level=0)
    return worst_ratio(Ft, ref['e'], ref['Me'], roundings(mtx))


def trial_points(x_in, d, lo, hi, count):
    """The first `count` trial points of one solve, as the kernel and the statement form them."""
    return [np.minimum(np.maximum(x_in + 2.0 ** -h * d, lo), hi) for h in range(count)]


# ---------------------------------------------------------------------------------------------------------
# systems
# ---------------------------------------------------------------------------------------------------------

INT_PHIS = [INT_TABLE[o - 1][:o + 1] for o in range(1, 5)]
BERN = 'Bernoulli Polynomials'
SYS_TOL, SYS_CTOL = 1e-9, 1e-8


def int_model(mtx, minmax, E, seed):
    mtx = np.array(mtx, dtype=np.int32)
    betas = np.random.default_rng(seed).integers(-3, 4, (E, mtx.shape[0] + 1)).astype(np.float64)
    return dict(betas=betas, mtx=mtx, phis=INT_PHIS, minmax=minmax, kernel=BERN)


def exact_system(name, E, S):
    """A prepared system on integer data whose first pass (lam = 0, rho = 10) is exact: dyadic maps, constraint levels
    and starts, scales that are powers of two.
      'equality'  one model, its output pinned, the objective a VARIABLE
      'ranges'    three models under a range each: at the start the upper side is active, the lower side is, neither is
                  (the levels are far outside, or inside, whatever the models can reach on the box)
      'tie'       model 0's output is the variable w that model 1 reads: a tie alone
      'both'      a range and a tie on ONE model
      'mapped'    a second reader of two variables through maps with b = 1 / 4 and 1 / 2 (training ranges [-1, 3], [0, 2])
    """
    unit = [[0.0, 1.0]] * 3
    a = int_model([[1, 0, 0], [0, 2, 0], [1, 1, 0], [0, 1, 2], [2, 1, 1]], unit, E, 11)
    b = int_model([[2, 0, 0], [0, 1, 0], [1, 0, 1], [1, 2, 0]], unit, E, 12)
    c = int_model([[1, 0, 0], [0, 1, 0], [2, 2, 0], [0, 0, 3]], unit, E, 13)
    xyz = ['x', 'y', 'z']
    kw = dict(sense='min', constraints=None, scales=None)
    if name == 'equality':
        args = ([a], [xyz], ['u'], 'x')
        kw.update(constraints={'u': (0.25, 0.25)}, scales={'u': 4.0})
    elif name == 'ranges':
        args = ([a, b, c], [xyz, xyz, xyz], ['u', 'v', 'w'], 'u')
        kw.update(constraints={'u': (None, -64.0), 'v': (64.0, None), 'w': (-512.0, 512.0)},
                  scales={'u': 8.0, 'v': 2.0, 'w': 16.0}, sense='max')
    elif name == 'tie':
        second = int_model([[1, 0], [0, 1], [2, 1]], [[0.0, 1.0], [-8.0, 8.0]], E, 14)
        args = ([a, second], [xyz, ['x', 'u']], ['u', 'v'], 'v')
        kw.update(scales={'u': 4.0, 'v': 1.0})
    elif name == 'both':
        second = int_model([[1, 0], [0, 1], [2, 1]], [[0.0, 1.0], [-8.0, 8.0]], E, 14)
        args = ([a, second], [xyz, ['x', 'u']], ['u', 'v'], 'v')
        kw.update(constraints={'u': (-0.5, 1.5)}, scales={'u': 4.0, 'v': 1.0})
    else:
        second = int_model([[1, 0], [0, 2], [2, 1], [1, 1]], [[-1.0, 3.0], [0.0, 2.0]], E, 15)
        args = ([a, second], [xyz, ['x', 'z']], ['u', 'v'], 'v')
        kw.update(constraints={'u': (None, -2.0)}, scales={'u': 2.0, 'v': 1.0})
    p = opt._prepare_system(*args, kw['sense'], kw['constraints'], None, 'paired', 1, 60, SYS_TOL, SYS_CTOL, kw['scales'])
    s, j = np.meshgrid(np.arange(S), np.arange(p['n']), indexing='ij')
    p['starts'] = np.ascontiguousarray(((s * (2 * j + 1) + j * j + s // 9) % 9) / 8.0)
    return p


EXACT_SYSTEMS = ('equality', 'ranges', 'tie', 'both', 'mapped')


def is_dyadic(a):
    a = np.ravel(np.asarray(a, dtype=np.float64)) * 2.0 ** 20
    return bool(np.all(a == np.round(a)))


def system_first_points(p):
    E, S = p['coef'].shape[0], p['starts'].shape[0]
    x0 = np.minimum(np.maximum(p['starts'], p['lo']), p['hi'])
    return np.ascontiguousarray(np.broadcast_to(x0, (E,) + x0.shape).reshape(E * S, -1)), np.repeat(p['coef'], S, axis=0)


def host_system_pass(system, z, coef, lam, rho):
    """The statement's pass at z [B, n]: ev, nz [B, K], L, its sum of magnitudes, viol, measure [B], g [B, n], H [B, h]."""
    e, noise_k = system.values(z, coef)
    L, size, viol, measure, weight, each = system.merit(z, e, noise_k, lam, rho)
    g, H = system.derivatives(z, coef, weight, each, rho)
    return dict(ev=e.T, nz=noise_k.T, F=L, noise=size, viol=viol, measure=measure, g=g.T, H=H.T, each=each)


def fraction_system(p, z, coef, lam, rho):
    """L, g and H of the merit function at ONE point by the formulas of optimize.py's docstring (S2, S3) in exact rational
    arithmetic, with Mg, MH, ML: the same expressions with every quantity replaced by its magnitude."""
    F = Fraction
    n, K = p['n'], p['K']
    offsets = np.concatenate([[0], np.cumsum([mtx.shape[0] + 1 for mtx in p['mtxs']])])
    zf = [F(float(v)) for v in z]
    rho = F(float(rho))
    parts = []
    for k in range(K):
        wide, a, b = opt._expanded(p, k)
        parts.append(fraction_parts(wide, p['table'], z, coef[offsets[k]:offsets[k + 1]], 1.0, 1.0, maps=(a, b)))
    sign = F(float(p['sign']))
    nh = n * (n + 1) // 2
    g, Mg, H, MH = [F(0)] * n, [F(0)] * n, [F(0)] * nh, [F(0)] * nh

    def add(weight, Mweight, k, grad=None, Mgrad=None):
        grad, Mgrad = grad or parts[k]['g'], Mgrad or parts[k]['Mg']
        for j in range(n):
            g[j], Mg[j] = g[j] + weight * grad[j], Mg[j] + Mweight * Mgrad[j]
        for h in range(nh):
            H[h], MH[h] = H[h] + weight * parts[k]['H'][h], MH[h] + Mweight * parts[k]['MH'][h]

    if p['obj_model'] >= 0:
        L, ML = sign * parts[p['obj_model']]['e'], parts[p['obj_model']]['Me']
        add(sign, F(1), p['obj_model'])
    else:
        L, ML = sign * zf[p['obj_var']], abs(zf[p['obj_var']])
        g[p['obj_var']], Mg[p['obj_var']] = g[p['obj_var']] + sign, Mg[p['obj_var']] + 1
    viol = measure = F(0)
    marginal = False
    for i, c in enumerate(p['cons']):
        k, s = c['model'], F(float(c['scale']))
        r, Mr = parts[k]['e'], parts[k]['Me']
        dr, Mdr = list(parts[k]['g']), list(parts[k]['Mg'])
        if c['var'] >= 0:
            tied = F(float(c['offset'])) + F(float(c['span'])) * zf[c['var']]
            r, Mr = r - tied, Mr + abs(F(float(c['offset']))) + abs(F(float(c['span']))) * abs(zf[c['var']])
            dr[c['var']], Mdr[c['var']] = dr[c['var']] - F(float(c['span'])), Mdr[c['var']] + abs(F(float(c['span'])))
        lam_lo, lam_hi = F(float(lam[2 * i])), F(float(lam[2 * i + 1]))
        slope = curve = Mslope = F(0)
        if c['lo'] == c['hi']:
            cc, Mc = (r - F(float(c['lo']))) / s, (Mr + abs(F(float(c['lo'])))) / s
            w, Mw = lam_hi + rho * cc, abs(lam_hi) + rho * Mc
            L, ML = L + lam_hi * cc + rho * cc * cc / 2, ML + abs(lam_hi) * Mc + rho * Mc * Mc / 2
            slope, Mslope, curve = w / s, Mw / s, rho / (s * s)
            viol, measure = max(viol, abs(cc)), max(measure, abs(cc))
        else:
            for side, level, lam_side in ((1, c['hi'], lam_hi), (-1, c['lo'], lam_lo)):
                if not np.isfinite(level):
                    continue
                gs, Mgs = side * (r - F(float(level))) / s, (Mr + abs(F(float(level)))) / s
                arg, Marg = lam_side + rho * gs, abs(lam_side) + rho * Mgs
                marginal = marginal or abs(arg) <= gamma(64) * Marg * 1024   # the side's activity is within rounding
                new = max(F(0), arg)
                L, ML = L + (new * new - lam_side * lam_side) / (2 * rho), ML + (Marg * Marg + lam_side * lam_side) / (2 * rho)
                slope, Mslope = slope + side * new / s, Mslope + Marg / s
                curve = curve + (rho / (s * s) if new > 0 else 0)
                viol, measure = max(viol, gs), max(measure, abs(max(gs, -lam_side / rho)))
        add(slope, Mslope, k, dr, Mdr)
        for a in range(n):
            for b in range(a + 1):
                H[tri(a, b)], MH[tri(a, b)] = H[tri(a, b)] + curve * dr[a] * dr[b], MH[tri(a, b)] + curve * Mdr[a] * Mdr[b]
    return dict(L=L, g=g, H=H, ML=ML, Mg=Mg, MH=MH, viol=viol, measure=measure, marginal=marginal,
                ev=[part['e'] for part in parts], Mev=[part['Me'] for part in parts])


def system_roundings(p):
    """N for the merit function's g and H: a mapped model's 4 p + k + T + 6 (module docstring), the constraint's weight
    -- residual, tie, division by the scale, times rho, plus lam, max, division by the scale: 8 with the residual's own
    error counted through the model's N again --, the rank-one product (3) and the sums over models and constraints."""
    worst = max(roundings(opt._expanded(p, k)[0], mapped=True) for k in range(p['K']))
    return 2 * worst + 8 + 3 + p['K'] + 2 * len(p['cons'])


def check_system_decisions(tr, p, system, k, steepest_in, label=''):
    """``check_decisions`` for a flat trace of the system kernel, and what is the system's own: the merit function, its
    allowance, the violation and the measure from the traced ev, nz, lam and rho by the statement's own operations; the
    update test; the multipliers, the penalty, the inner tolerance and the target at the exit -- all bit for bit."""
    run = tr['running']
    C_ = len(p['cons'])
    x = tr['x_in'][run]
    lam, rho = tr['lam'][run].T, tr['rho'][run]
    with np.errstate(invalid='ignore', over='ignore'):
        L, size, viol, measure, weight, each = system.merit(x, tr['ev'][run].T, tr['nz'][run].T, lam, rho)
    for key, value in (('F', L), ('noise', size), ('viol', viol), ('measure', measure)):
        assert same(tr[key][run], value), (label, key)
    settled = np.zeros(run.shape, dtype=bool)
    settled[run] = (tr['pg'][run] <= p['tol']) & (measure <= p['ctol'])
    # the update test of the solves that run on
    on = run & (tr['status_tests'] == -1)
    update = on & (tr['pg'] <= tr['inner'])
    capped = tr['rho'] >= opt.RHO_MAX
    with np.errstate(invalid='ignore'):
        gives_up = update & ~(tr['measure'] <= tr['target']) & capped & (tr['viol'] > p['ctol'])
        good = (tr['measure'] <= tr['target']) | capped
    update = update & ~gives_up
    reached = ~np.isnan(tr['alpha']) & on                            # (the wavefront went on beyond the tests)
    assert np.array_equal(tr['update'][reached], update[reached]) and np.array_equal(tr['good'][reached], good[reached]), label
    counts = check_decisions(tr, p['lo'], p['hi'], p['tol'], k, p['max_iter'], steepest_in, label, settled=settled,
                             update=update | gives_up)
    new_lam = np.array([side for s in each for side in s[2:]]).reshape(2 * C_, -1).T   # [running, 2 C]
    full = np.full((run.shape[0], 2 * C_), np.nan)
    full[run] = new_lam
    moves, grows = reached & update & good, reached & update & ~good
    stays = reached & ~moves
    assert same(tr['lam_out'][moves], full[moves]) and same(tr['lam_out'][stays], tr['lam'][stays]), label
    assert same(tr['inner_out'][moves], np.maximum(p['tol'], opt.INNER_SHRINK * tr['inner'][moves])), label
    assert same(tr['target_out'][moves], np.maximum(p['ctol'], opt.FEASIBLE_SHRINK * tr['target'][moves])), label
    assert same(tr['inner_out'][stays], tr['inner'][stays]) and same(tr['target_out'][stays], tr['target'][stays]), label
    assert same(tr['rho_out'][grows], np.minimum(opt.RHO_GROWTH * tr['rho'][grows], opt.RHO_MAX)), label
    assert same(tr['rho_out'][reached & ~grows], tr['rho'][reached & ~grows]), label
    assert same(tr['x_out'][reached & update], tr['x_in'][reached & update]), label
    assert np.all(tr['status'][reached & gives_up] == opt.INFEASIBLE), label
    counts.update(update=int((reached & update).sum()), good_update=int(moves.sum()), penalty_update=int(grows.sum()))
    return counts


def host_system_walk(p, max_iter=None):
    """``optimize._solve_system_block`` from the system's first points: its results, and (lam, rho, measure) of every
    evaluation of the merit function it made, iterates and trial points in order."""
    system = opt._System(p)
    merit = system.merit

    def recording(z, e, noise, lam, rho):
        out = merit(z, e, noise, lam, rho)
        recording.calls.append((lam.copy(), np.array(rho, dtype=np.float64).copy(), out[3].copy()))
        return out

    recording.calls = []
    system.merit = recording
    x0, coef = system_first_points(p)
    out = opt._solve_system_block(system, coef, x0, p['max_iter'] if max_iter is None else max_iter)
    return out, recording.calls


def system_ratios(p, x, coef, lam, rho, values):
    """Largest error / bound of ev, F (= L), g and H of ONE solve (`values`: those four) against ``fraction_system``;
    None where a side's activity is within rounding of switching (its rank-one term is then not decided)."""
    ref = fraction_system(p, x, coef, lam, rho)
    if ref['marginal']:
        return None
    N = system_roundings(p)
    return dict(ev=worst_ratio(values['ev'], ref['ev'], ref['Mev'], N), F=worst_ratio(values['F'], ref['L'], ref['ML'], N),
                g=worst_ratio(values['g'], ref['g'], ref['Mg'], N), H=worst_ratio(values['H'], ref['H'], ref['MH'], N))

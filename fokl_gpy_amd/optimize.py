"""
Optimise a fitted model over its whole posterior: a multistart, box-constrained optimiser, one local solve per
(posterior draw, starting point), all solves at once on the device.

A fitted 'Bernoulli Polynomials' model is a polynomial in its normalised inputs,

    model(x) = betas[0] + sum_t betas[t + 1] * prod_j phi_{mtx[t, j]}(x_j)          (phi_0 = 1),

smooth on the box the search is confined to, so every solve is a projected Newton iteration with a safeguard:

  1. value, gradient and Hessian of F = +-model (minus for 'max') from the term table: phi, phi', phi'' of every distinct
     (input, order) factor once per iterate by Horner, then per term the products value, gradient and Hessian need;
  2. stop on the projected gradient, max_j |P(x - g)_j - x_j| <= tol (P clips to the box; normalised coordinates), on
     ``max_iter`` iterations or on a non-finite value;
  3. active set: a coordinate on a bound whose descent direction points outwards, and every fixed coordinate (lo == hi),
     gets the unit row / column in the Hessian and a zero in the right-hand side;
  4. Cholesky of that matrix in place, modified where it is not positive definite: a pivot that is not above
     1e-8 max(1, largest free diagonal) is replaced by its magnitude (at least that floor) -- one factorisation, the same
     loop in every solve, and always a descent direction.  The Newton direction is scaled to at most one box width.
     (The Levenberg retry the design started from needs the unfactored matrix a second time, and 16 inputs leave no room
     for a copy next to the factor.)
  5. halving along the projection arc P(x + alpha d), at most 31 trial points, under the Armijo test
     F(trial) <= F(x) + 1e-4 min(g . (trial - x), 0) + 1e-13 sum_t |term_t|; the last summand is the rounding noise of F
     itself, without it the test is decided by noise next to the optimum.  If no trial passes, the next iteration takes
     the projected steepest-descent direction from the same point; if that fails as well the solve stops as 'stalled':
     no representable decrease is left although the projected gradient is above ``tol``.

``optimize`` runs the solves on the device (``fokl_model_optimize``: one lane per solve; without the library or a gfx950
device it raises, there is no host fallback).  ``optimize_host`` is the same algorithm in numpy with no device: the
STATEMENT the kernel is tested against.  It carries a batch of solves through every numpy operation (each solve sees
exactly the element-wise arithmetic it would see alone) because a Python loop over 32 000 solves is of no use to a test.
The device and the host may differ in the last bits of a sum (the order of the terms differs), which can flip a
line-search test: compare results, not iterates.

Limits, checked before anything is launched: at most 16 inputs; 3 x distinct factors + m (m + 1) / 2 + 3 m values per
solve within the 144 KB of LDS a wavefront of 64 solves gets (the 16-input, 32-factor models fit: 280 of 288); orders
within the table; lo <= hi inside the training range; draws x starts <= 1 048 576 per call.
"""
import numpy as np

from . import getKernels
from .GP_Integrate import bounds_cut, _device_context

MAX_INPUTS = 16
MAX_SOLVES = 1 << 20
MAX_HALVINGS = 30                 # alpha = 1, 1/2, ..., 2**-30: 31 trial points
ARMIJO = 1e-4
NOISE = 1e-13                     # x sum |term|: differences of F below this are rounding
PIVOT_FLOOR = 1e-8                # x max(1, largest free diagonal entry)

CONVERGED, ITERATION_LIMIT, NON_FINITE, STALLED = 0, 1, 2, 3
STATUS_TEXT = {CONVERGED: 'converged', ITERATION_LIMIT: 'iteration limit', NON_FINITE: 'non-finite', STALLED: 'stalled'}

_PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53)


class OptimizeResult(dict):
    """A dict whose entries are also attributes (``res.x``, ``res['x']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def start_points(count, lo, hi):
    """``count`` deterministic low-discrepancy points in the box [lo, hi] (Halton, one prime base per input, indices
    1 .. count): no random generator is involved.  lo, hi [m]; returns [count, m]."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    m = lo.shape[0]
    if m > len(_PRIMES):
        raise ValueError(f"start_points: at most {len(_PRIMES)} inputs")
    unit = np.zeros((int(count), m))
    for j in range(m):
        index = np.arange(1, int(count) + 1)
        scale = 1.0
        while index.any():
            scale /= _PRIMES[j]
            unit[:, j] += scale * (index % _PRIMES[j])
            index = index // _PRIMES[j]
    return np.minimum(np.maximum(lo + (hi - lo) * unit, lo), hi)


def _prepare(betas, mtx, phis, minmax, kernel, sense, objective, bounds, starts, max_iter, tol):
    """Every check and every array the solver needs, in normalised coordinates; touches no device."""
    if kernel in (0, 'Cubic Splines'):
        raise ValueError("optimize handles the 'Bernoulli Polynomials' kernel only: a 'Cubic Splines' model is piecewise "
                         "and is not optimised")
    if kernel not in (1, 'Bernoulli Polynomials') or (len(phis) > 0 and np.ndim(phis[0][0]) != 0):
        raise ValueError("optimize needs the 'Bernoulli Polynomials' kernel and its coefficient table in phis")
    if sense not in ('max', 'min'):
        raise ValueError("sense must be 'max' or 'min'")
    if objective not in ('mean', 'draws'):
        raise ValueError("objective must be 'mean' or 'draws'")
    mtx = np.asarray(mtx)
    if mtx.ndim == 1:
        mtx = mtx[np.newaxis, :]
    if mtx.ndim != 2 or mtx.shape[1] == 0:
        raise ValueError("mtx must be [terms, inputs]")
    mtx = np.ascontiguousarray(mtx, dtype=np.int32)
    n_terms, m = mtx.shape
    if m > MAX_INPUTS:
        raise ValueError(f"optimize handles at most {MAX_INPUTS} inputs, the model has {m}")
    if mtx.min(initial=0) < 0 or mtx.max(initial=0) > len(phis):
        raise ValueError("mtx holds an order outside the coefficient table")
    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim == 1:
        betas = betas[np.newaxis, :]
    if betas.ndim != 2 or betas.shape[0] == 0:
        raise ValueError("betas must be [draws, terms + 1] or [terms + 1]")
    if betas.shape[1] != n_terms + 1:
        raise ValueError(f"betas has {betas.shape[1]} coefficients per draw, mtx describes {n_terms} terms + the constant")
    if objective == 'mean':
        betas = np.mean(betas, axis=0, keepdims=True)
    betas = np.ascontiguousarray(betas)
    if len(minmax) != m:
        raise ValueError(f"minmax describes {len(minmax)} inputs, mtx {m}")
    low = np.array([float(minmax[j][0]) for j in range(m)])
    high = np.array([float(minmax[j][1]) for j in range(m)])
    span = high - low
    if not np.all(span > 0):
        raise ValueError("minmax must have max > min for every input")
    if bounds is None:
        box = np.stack([low, high], axis=1)
        lo, hi = np.zeros(m), np.ones(m)
    else:
        box = np.array(bounds, dtype=np.float64)
        if box.shape != (m, 2) or not np.isfinite(box).all():
            raise ValueError(f"bounds must be [{m}, 2] finite numbers (true scale)")
        if np.any(box[:, 0] > box[:, 1]):
            raise ValueError("bounds: a lower bound is above its upper bound")
        lo, hi = (box[:, 0] - low) / span, (box[:, 1] - low) / span
        if np.any(lo < -1e-12) or np.any(hi > 1 + 1e-12):
            raise ValueError("bounds reach outside the training range (minmax): the model is not extrapolated")
        lo, hi = np.clip(lo, 0.0, 1.0), np.clip(hi, 0.0, 1.0)
        hi = np.where(box[:, 0] == box[:, 1], lo, hi)                 # a fixed input stays fixed after rounding
    if np.ndim(starts) == 0:
        if int(starts) != starts or int(starts) < 1:
            raise ValueError("starts must be a positive count or an array [S, inputs]")
        x0 = start_points(int(starts), lo, hi)
    else:
        user = np.array(starts, dtype=np.float64)
        if user.ndim == 1:
            user = user[np.newaxis, :]
        if user.ndim != 2 or user.shape[1] != m or user.shape[0] == 0 or not np.isfinite(user).all():
            raise ValueError(f"starts must be a positive count or finite numbers [S, {m}] (true scale)")
        x0 = np.minimum(np.maximum((user - low) / span, lo), hi)      # a start outside the box begins on its face
    x0 = np.ascontiguousarray(x0)
    if betas.shape[0] * x0.shape[0] > MAX_SOLVES:
        raise ValueError(f"{betas.shape[0]} draws x {x0.shape[0]} starts: one call runs at most {MAX_SOLVES} solves")
    if int(max_iter) != max_iter or int(max_iter) < 0:
        raise ValueError("max_iter must be a non-negative integer")
    if not (tol >= 0):
        raise ValueError("tol must be >= 0")
    table, n_basis, width = getKernels.pack_phis(phis, getKernels.KERNEL_BERNOULLI)
    return dict(betas=betas, mtx=mtx, table=table, n_basis=n_basis, width=width, lo=np.ascontiguousarray(lo),
                hi=np.ascontiguousarray(hi), starts=x0, sign=-1.0 if sense == 'max' else 1.0, max_iter=int(max_iter),
                tol=float(tol), low=low, span=span, box=box, objective=objective)


def _assemble(p, x_all, f_all, it_all, st_all, ReturnBounds, ReturnAll):
    """The best start of every draw, true-scale coordinates and, over the draws, the mean and the order statistics."""
    E, S = f_all.shape
    key = np.where(np.isfinite(f_all) & (st_all != NON_FINITE), p['sign'] * f_all, np.inf)
    best = np.argmin(key, axis=1)
    rows = np.arange(E)

    def true_scale(xn):
        out = p['low'] + xn * p['span']
        out = np.where(xn == p['lo'], p['box'][:, 0], out)            # a point on a face of the box is ON it
        return np.where(xn == p['hi'], p['box'][:, 1], out)

    x, f, status = true_scale(x_all[rows, best]), f_all[rows, best], st_all[rows, best]
    res = OptimizeResult()
    if p['objective'] == 'mean':
        res.update(x=x[0], f=float(f[0]), status=int(status[0]))
    else:
        res.update(x=x, f=f, status=status)
        if ReturnBounds and E >= 2:
            cut = bounds_cut(E)
            xs, fs = np.sort(x, axis=0), np.sort(f)
            res.update(x_mean=x.mean(axis=0), f_mean=float(f.mean()),
                       x_bounds=np.stack([xs[cut], xs[E - cut]], axis=1), f_bounds=np.array([fs[cut], fs[E - cut]]))
    if ReturnAll:
        res.update(x_all=true_scale(x_all), f_all=f_all, iterations_all=it_all, status_all=st_all, best_start=best)
    return res


_SIGNATURE = """
    sense       : 'max' | 'min'
    objective   : 'draws' -- one optimum per row of betas (the posterior of the optimum); 'mean' -- one objective, the
                  model with betas averaged over its rows (what ``evaluate`` returns as the mean)
    bounds      : [m, 2] in true scale (default: the training range, ``minmax``); lo == hi fixes an input; a box
                  outside the training range is refused
    starts      : a count -- that many deterministic low-discrepancy points of the box (``start_points``; numpy's random
                  stream is not touched) -- or an array [S, m] of starting points in true scale
    max_iter, tol : iteration limit of a solve; projected-gradient tolerance (in normalised coordinates)
    ReturnBounds : for 'draws' with at least two draws also x_mean [m], f_mean, x_bounds [m, 2], f_bounds [2] over the
                  draws' optima: order statistics (sorted[cut], sorted[E - cut]), cut = ``bounds_cut(E)`` as in ``evaluate``
    ReturnAll   : also every solve: x_all [E, S, m], f_all, iterations_all, status_all [E, S], best_start [E]

    Returns an ``OptimizeResult`` (a dict with attribute access): x, f, status -- the best of all starts, [E, m], [E], [E]
    for 'draws' and [m], scalar, scalar for 'mean'; x in true scale, f in the model's output scale; status 0 converged,
    1 iteration limit, 2 non-finite, 3 stalled (``STATUS_TEXT``).  A solve that ended non-finite is never the best."""


def optimize(betas, mtx, phis, minmax, kernel='Bernoulli Polynomials', sense='max', objective='draws', bounds=None,
             starts=32, max_iter=60, tol=1e-10, ReturnBounds=True, ReturnAll=False, device=None):
    """Where is the model largest (smallest), for every posterior draw?  draws x starts local solves on the device.

    betas       : [E, terms + 1] (rows are draws as ``fit`` returns them) or [terms + 1]
    mtx, phis, minmax, kernel : the model's (``FoKL.optimize`` passes its own)
    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare(betas, mtx, phis, minmax, kernel, sense, objective, bounds, starts, max_iter, tol)
    ctx = _device_context(device)
    x_all, f_all, it_all, st_all = ctx.model_optimize(p['mtx'], p['betas'], p['table'], p['lo'], p['hi'], p['starts'],
                                                      p['sign'], p['max_iter'], p['tol'])
    return _assemble(p, x_all, f_all, it_all, st_all, ReturnBounds, ReturnAll)


def optimize_host(betas, mtx, phis, minmax, kernel='Bernoulli Polynomials', sense='max', objective='draws', bounds=None,
                  starts=32, max_iter=60, tol=1e-10, ReturnBounds=True, ReturnAll=False):
    """``optimize`` with the solves in numpy on this host: the statement of the algorithm (module docstring), for tests
    and for reading.  Same arguments, same result fields."""
    p = _prepare(betas, mtx, phis, minmax, kernel, sense, objective, bounds, starts, max_iter, tol)
    return _assemble(p, *solve_host(p['mtx'], p['betas'], p['table'], p['lo'], p['hi'], p['starts'], p['sign'],
                                    p['max_iter'], p['tol']), ReturnBounds, ReturnAll)


optimize.__doc__ += _SIGNATURE
optimize_host.__doc__ += _SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# the host statement
# ---------------------------------------------------------------------------------------------------------

class TermTable:
    """The model as the solver reads it: the distinct (input, order) factors, and per term its factors' slots in
    ascending input order.  Padded to the widest term with a slot that holds (1, 0, 0) on a dummy input."""

    def __init__(self, mtx):
        n_terms, m = mtx.shape
        slot_of, self.src, self.order, rows = {}, [], [], []
        for t in range(n_terms):
            row = []
            for j in range(m):
                order = int(mtx[t, j])
                if order:
                    if (j, order) not in slot_of:
                        slot_of[(j, order)] = len(self.src)
                        self.src.append(j)
                        self.order.append(order)
                    row.append(slot_of[(j, order)])
            rows.append(row)
        self.m, self.n_terms, self.n_slots = m, n_terms, len(self.src)
        self.width = max([len(r) for r in rows] + [1])
        self.slots = np.full((n_terms, self.width), self.n_slots, dtype=np.intp)
        inputs = np.full((n_terms, self.width), m, dtype=np.intp)
        for t, row in enumerate(rows):
            self.slots[t, :len(row)] = row
            inputs[t, :len(row)] = [self.src[s] for s in row]
        self.n_hess = m * (m + 1) // 2
        # 0 / 1 matrices that add a term's contribution to its gradient / Hessian entry (the last row collects padding)
        self.to_grad = np.zeros((self.width, m + 1, n_terms))
        self.to_hess = np.zeros((self.width, self.width, self.n_hess + 1, n_terms))
        for t in range(n_terms):
            for a in range(self.width):
                ja = inputs[t, a]
                self.to_grad[a, ja, t] = 1.0
                for b in range(a + 1):
                    jb = inputs[t, b]
                    self.to_hess[a, b, self.n_hess if ja == m else ja * (ja + 1) // 2 + jb, t] = 1.0


def _evaluate(tt, table, x, coef, sign, level):
    """F = sign * model at x [B, m] with coefficients coef [B, terms + 1]: (F [B], sum |term| [B]) and with level 2 also
    the gradient [m, B] and the Hessian's lower triangle [m (m + 1) / 2, B] (entry i (i + 1) / 2 + j, j <= i)."""
    B = x.shape[0]
    fac = np.empty((tt.n_slots + 1, 3, B))
    fac[tt.n_slots] = np.array([1.0, 0.0, 0.0])[:, None]
    for s in range(tt.n_slots):
        c = table[tt.order[s] - 1]
        xs = x[:, tt.src[s]]
        value = np.full(B, c[tt.order[s]])
        slope = np.zeros(B)
        bend = np.zeros(B)
        for k in range(tt.order[s] - 1, -1, -1):                     # Horner, three rows at once
            bend = bend * xs + slope
            slope = slope * xs + value
            value = value * xs + c[k]
        fac[s, 0], fac[s, 1], fac[s, 2] = value, slope, 2.0 * bend
    w = sign * coef[:, 1:].T                                         # [terms, B]
    A = fac[tt.slots, 0]                                             # [terms, width, B]
    product = A[:, 0].copy()
    for i in range(1, tt.width):
        product = product * A[:, i]
    each = w * product
    F = sign * coef[:, 0] + each.sum(axis=0)
    noise = np.abs(sign * coef[:, 0]) + np.abs(each).sum(axis=0)
    if level == 0:
        return F, noise
    D1, D2 = fac[tt.slots, 1], fac[tt.slots, 2]

    def others(skip):
        out = np.ones((tt.n_terms, B))
        for i in range(tt.width):
            if i not in skip:
                out = out * A[:, i]
        return out

    grad = np.zeros((tt.m + 1, B))
    hess = np.zeros((tt.n_hess + 1, B))
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(tt.width):
            rest = w * others((a,))
            grad += tt.to_grad[a] @ (rest * D1[:, a])
            hess += tt.to_hess[a, a] @ (rest * D2[:, a])
            for b in range(a):
                hess += tt.to_hess[a, b] @ (w * others((a, b)) * D1[:, a] * D1[:, b])
    return F, noise, grad[:tt.m], hess[:tt.n_hess]


def _direction(H, g, active):
    """The modified-Cholesky Newton direction of every solve: H [m (m + 1) / 2, B] is factored in place."""
    m, B = g.shape
    at = lambda i, j: i * (i + 1) // 2 + j
    free_diag = np.zeros(B)
    for j in range(m):
        free_diag = np.where(active[j], free_diag, np.maximum(free_diag, np.abs(H[at(j, j)])))
    floor = PIVOT_FLOOR * np.maximum(1.0, free_diag)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(m):
            for j in range(i + 1):
                s = np.where(active[i] | active[j], 1.0 if i == j else 0.0, H[at(i, j)])
                for k in range(j):
                    s = s - H[at(i, k)] * H[at(j, k)]
                if j < i:
                    H[at(i, j)] = s / H[at(j, j)]
                else:
                    s = np.where(s > floor, s, np.fmax(np.abs(s), floor))
                    H[at(i, i)] = np.sqrt(s)
        d = np.empty((m, B))
        for i in range(m):
            s = np.where(active[i], 0.0, -g[i])
            for k in range(i):
                s = s - H[at(i, k)] * d[k]
            d[i] = s / H[at(i, i)]
        for i in range(m - 1, -1, -1):
            s = d[i]
            for k in range(i + 1, m):
                s = s - H[at(k, i)] * d[k]
            d[i] = s / H[at(i, i)]
    return d


def _solve_block(tt, table, coef, lo, hi, x, sign, max_iter, tol):
    B, m = x.shape
    x = x.copy()
    status = np.full(B, -1, dtype=np.int32)                          # -1: running
    iterations = np.zeros(B, dtype=np.int32)
    f_end = np.full(B, np.nan)
    steepest = np.zeros(B, dtype=bool)
    fixed = (lo == hi)[:, None]
    lo_c, hi_c = lo[:, None], hi[:, None]
    for it in range(max_iter + 1):
        running = status < 0
        if not running.any():
            break
        F, noise, g, H = _evaluate(tt, table, x, coef, sign, 2)
        xt = x.T                                                     # [m, B]
        with np.errstate(invalid='ignore', over='ignore'):
            pg = np.max(np.abs(np.minimum(np.maximum(xt - g, lo_c), hi_c) - xt), axis=0)
            finite = np.isfinite(F) & np.isfinite(g).all(axis=0)

        def stop(which, code):
            which = which & (status < 0)
            status[which], iterations[which], f_end[which] = code, it, F[which]

        stop(~finite, NON_FINITE)
        stop(pg <= tol, CONVERGED)
        if it == max_iter:
            stop(np.ones(B, dtype=bool), ITERATION_LIMIT)
            break
        running = status < 0
        if not running.any():
            break
        with np.errstate(invalid='ignore', over='ignore'):
            active = fixed | ((xt <= lo_c) & (g > 0)) | ((xt >= hi_c) & (g < 0))
            d = _direction(H, g, active)
            reach = np.max(np.abs(d), axis=0)
            use_steepest = steepest | ~(reach <= np.finfo(np.float64).max)
            d = np.where(use_steepest, np.where(active, 0.0, -g), d)
            reach = np.max(np.abs(d), axis=0)
            d = np.where(reach > 1.0, d / reach, d)
            alpha = np.ones(B)
            searching = running.copy()
            for _ in range(MAX_HALVINGS + 1):
                if not searching.any():
                    break
                trial = np.minimum(np.maximum(xt + alpha * d, lo_c), hi_c)
                Ft, _ = _evaluate(tt, table, np.ascontiguousarray(trial.T), coef, sign, 0)
                step = trial - xt
                slope = np.zeros(B)
                for j in range(m):
                    slope = slope + g[j] * step[j]
                ok = (Ft <= F + ARMIJO * np.minimum(slope, 0.0) + NOISE * noise) & (np.max(np.abs(step), axis=0) > 0)
                take = searching & ok
                x[take] = trial.T[take]
                searching = searching & ~ok
                alpha = np.where(searching, alpha * 0.5, alpha)
        failed = searching                                           # no trial point passed
        stop(failed & use_steepest, STALLED)
        steepest = failed & ~use_steepest
    return x, sign * f_end, iterations, status


def solve_host(mtx, betas, table, lo, hi, starts, sign, max_iter, tol):
    """Every (draw, start) solve in normalised coordinates -- the arguments and the results of
    ``DeviceContext.model_optimize``: x [E, S, m], model value [E, S], iterations [E, S], status [E, S]."""
    tt = TermTable(mtx)
    E, S, m = betas.shape[0], starts.shape[0], mtx.shape[1]
    x0 = np.broadcast_to(starts, (E, S, m)).reshape(E * S, m)
    coef = np.repeat(betas, S, axis=0)
    block = int(max(64, min(4096, 12_000_000 // max(1, tt.n_terms * tt.width))))
    x = np.empty((E * S, m))
    f = np.empty(E * S)
    iterations = np.empty(E * S, dtype=np.int32)
    status = np.empty(E * S, dtype=np.int32)
    for b0 in range(0, E * S, block):
        part = slice(b0, min(b0 + block, E * S))
        x[part], f[part], iterations[part], status[part] = _solve_block(tt, table, coef[part], lo, hi, x0[part], sign,
                                                                        max_iter, tol)
    return x.reshape(E, S, m), f.reshape(E, S), iterations.reshape(E, S), status.reshape(E, S)

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
STATEMENT the kernel is tested against.  Step 1 is ``_model_parts`` and steps 3-5 are ``_newton_step``, for this solver
and for the system solver below alike -- as both kernels have them from ``csrc/fokl_optimize_core.inc``.  It carries a batch of solves through every numpy operation (each solve sees
exactly the element-wise arithmetic it would see alone) because a Python loop over 32 000 solves is of no use to a test.
The device and the host may differ in the last bits of a sum (the order of the terms differs), which can flip a
line-search test, so whole solves are compared by their results.  Iterates are compared one iteration at a time
(``DeviceContext.model_optimize(..., trace_iteration=k)`` / ``system_optimize(p, trace_iteration=k)``: the product kernels
write what iteration k saw and decided): the values against exact references -- integer data, where the order of a sum
does not matter, bit for bit; the real table against rational arithmetic within a derived rounding bound -- and the
decisions against the traced values themselves: ``_step_direction``, ``_armijo`` and ``_constraint`` on the device's own
F, g, H and trial values must give the device's factor, direction, trial count, step and update bit for bit
(tests/optimize_step_cases.py).

Limits, checked before anything is launched: at most 16 inputs; 3 x distinct factors + m (m + 1) / 2 + 3 m values per
solve within the 144 KB of LDS a wavefront of 64 solves gets (the 16-input, 32-factor models fit: 280 of 288); orders
within the table; lo <= hi inside the training range; draws x starts <= 1 048 576 per call.

A SYSTEM of models -- ``optimize_system`` (device: ``fokl_system_optimize``) and its statement ``optimize_system_host``.
Several fitted models in one problem: the output of one may be an input of another (an *intermediate*), an output may
be pinned to a value or held inside a range, and the objective is one model's output or one variable.  This is what
the reference's ``fokl_to_pyomo`` export is used for; here every posterior draw is solved, from every start, by a
bound-constrained augmented Lagrangian whose inner iteration is the projected Newton step above:

  S1. Common coordinates.  The decision variables are the distinct names of ``xvars`` in order of first appearance.  A
      variable lives in the normalised coordinate z of the FIRST model that reads it; its box [lo, hi] inside [0, 1] is
      the intersection of its ``bounds`` entry with the training range of every model that reads it.  Another model k
      that reads it as input j sees a_kj + b_kj z in its own normalised coordinate (a = 0, b = 1 for the first reader):
      its phi' picks up b, its phi'' b**2.  The maps belong to the problem, not to a solve.  ``tol`` is measured in these
      coordinates.  An intermediate's tie model_k(x) - x_name = 0 is written in true scale (x_name = min + span z): its
      gradient has -span in that variable's place.  A variable that is the objective enters as its z (the optimum is the
      same; f and the multipliers are reported in true scale).
  S2. Merit function L(z; lam, rho) = sign * objective + sum_i psi_i (Powell-Hestenes-Rockafellar): lam c + rho / 2 c**2
      for an equality c = 0, (max(0, lam + rho g)**2 - lam**2) / (2 rho) for each present side g <= 0 of a range; c and
      g are residuals divided by the constraint's scale (``scales``; default the mean over the draws of sum_t |beta_t| of
      its model: from the coefficients, never from the iterates).
  S3. One VALUE pass over the models (the constraints' weights need the values), then one DERIVATIVE pass: grad L =
      sum_i w_i grad c_i and hess L = sum_i w_i hess c_i + rho sum_active grad c_i grad c_i^T with w_i = lam_i + rho c_i
      (max(0, lam + rho g) for a side, 0 when it is inactive).  Each model's Hessian terms are formed already weighted by
      d L / d (its output); its plain gradient is kept whole for the rank-one terms.
  S4. ONE loop over iterations (no nested outer / inner loop).  An iteration evaluates L, its gradient and Hessian, then:
      converged if the projected gradient of L is <= tol and the measure is <= ctol, where the measure is the largest
      scaled residual |c|, or for a side |max(g, -lam / rho)| (violation, or distance of its multiplier from
      complementarity); else, if the projected gradient is <= the current inner tolerance, an UPDATE and no step (the
      iterate stays; the update counts as an iteration): where the measure is <= the current feasibility target the
      multipliers take their first-order values (lam + rho c; max(0, lam + rho g)), the inner tolerance shrinks by 1e-2
      towards tol and the target by 1e-1 towards ctol (first values 1e-2 and 1e-1); otherwise rho <- 10 rho (first
      value 10).  rho is capped at 1e10: an update that finds the target missed at the cap ends the solve as infeasible
      if its violation is above ctol, and updates the multipliers otherwise.  Else steps 3-5 above on L, unchanged: active
      set, modified Cholesky, arc search with the rounding allowance 1e-13 x (sum |terms| of the objective + sum_i |d L /
      d c_i| sum |terms| of c_i), steepest-descent fall-back.  With no constraint the inner tolerance is tol from the
      start, and the loop is ``optimize``'s, iterate for iterate.
  S5. A solve ends converged, at ``max_iter``, non-finite or stalled as above; one that ended at the limit or stalled with
      a violation above ctol is reported as 4, infeasible.  The reported multipliers are the first-order values at the
      end point (the weights w_i of S3, per unit of the unscaled output): >= 0 where the upper side or the equality pushes
      down, <= 0 for the lower side, exactly 0 for an inactive side.  The best start of a draw is its best feasible one.

Limits of a system, checked before anything is launched and again by the native entry point: at most 16 decision
variables and 8 models; per solve 3 F + n (n + 1) / 2 + 3 n + 2 K + 2 C values in LDS (F the most distinct (input,
order) factors any ONE model has -- the models are evaluated one after the other through the same rows --, n variables,
K models, C constraints with the ties) within the same 288 (144 KB a wavefront); draws x starts <= 1 048 576.  The
solves are sliced over launches of at most 4 194 304 / max_iter solves (``ITERATION_CAP``).  When the objective is
orders of magnitude larger than the scaled constraints the multipliers are large and the updates many; ``scales`` is
the handle.
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


def _true_scale(xn, offset, span, lo, hi, box):
    """Normalised points xn [..., n] in true scale; a point on a face of the box [n, 2] is ON it."""
    out = offset + xn * span
    out = np.where(xn == lo, box[:, 0], out)
    return np.where(xn == hi, box[:, 1], out)


def _over_draws(x, f):
    """The mean and the order statistics over the draws' optima x [E, n], f [E]."""
    E = f.shape[0]
    cut = bounds_cut(E)
    xs, fs = np.sort(x, axis=0), np.sort(f)
    return dict(x_mean=x.mean(axis=0), f_mean=float(f.mean()), x_bounds=np.stack([xs[cut], xs[E - cut]], axis=1),
                f_bounds=np.array([fs[cut], fs[E - cut]]))


def _assemble(p, x_all, f_all, it_all, st_all, ReturnBounds, ReturnAll):
    """The best start of every draw, true-scale coordinates and, over the draws, the mean and the order statistics."""
    E, S = f_all.shape
    key = np.where(np.isfinite(f_all) & (st_all != NON_FINITE), p['sign'] * f_all, np.inf)
    best = np.argmin(key, axis=1)
    rows = np.arange(E)
    true_scale = lambda xn: _true_scale(xn, p['low'], p['span'], p['lo'], p['hi'], p['box'])
    x, f, status = true_scale(x_all[rows, best]), f_all[rows, best], st_all[rows, best]
    res = OptimizeResult()
    if p['objective'] == 'mean':
        res.update(x=x[0], f=float(f[0]), status=int(status[0]))
    else:
        res.update(x=x, f=f, status=status)
        if ReturnBounds and E >= 2:
            res.update(_over_draws(x, f))
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


def _model_parts(tt, table, z, coef, level, scale=1.0, weight=None, maps=None):
    """Step 1 for one model at z [B, n] with coefficients coef [B, terms + 1]: e = scale x its value [B] and sum |term|
    [B]; with level 2 also scale x its gradient [n, B] and ``weight`` (a number, or [B]) x its Hessian's lower triangle
    [n (n + 1) / 2, B] (entry i (i + 1) / 2 + j, j <= i).  scale is +-1: the plain value and gradient or their exact
    negatives.  With maps = (a, b) [n] each the model reads a + b z and the derivatives are with respect to z; without,
    it reads z itself (no 0 + 1 * z)."""
    B = z.shape[0]
    fac = np.empty((tt.n_slots + 1, 3, B))
    fac[tt.n_slots] = np.array([1.0, 0.0, 0.0])[:, None]
    for s in range(tt.n_slots):
        c = table[tt.order[s] - 1]
        v = tt.src[s]
        xs = z[:, v] if maps is None else maps[0][v] + maps[1][v] * z[:, v]
        value = np.full(B, c[tt.order[s]])
        slope = np.zeros(B)
        bend = np.zeros(B)
        for k in range(tt.order[s] - 1, -1, -1):                     # Horner, three rows at once
            bend = bend * xs + slope
            slope = slope * xs + value
            value = value * xs + c[k]
        if maps is None:
            fac[s, 0], fac[s, 1], fac[s, 2] = value, slope, 2.0 * bend
        else:
            fac[s, 0], fac[s, 1], fac[s, 2] = value, slope * maps[1][v], 2.0 * bend * (maps[1][v] * maps[1][v])
    w = scale * coef[:, 1:].T                                        # [terms, B]
    A = fac[tt.slots, 0]                                             # [terms, width, B]
    product = A[:, 0].copy()
    for i in range(1, tt.width):
        product = product * A[:, i]
    each = w * product
    e = scale * coef[:, 0] + each.sum(axis=0)
    noise = np.abs(scale * coef[:, 0]) + np.abs(each).sum(axis=0)
    if level == 0:
        return e, noise
    D1, D2 = fac[tt.slots, 1], fac[tt.slots, 2]
    wh = weight * coef[:, 1:].T

    def others(skip):
        out = np.ones((tt.n_terms, B))
        for i in range(tt.width):
            if i not in skip:
                out = out * A[:, i]
        return out

    grad = np.zeros((tt.m + 1, B))
    hess = np.zeros((tt.n_hess + 1, B))
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(tt.width):
            rest = others((i,))
            grad += tt.to_grad[i] @ (w * rest * D1[:, i])
            hess += tt.to_hess[i, i] @ (wh * rest * D2[:, i])
            for j in range(i):
                hess += tt.to_hess[i, j] @ (wh * others((i, j)) * D1[:, i] * D1[:, j])
    return e, noise, grad[:tt.m], hess[:tt.n_hess]


def _evaluate(tt, table, x, coef, sign, level):
    """F = sign * model at x [B, m]: (F, sum |term|) and with level 2 also its gradient and Hessian triangle."""
    return _model_parts(tt, table, x, coef, level, scale=sign, weight=sign)


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


def _active_set(xt, g, lo_c, hi_c):
    """Step 3: the fixed coordinates and those on a bound whose descent direction points outwards; xt, g [m, B]."""
    with np.errstate(invalid='ignore'):
        return (lo_c == hi_c) | ((xt <= lo_c) & (g > 0)) | ((xt >= hi_c) & (g < 0))


def _step_direction(x, g, H, lo, hi, steepest):
    """Steps 3 and 4 at the iterates x [B, m]: the active set [m, B], the direction d [m, B] -- the modified-Cholesky
    Newton direction (H is factored in place), projected steepest descent where ``steepest`` asks for it or the Newton
    direction is not finite, scaled to at most one box width -- and which of the two it is."""
    xt = x.T                                                         # [m, B]
    lo_c, hi_c = lo[:, None], hi[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        active = _active_set(xt, g, lo_c, hi_c)
        d = _direction(H, g, active)
        reach = np.max(np.abs(d), axis=0)
        use_steepest = steepest | ~(reach <= np.finfo(np.float64).max)
        d = np.where(use_steepest, np.where(active, 0.0, -g), d)
        reach = np.max(np.abs(d), axis=0)
        d = np.where(reach > 1.0, d / reach, d)
    return active, d, use_steepest


def _armijo(Ft, F, noise, g, step):
    """Step 5's test of the trial points x + step (step [m, B], already projected): the decrease with its rounding
    allowance, and that the point moved at all."""
    slope = np.zeros(F.shape[0])
    for j in range(step.shape[0]):
        slope = slope + g[j] * step[j]
    return (Ft <= F + ARMIJO * np.minimum(slope, 0.0) + NOISE * noise) & (np.max(np.abs(step), axis=0) > 0)


def _arc_search(x, F, noise, g, d, lo, hi, stepping, merit_at):
    """Step 5 for the solves ``stepping``: halving along the projection arc; x moves in place where a trial point
    passes.  Returns which solves found none."""
    B, m = x.shape
    xt = x.T
    lo_c, hi_c = lo[:, None], hi[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        alpha = np.ones(B)
        searching = stepping.copy()
        for _ in range(MAX_HALVINGS + 1):
            if not searching.any():
                break
            trial = np.minimum(np.maximum(xt + alpha * d, lo_c), hi_c)
            Ft = merit_at(np.ascontiguousarray(trial.T))
            ok = _armijo(Ft, F, noise, g, trial - xt)
            take = searching & ok
            x[take] = trial.T[take]
            searching = searching & ~ok
            alpha = np.where(searching, alpha * 0.5, alpha)
    return searching


def _newton_step(x, F, noise, g, H, lo, hi, stepping, steepest, merit_at):
    """Steps 3-5 for the solves ``stepping`` [B] at the iterates x [B, m], where the merit is F [B] (sum of magnitudes
    ``noise``) with gradient g [m, B] and Hessian triangle H (factored in place); ``merit_at(points)`` is the merit at
    trial points [B, m].  x moves in place where a trial point passes.  Returns (failed, use_steepest): no trial point
    passed; the direction was projected steepest descent (asked for by ``steepest``, or the Newton one was not finite)."""
    _, d, use_steepest = _step_direction(x, g, H, lo, hi, steepest)
    return _arc_search(x, F, noise, g, d, lo, hi, stepping, merit_at), use_steepest


def _solve_block(tt, table, coef, lo, hi, x, sign, max_iter, tol):
    B, m = x.shape
    x = x.copy()
    status = np.full(B, -1, dtype=np.int32)                          # -1: running
    iterations = np.zeros(B, dtype=np.int32)
    f_end = np.full(B, np.nan)
    steepest = np.zeros(B, dtype=bool)
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
        failed, use_steepest = _newton_step(x, F, noise, g, H, lo, hi, running, steepest,
                                            lambda trial: _evaluate(tt, table, trial, coef, sign, 0)[0])
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


# ---------------------------------------------------------------------------------------------------------
# a system of models: constraints on outputs, fixed outputs, one model's output as another's input
# ---------------------------------------------------------------------------------------------------------

MAX_VARIABLES = MAX_INPUTS
MAX_MODELS = 8
LDS_ROWS = 288                    # values per solve: 144 KB of LDS, 64 solves wide, 8 bytes each
ITERATION_CAP = 1 << 22           # solves x max_iter asked of one launch (the native entry point slices by it)
RHO_START, RHO_GROWTH, RHO_MAX = 10.0, 10.0, 1e10
INNER_START, INNER_SHRINK = 1e-2, 1e-2       # tolerance of the inner problem: first value, factor per update
FEASIBLE_START, FEASIBLE_SHRINK = 1e-1, 1e-1  # feasibility target: first value, factor per multiplier update

INFEASIBLE = 4
STATUS_TEXT[INFEASIBLE] = 'infeasible'


def _model_fields(model, k):
    if isinstance(model, dict):
        missing = [key for key in ('betas', 'mtx', 'phis', 'minmax', 'kernel') if key not in model]
        if missing:
            raise ValueError(f"models[{k}] lacks {missing}")
        return model
    missing = [key for key in ('betas', 'mtx', 'phis', 'minmax', 'kernel') if not hasattr(model, key)]
    if missing:
        raise ValueError(f"models[{k}] is not a fitted model: it has no {missing}")
    return {key: getattr(model, key) for key in ('betas', 'mtx', 'phis', 'minmax', 'kernel')}


def system_lds_rows(n_factors, n_vars, n_models, n_constraints):
    """Values a solve keeps in LDS: 3 x the most distinct (input, order) factors any ONE model has (the models are
    evaluated one after the other through the same rows) + the Hessian's triangle + iterate, gradient and direction
    + per model its value and the sum of its terms' magnitudes + two multipliers per constraint."""
    return 3 * n_factors + n_vars * (n_vars + 1) // 2 + 3 * n_vars + 2 * n_models + 2 * n_constraints


def _prepare_system(models, xvars, yvars, objective, sense, constraints, bounds, draws, starts, max_iter, tol, ctol,
                    scales):
    """Every check and every array ``solve_system_host`` and the device need; touches no device."""
    models = [_model_fields(model, k) for k, model in enumerate(models)]
    K = len(models)
    if K == 0 or K > MAX_MODELS:
        raise ValueError(f"optimize_system handles 1 to {MAX_MODELS} models, not {K}")
    if len(xvars) != K or len(yvars) != K:
        raise ValueError("xvars and yvars need one entry per model")
    for k, model in enumerate(models):
        kernel = model['kernel']
        if kernel in (0, 'Cubic Splines'):
            raise ValueError(f"models[{k}]: optimize_system handles the 'Bernoulli Polynomials' kernel only: a 'Cubic "
                             f"Splines' model is piecewise and is not optimised")
        if kernel not in (1, 'Bernoulli Polynomials') or (len(model['phis']) > 0 and np.ndim(model['phis'][0][0]) != 0):
            raise ValueError(f"models[{k}]: optimize_system needs the 'Bernoulli Polynomials' kernel and its coefficient "
                             f"table in phis")
    if sense not in ('max', 'min'):
        raise ValueError("sense must be 'max' or 'min'")
    if draws not in ('paired', 'mean'):
        raise ValueError("draws must be 'paired' or 'mean'")
    yvars = [str(name) for name in yvars]
    if len(set(yvars)) != K:
        raise ValueError("yvars: every model needs an output name of its own")
    xvars = [[str(name) for name in names] for names in xvars]
    variables = []
    for names in xvars:
        if len(set(names)) != len(names):
            raise ValueError(f"xvars: a model reads a name twice: {names}")
        variables += [name for name in names if name not in variables]
    n = len(variables)
    if n > MAX_VARIABLES:
        raise ValueError(f"optimize_system handles at most {MAX_VARIABLES} decision variables, the system has {n}")
    index = {name: v for v, name in enumerate(variables)}

    # ---- the models: terms, coefficients, the affine map of every input into the common coordinates ----
    tables = [getKernels.pack_phis(model['phis'], getKernels.KERNEL_BERNOULLI) for model in models]
    table, n_basis, width = max(tables, key=lambda t: t[1])
    vmin, vspan = np.zeros(n), np.zeros(n)
    true_lo, true_hi = np.full(n, -np.inf), np.full(n, np.inf)
    mtxs, betas, var_of, shift, slope = [], [], [], [], []
    for k, model in enumerate(models):
        if not np.array_equal(tables[k][0], table[:tables[k][1], :tables[k][2]]):
            raise ValueError(f"models[{k}]: its coefficient table (phis) differs from the other models'")
        mtx = np.asarray(model['mtx'])
        if mtx.ndim == 1:
            mtx = mtx[np.newaxis, :]
        if mtx.ndim != 2 or mtx.shape[1] == 0:
            raise ValueError(f"models[{k}]: mtx must be [terms, inputs]")
        mtx = np.ascontiguousarray(mtx, dtype=np.int32)
        if mtx.shape[1] != len(xvars[k]):
            raise ValueError(f"models[{k}] has {mtx.shape[1]} inputs, xvars[{k}] names {len(xvars[k])}")
        if mtx.min(initial=0) < 0 or mtx.max(initial=0) > tables[k][1]:
            raise ValueError(f"models[{k}]: mtx holds an order outside the coefficient table")
        b = np.asarray(model['betas'], dtype=np.float64)
        if b.ndim == 1:
            b = b[np.newaxis, :]
        if b.ndim != 2 or b.shape[0] == 0:
            raise ValueError(f"models[{k}]: betas must be [draws, terms + 1] or [terms + 1]")
        if b.shape[1] != mtx.shape[0] + 1:
            raise ValueError(f"models[{k}]: betas has {b.shape[1]} coefficients per draw, mtx describes {mtx.shape[0]} "
                             f"terms + the constant")
        if draws == 'mean':
            b = np.mean(b, axis=0, keepdims=True)
        minmax = model['minmax']
        if len(minmax) != mtx.shape[1]:
            raise ValueError(f"models[{k}]: minmax describes {len(minmax)} inputs, mtx {mtx.shape[1]}")
        low = np.array([float(minmax[j][0]) for j in range(mtx.shape[1])])
        span = np.array([float(minmax[j][1]) for j in range(mtx.shape[1])]) - low
        if not np.all(span > 0):
            raise ValueError(f"models[{k}]: minmax must have max > min for every input")
        vs = np.array([index[name] for name in xvars[k]], dtype=np.int32)
        a_k, b_k = np.zeros(len(vs)), np.ones(len(vs))
        for j, v in enumerate(vs):
            if vspan[v] == 0:                                          # the first reader: its coordinate is the common one
                vmin[v], vspan[v] = low[j], span[j]
            else:
                a_k[j], b_k[j] = (vmin[v] - low[j]) / span[j], vspan[v] / span[j]
            true_lo[v], true_hi[v] = max(true_lo[v], low[j]), min(true_hi[v], low[j] + span[j])
        mtxs.append(mtx)
        betas.append(np.ascontiguousarray(b))
        var_of.append(vs)
        shift.append(a_k)
        slope.append(b_k)
    rows = sorted({b.shape[0] for b in betas} - {1})
    if len(rows) > 1:
        raise ValueError(f"draws='paired' needs the same number of draws in every model (or one row, which is shared): "
                         f"the models have {[b.shape[0] for b in betas]}")
    E = rows[0] if rows else 1
    coef = np.ascontiguousarray(np.concatenate([np.broadcast_to(b, (E, b.shape[1])) for b in betas], axis=1))

    # ---- the box ----
    bounds = dict(bounds or {})
    fixed = np.zeros(n, dtype=bool)
    for name, pair in bounds.items():
        if name not in index:
            raise ValueError(f"bounds: '{name}' is not a decision variable ({variables})")
        lo_b, hi_b = pair
        if lo_b is not None and hi_b is not None and float(lo_b) > float(hi_b):
            raise ValueError(f"bounds['{name}']: the lower bound {lo_b} is above the upper bound {hi_b}")
        v = index[name]
        for side in (lo_b, hi_b):
            if side is not None and not np.isfinite(float(side)):
                raise ValueError(f"bounds['{name}'] must be finite numbers or None")
        if lo_b is not None:
            true_lo[v] = max(true_lo[v], float(lo_b))
        if hi_b is not None:
            true_hi[v] = min(true_hi[v], float(hi_b))
        fixed[v] = lo_b is not None and hi_b is not None and float(lo_b) == float(hi_b)
    for v, name in enumerate(variables):
        if true_lo[v] > true_hi[v]:
            raise ValueError(f"variable '{name}': its bounds and the training ranges of the models that read it have no "
                             f"point in common (lower {true_lo[v]}, upper {true_hi[v]})")
    lo = np.clip((true_lo - vmin) / vspan, 0.0, 1.0)
    hi = np.clip((true_hi - vmin) / vspan, 0.0, 1.0)
    hi = np.where(fixed, lo, hi)                                       # a fixed variable stays fixed after rounding
    box = np.stack([true_lo, true_hi], axis=1)

    # ---- objective and constraints ----
    objective = str(objective)
    if objective in yvars:
        obj_model, obj_var = yvars.index(objective), -1
    elif objective in index:
        obj_model, obj_var = -1, index[objective]
    else:
        raise ValueError(f"objective '{objective}' is neither a model output ({yvars}) nor a decision variable ({variables})")
    constraints = dict(constraints or {})
    for name, pair in constraints.items():
        if name not in yvars:
            raise ValueError(f"constraints: '{name}' is not a model output ({yvars})")
        lo_c, hi_c = pair
        if lo_c is not None and hi_c is not None and float(lo_c) > float(hi_c):
            raise ValueError(f"constraints['{name}']: the lower limit {lo_c} is above the upper limit {hi_c}")
    scales = dict(scales or {})
    for name, value in scales.items():
        if name not in yvars:
            raise ValueError(f"scales: '{name}' is not a model output ({yvars})")
        if not (float(value) > 0 and np.isfinite(float(value))):
            raise ValueError(f"scales['{name}'] must be a positive number")
    cons = []                                                          # ordered by model; a model's tie comes last
    for k, name in enumerate(yvars):
        size = float(np.mean(np.sum(np.abs(betas[k]), axis=1)))        # from the coefficients, never from the iterates
        scale = float(scales.get(name, size if size > 0 and np.isfinite(size) else 1.0))
        if name in constraints:
            lo_c, hi_c = constraints[name]
            lo_c = -np.inf if lo_c is None else float(lo_c)
            hi_c = np.inf if hi_c is None else float(hi_c)
            if np.isnan(lo_c) or np.isnan(hi_c) or lo_c == np.inf or hi_c == -np.inf:
                raise ValueError(f"constraints['{name}'] must be numbers or None")
            if lo_c > -np.inf or hi_c < np.inf:
                cons.append(dict(name=name, model=k, var=-1, lo=lo_c, hi=hi_c, scale=scale, offset=0.0, span=0.0))
        if name in index:                                              # an intermediate: model_k(x) - x_name = 0, true scale
            v = index[name]
            cons.append(dict(name='tie:' + name, model=k, var=v, lo=0.0, hi=0.0, scale=scale, offset=vmin[v],
                             span=vspan[v]))

    # ---- starts, limits ----
    if np.ndim(starts) == 0:
        if int(starts) != starts or int(starts) < 1:
            raise ValueError("starts must be a positive count or an array [S, variables]")
        x0 = start_points(int(starts), lo, hi)
    else:
        user = np.array(starts, dtype=np.float64)
        if user.ndim == 1:
            user = user[np.newaxis, :]
        if user.ndim != 2 or user.shape[1] != n or user.shape[0] == 0 or not np.isfinite(user).all():
            raise ValueError(f"starts must be a positive count or finite numbers [S, {n}] (true scale, columns {variables})")
        x0 = np.minimum(np.maximum((user - vmin) / vspan, lo), hi)
    x0 = np.ascontiguousarray(x0)
    if E * x0.shape[0] > MAX_SOLVES:
        raise ValueError(f"{E} draws x {x0.shape[0]} starts: one call runs at most {MAX_SOLVES} solves")
    if int(max_iter) != max_iter or int(max_iter) < 0:
        raise ValueError("max_iter must be a non-negative integer")
    if not (tol >= 0) or not (ctol >= 0):
        raise ValueError("tol and ctol must be >= 0")
    n_factors = max(len({(j, int(o)) for row in mtx for j, o in enumerate(row) if o}) for mtx in mtxs)
    need = system_lds_rows(n_factors, n, K, len(cons))
    if need > LDS_ROWS:
        raise ValueError(f"the system needs {need} values per solve in LDS (3 x {n_factors} factors of its largest model + "
                         f"{n * (n + 1) // 2} Hessian entries + 3 x {n} + 2 x {K} models + 2 x {len(cons)} multipliers), "
                         f"a wavefront's {LDS_ROWS * 512 // 1024} KB hold {LDS_ROWS}")
    return dict(n=n, K=K, E=E, variables=variables, yvars=yvars, mtxs=mtxs, coef=coef, var_of=var_of, shift=shift,
                slope=slope, table=table, n_basis=n_basis, width=width, lo=np.ascontiguousarray(lo),
                hi=np.ascontiguousarray(hi), box=box, vmin=vmin, vspan=vspan, starts=x0,
                sign=-1.0 if sense == 'max' else 1.0, obj_model=obj_model, obj_var=obj_var, cons=cons,
                max_iter=int(max_iter), tol=float(tol), ctol=float(ctol), draws=draws)


def _assemble_system(p, out, ReturnBounds, ReturnAll):
    """The best FEASIBLE start of every draw (the least violating one where there is none), true-scale coordinates
    and, over the draws, the mean and the order statistics."""
    x_all, f_all, viol_all, y_all, mu_all, it_all, st_all = out
    E, S = f_all.shape
    if p['obj_var'] >= 0:                                             # the solver's objective was the normalised coordinate
        mu_all = mu_all * p['vspan'][p['obj_var']]
    finite = np.isfinite(f_all) & np.isfinite(viol_all) & (st_all != NON_FINITE)
    feasible = finite & (viol_all <= p['ctol'])
    key = np.where(feasible, p['sign'] * f_all, np.inf)
    best = np.argmin(key, axis=1)
    none = ~feasible.any(axis=1)
    best = np.where(none, np.argmin(np.where(finite, viol_all, np.inf), axis=1), best)
    rows = np.arange(E)

    true_scale = lambda xn: _true_scale(xn, p['vmin'], p['vspan'], p['lo'], p['hi'], p['box'])
    if p['obj_var'] >= 0:
        f_all = true_scale(x_all)[..., p['obj_var']]
    x, f, status = true_scale(x_all[rows, best]), f_all[rows, best], st_all[rows, best]
    y, mu, violation = y_all[rows, best], mu_all[rows, best], viol_all[rows, best]
    names = [c['name'] for c in p['cons']]
    res = OptimizeResult()
    one = p['draws'] == 'mean'
    pick = (lambda a: a[0]) if one else (lambda a: a)
    res.update(x={name: pick(x[:, v]) for v, name in enumerate(p['variables'])}, x_array=pick(x),
               y={name: pick(y[:, k]) for k, name in enumerate(p['yvars'])},
               f=float(f[0]) if one else f, violation=float(violation[0]) if one else violation,
               multipliers={name: pick(mu[:, i]) for i, name in enumerate(names)},
               status=int(status[0]) if one else status, variables=list(p['variables']), constraint_names=names)
    if not one and ReturnBounds and E >= 2:
        res.update(_over_draws(x, f))
    if ReturnAll:
        res.update(x_all=true_scale(x_all), f_all=f_all, violation_all=viol_all, y_all=y_all, multipliers_all=mu_all,
                   iterations_all=it_all, status_all=st_all, best_start=best)
    return res


_SYSTEM_SIGNATURE = """
    models      : fitted ``FoKL`` objects, or dicts with betas, mtx, phis, minmax, kernel ('Bernoulli Polynomials' only)
    xvars, yvars : per model the names its input columns read, and the name of its output (``fokl_to_pyomo``'s
                  meaning).  The decision variables are the distinct names of xvars in order of first appearance; a
                  yvar that is also an xvar is an intermediate, tied to its model by model_k(x) - x_name = 0
    objective   : a yvar or an xvar name;  sense 'max' | 'min'
    constraints : {yvar: (lo, hi)} in the model's output scale; None for a missing side; lo == hi pins the output
    bounds      : {variable: (lo, hi)} in true scale; lo == hi fixes it.  A variable's box is this intersected with the
                  training range of every model that reads it; an empty intersection is refused
    draws       : 'paired' -- solve e uses row e of every model's betas (equal row counts, or one row, which is shared);
                  'mean' -- every model with its rows averaged, one problem
    starts      : a count (``start_points`` over the variables' boxes; numpy's random stream is not touched) or an
                  array [S, variables] in true scale
    max_iter    : Newton iterations of a solve over all its multiplier / penalty rounds (an update counts as one)
    tol, ctol   : projected gradient of the merit function (common normalised coordinates); largest scaled residual
    scales      : {yvar: positive number} the residuals of that output's constraint and tie are divided by.  Default:
                  the mean over the draws of sum_t |betas[t]| of that model -- from the coefficients, never the iterates
    ReturnBounds, ReturnAll : as for ``optimize``

    Returns an ``OptimizeResult``: x {variable: [E]} and x_array [E, n] (true scale, columns ``variables``), y {yvar:
    [E]} every model's value there, f [E] the objective, violation [E] the largest scaled constraint residual,
    multipliers {constraint: [E]} (keys: the constrained yvar, 'tie:' + name for an intermediate; d merit / d output:
    positive where the upper side or the equality pushes down, negative for the lower side, 0 for an inactive side; in
    units of sign * objective per unit of the output), status [E]: 0 converged, 1 iteration limit, 2 non-finite,
    3 stalled, 4 infeasible (the solve ended with violation > ctol).  The best start of a draw is its best FEASIBLE
    one; a draw with none reports status 4 and its least-violating point.  With draws='mean' the arrays lose the
    draw axis.  ReturnBounds adds x_mean, f_mean, x_bounds [n, 2], f_bounds [2]; ReturnAll x_all [E, S, n], f_all,
    violation_all, y_all [E, S, models], multipliers_all [E, S, constraints], iterations_all, status_all, best_start."""


def optimize_system(models, xvars, yvars, objective, sense='max', constraints=None, bounds=None, draws='paired',
                    starts=32, max_iter=200, tol=1e-9, ctol=1e-8, scales=None, ReturnBounds=True, ReturnAll=False,
                    device=None):
    """Optimise over a SYSTEM of fitted models, for every posterior draw: constraints on outputs, pinned outputs, one
    model's output as another's input.  draws x starts constrained local solves on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_system(models, xvars, yvars, objective, sense, constraints, bounds, draws, starts, max_iter, tol, ctol,
                        scales)
    ctx = _device_context(device)
    return _assemble_system(p, ctx.system_optimize(p), ReturnBounds, ReturnAll)


def optimize_system_host(models, xvars, yvars, objective, sense='max', constraints=None, bounds=None, draws='paired',
                         starts=32, max_iter=200, tol=1e-9, ctol=1e-8, scales=None, ReturnBounds=True, ReturnAll=False):
    """``optimize_system`` with the solves in numpy on this host: the statement of the algorithm (module docstring),
    for tests and for reading.  Same arguments, same result fields."""
    p = _prepare_system(models, xvars, yvars, objective, sense, constraints, bounds, draws, starts, max_iter, tol, ctol,
                        scales)
    return _assemble_system(p, solve_system_host(p), ReturnBounds, ReturnAll)


optimize_system.__doc__ += _SYSTEM_SIGNATURE
optimize_system_host.__doc__ += _SYSTEM_SIGNATURE


def _expanded(p, k):
    """Model k's term table over the system's variables (column v holds the order of the input that reads variable v):
    the factors of a term are then in ascending VARIABLE order, which is how the kernel lists them."""
    wide = np.zeros((p['mtxs'][k].shape[0], p['n']), dtype=np.int32)
    wide[:, p['var_of'][k]] = p['mtxs'][k]
    a, b = np.zeros(p['n']), np.ones(p['n'])
    a[p['var_of'][k]], b[p['var_of'][k]] = p['shift'][k], p['slope'][k]
    return wide, a, b


def _constraint(c, r, lam_lo, lam_hi, rho):
    """One constraint at residual r [B] (the output, minus the tied variable's value for a tie): its summand of the merit
    function, d merit / d r, the weight of its rank-one Hessian term, its scaled violation, the measure the updates and
    the convergence test use (the violation, or for a side that holds how far its multiplier still is from
    complementarity: |max(g, -lam / rho)|), and the multipliers a first-order update gives (lower side, upper side or
    equality)."""
    s = c['scale']
    zero = np.zeros_like(r)
    if c['lo'] == c['hi']:
        cc = (r - c['lo']) / s
        w = lam_hi + rho * cc
        return lam_hi * cc + 0.5 * rho * cc * cc, w / s, rho / (s * s) + zero, np.abs(cc), np.abs(cc), lam_lo, w
    psi, slope, curve, viol, measure, new_lo, new_hi = zero, zero, zero, zero, zero, lam_lo, lam_hi
    if c['hi'] < np.inf:
        g = (r - c['hi']) / s
        new_hi = np.maximum(0.0, lam_hi + rho * g)
        psi = psi + (new_hi * new_hi - lam_hi * lam_hi) / (2.0 * rho)
        slope = slope + new_hi / s
        curve = curve + np.where(new_hi > 0.0, rho / (s * s), 0.0)
        viol = np.maximum(viol, g)
        measure = np.maximum(measure, np.abs(np.maximum(g, -lam_hi / rho)))
    if c['lo'] > -np.inf:
        g = (c['lo'] - r) / s
        new_lo = np.maximum(0.0, lam_lo + rho * g)
        psi = psi + (new_lo * new_lo - lam_lo * lam_lo) / (2.0 * rho)
        slope = slope - new_lo / s
        curve = curve + np.where(new_lo > 0.0, rho / (s * s), 0.0)
        viol = np.maximum(viol, g)
        measure = np.maximum(measure, np.abs(np.maximum(g, -lam_lo / rho)))
    return psi, slope, curve, viol, measure, new_lo, new_hi


class _System:
    """The system as the host statement reads it: per model the expanded term table and the maps."""

    def __init__(self, p):
        self.p = p
        self.parts = []
        self.offsets = np.concatenate([[0], np.cumsum([mtx.shape[0] + 1 for mtx in p['mtxs']])])
        for k in range(p['K']):
            wide, a, b = _expanded(p, k)
            self.parts.append((TermTable(wide), a, b))

    def values(self, z, coef):
        """Every model's value [K, B] and sum |term| [K, B] at z [B, n]."""
        out = [_model_parts(tt, self.p['table'], z, coef[:, self.offsets[k]:self.offsets[k + 1]], 0, maps=(a, b))
               for k, (tt, a, b) in enumerate(self.parts)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])

    def merit(self, z, e, noise, lam, rho):
        """L, its rounding allowance's sum of magnitudes, the violation, the convergence measure, d L / d (model value)
        [K, B], per constraint (d L / d r, rank-one weight, updated multipliers)."""
        p = self.p
        B = z.shape[0]
        weight = np.zeros((p['K'], B))
        if p['obj_model'] >= 0:
            L = p['sign'] * e[p['obj_model']]
            size = noise[p['obj_model']].copy()
            weight[p['obj_model']] = p['sign']
        else:
            value = z[:, p['obj_var']]                                 # a variable: its normalised coordinate
            L, size = p['sign'] * value, np.abs(value)
        viol, measure = np.zeros(B), np.zeros(B)
        each = []
        for i, c in enumerate(p['cons']):
            r, reach = e[c['model']], noise[c['model']]
            if c['var'] >= 0:
                tied = c['offset'] + c['span'] * z[:, c['var']]
                r, reach = r - tied, reach + np.abs(tied)
            psi, slope, curve, v, far, new_lo, new_hi = _constraint(c, r, lam[2 * i], lam[2 * i + 1], rho)
            L = L + psi
            size = size + np.abs(slope) * reach
            viol, measure = np.maximum(viol, v), np.maximum(measure, far)
            weight[c['model']] = weight[c['model']] + slope
            each.append((slope, curve, new_lo, new_hi))
        return L, size, viol, measure, weight, each

    def derivatives(self, z, coef, weight, each, rho):
        """Gradient [n, B] and Hessian triangle of L at z from every model's plain gradient and weighted Hessian."""
        p = self.p
        n, B = p['n'], z.shape[0]
        at = lambda i, j: i * (i + 1) // 2 + j
        g, H = np.zeros((n, B)), np.zeros((n * (n + 1) // 2, B))
        if p['obj_var'] >= 0:
            g[p['obj_var']] += p['sign']
        with np.errstate(invalid='ignore', over='ignore'):
            for k, (tt, a, b) in enumerate(self.parts):
                _, _, gm, Hk = _model_parts(tt, p['table'], z, coef[:, self.offsets[k]:self.offsets[k + 1]], 2,
                                            weight=weight[k], maps=(a, b))
                H += Hk
                g += weight[k] * gm
                plain = np.zeros(B)
                for i, c in enumerate(p['cons']):
                    if c['model'] == k and c['var'] < 0:
                        plain = plain + each[i][1]
                ranks = [(plain, None)] + [(each[i][1], c) for i, c in enumerate(p['cons'])
                                           if c['model'] == k and c['var'] >= 0]
                for curve, c in ranks:
                    if c is not None:                                  # the tie: its residual's gradient has -span at the variable
                        g[c['var']] += each[p['cons'].index(c)][0] * (-c['span'])
                        gm = gm.copy()
                        gm[c['var']] = gm[c['var']] - c['span']
                    for i in range(n):
                        for j in range(i + 1):
                            H[at(i, j)] += curve * gm[i] * gm[j]
        return g, H


def _solve_system_block(system, coef, x, max_iter):
    p = system.p
    lo, hi, sign, tol, ctol = p['lo'], p['hi'], p['sign'], p['tol'], p['ctol']
    B, n = x.shape
    C = len(p['cons'])
    x = x.copy()
    status = np.full(B, -1, dtype=np.int32)
    iterations = np.zeros(B, dtype=np.int32)
    steepest = np.zeros(B, dtype=bool)
    lam = np.zeros((2 * C, B))
    rho = np.full(B, RHO_START)
    inner = np.full(B, max(tol, INNER_START) if C else tol)
    target = np.full(B, max(ctol, FEASIBLE_START))
    lo_c, hi_c = lo[:, None], hi[:, None]
    for it in range(max_iter + 1):
        running = status < 0
        if not running.any():
            break
        e, noise_k = system.values(x, coef)
        F, noise, viol, measure, weight, each = system.merit(x, e, noise_k, lam, rho)
        g, H = system.derivatives(x, coef, weight, each, rho)
        xt = x.T
        with np.errstate(invalid='ignore', over='ignore'):
            pg = np.max(np.abs(np.minimum(np.maximum(xt - g, lo_c), hi_c) - xt), axis=0)
            finite = np.isfinite(F) & np.isfinite(g).all(axis=0)

        def stop(which, code):
            which = which & (status < 0)
            status[which], iterations[which] = code, it

        stop(~finite, NON_FINITE)
        stop((pg <= tol) & (measure <= ctol), CONVERGED)
        if it == max_iter:
            stop(np.ones(B, dtype=bool), ITERATION_LIMIT)
            break
        # the inner problem is solved to its tolerance: multipliers or penalty move, the iterate does not
        update = (status < 0) & (pg <= inner)
        capped = rho >= RHO_MAX                                      # no larger penalty: give up where the point is infeasible
        stop(update & ~(measure <= target) & capped & (viol > ctol), INFEASIBLE)
        update = update & (status < 0)
        good = (measure <= target) | capped
        for i in range(C):
            lam[2 * i] = np.where(update & good, each[i][2], lam[2 * i])
            lam[2 * i + 1] = np.where(update & good, each[i][3], lam[2 * i + 1])
        inner = np.where(update & good, np.maximum(tol, INNER_SHRINK * inner), inner)
        target = np.where(update & good, np.maximum(ctol, FEASIBLE_SHRINK * target), target)
        rho = np.where(update & ~good, np.minimum(RHO_GROWTH * rho, RHO_MAX), rho)
        running = (status < 0) & ~update
        if not running.any():
            continue

        def merit_at(trial):
            et, nt = system.values(trial, coef)
            return system.merit(trial, et, nt, lam, rho)[0]

        failed, use_steepest = _newton_step(x, F, noise, g, H, lo, hi, running, steepest, merit_at)
        stop(failed & use_steepest, STALLED)
        steepest = failed & ~use_steepest
    # the results at the end point: objective, violation, every model's value, first-order multipliers
    e, noise_k = system.values(x, coef)
    _, _, viol, _, _, each = system.merit(x, e, noise_k, lam, rho)
    if p['obj_model'] >= 0:
        f = e[p['obj_model']].copy()
    else:
        f = x[:, p['obj_var']].copy()
    with np.errstate(invalid='ignore'):
        status = np.where(np.isin(status, (ITERATION_LIMIT, STALLED)) & ~(viol <= ctol), INFEASIBLE, status)
    mu = np.array([s[0] for s in each]).reshape(C, B)
    return x, f, viol, e.T, mu.T, iterations, status.astype(np.int32)


def solve_system_host(p):
    """Every (draw, start) solve of a prepared system in the common normalised coordinates -- the results of
    ``DeviceContext.system_optimize``: x [E, S, n], objective [E, S], violation [E, S], model values [E, S, K],
    multipliers [E, S, C], iterations [E, S], status [E, S]."""
    system = _System(p)
    E, S, n, K, C = p['E'], p['starts'].shape[0], p['n'], p['K'], len(p['cons'])
    x0 = np.broadcast_to(p['starts'], (E, S, n)).reshape(E * S, n)
    coef = np.repeat(p['coef'], S, axis=0)
    work = sum(tt.n_terms * tt.width for tt, _, _ in system.parts)
    block = int(max(64, min(4096, 12_000_000 // max(1, work))))
    x, f, viol = np.empty((E * S, n)), np.empty(E * S), np.empty(E * S)
    y, mu = np.empty((E * S, K)), np.empty((E * S, C))
    iterations, status = np.empty(E * S, dtype=np.int32), np.empty(E * S, dtype=np.int32)
    for b0 in range(0, E * S, block):
        part = slice(b0, min(b0 + block, E * S))
        x[part], f[part], viol[part], y[part], mu[part], iterations[part], status[part] = \
            _solve_system_block(system, coef[part], x0[part], p['max_iter'])
    return (x.reshape(E, S, n), f.reshape(E, S), viol.reshape(E, S), y.reshape(E, S, K), mu.reshape(E, S, C),
            iterations.reshape(E, S), status.reshape(E, S))

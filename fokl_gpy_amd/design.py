"""
Choose the next measurements: greedy optimal design over a pool of candidate inputs.

After ``score`` or ``propagate`` shows a fitted model to be too uncertain somewhere, which points should be measured next?
Once ``mtx`` is fixed the model is linear in ``betas``, so the classical answer is exact.  With X the basis values of the
training inputs (ones first), G = X'X and tau^2 the prior scale of the coefficients,

  A0 = G + I / tau^2            the information about betas (in units of 1 / sigma^2) before any new point
  C  = A^-1                     sigma^2 C is the posterior covariance of betas
  v_s = x_s' C x_s              the predictive variance (over sigma^2) at pool row s; measuring it turns A into A + x_s x_s'
                                and log det A grows by log(1 + v_s)
  M  = X_T' X_T / rows(X_T)     the Gram of a TARGET population, so that mean over the target of x' C x = trace(M C)
  w_s = x_s' (C M C) x_s        measuring row s lowers that mean by w_s / (1 + v_s)

  criterion='variance'   greedy D-optimal: pick argmax_s v_s; the gain of a pick is v*, its information log(1 + v*)
  criterion='ivr'        integrated variance reduction (I-optimal): pick argmax_s w_s / (1 + v_s)

A pick x* with u = C x*, a = (C M C) x*, v* = x*' u, w* = x*' a, d = 1 + v* changes (Sherman-Morrison)

  C   <- C - u u' / d
  CMC <- CMC - (u a' + a u') / d + u u' w* / d^2
  v_s <- v_s - p_s^2 / d,   w_s <- w_s - 2 p_s q_s / d + p_s^2 w* / d^2      with p_s = x_s' u, q_s = x_s' a

``refresh_every=r``: before the picks r, 2 r, ... v and w are formed again from the current C and CMC instead of
downdated (0: never), which bounds the drift of the downdates.  Ties go to the lowest pool index; NaN never wins.
``replicates=False`` masks a picked row, ``True`` lets a row be taken again (a noisy measurement repeated is a legitimate
design).  sigma^2 changes no pick: its posterior mean only scales ``target_var``.  Nothing is drawn at random.

``design`` runs the columns (K1), the two Grams (K2) and the selection (``fokl_design_select``,
csrc/fokl_design_device.inc: three kernels, no host round trip between the picks) on the device; without the library or a
gfx950 device it raises, there is no host fallback.  ``design_host`` is the same function in numpy with no device: the
STATEMENT the kernels are tested against (``select_host``).  They share ``_prepare`` (every check; touches no device), the
inverse and the assembly, and differ only in who forms columns and Grams and who selects.
"""
import os

import numpy as np

from . import _capi
from . import getKernels
from .embedded import basis_matrix, _kernel_id

MAX_COLUMNS = _capi.DESIGN_MAX_COLUMNS
CRITERIA = ('variance', 'ivr')
SPARE_BYTES = 64 << 20


class DesignResult(dict):
    """A dict whose entries are also attributes (``res.index``, ``res['index']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def quadratic_forms(X, C, block=1 << 16):
    """x_s' C x_s for every row of X, in blocks of rows."""
    out = np.empty(X.shape[0])
    for r0 in range(0, X.shape[0], block):
        Xb = X[r0:r0 + block]
        out[r0:r0 + block] = np.einsum('sj,sj->s', Xb @ C, Xb)
    return out


def select_host(X, C0, CMC0=None, picks=1, replicates=False, refresh_every=64, keep=False):
    """The statement of ``fokl_design_select``: X [S, nc] the pool's columns, C0 and (for 'ivr') CMC0 [nc, nc] ->
    dict(index [picks] int64, gain, vstar [picks], x [picks, nc], v and w [S] after the last pick with ``keep``, else None).
    A pick that finds no row (all masked, or every criterion NaN) has index -1, gain -inf, x* = 0 and so v* = 0.

    On integer data (X, C0, CMC0 small integers, every sum below 2^53) the device returns the same BITS for the first pick
    (index, gain, v*, x*), the first downdate (v and w of every row with ``picks=1, keep=True``) and the second pick's index
    and gain: up to there every sum is exact in any order, and the divisions that follow are written alike on both sides.
    After a pick C and CMC are no longer integer, the two sides sum in different orders, and everything later (the second
    v*, later picks' gains, a refresh) is equal to rounding (tests/test_design_select_gpu.py)."""
    X = np.asarray(X, dtype=np.float64)
    S, nc = X.shape
    C = np.array(C0, dtype=np.float64)
    ivr = CMC0 is not None
    K = np.array(CMC0, dtype=np.float64) if ivr else None
    mask = np.zeros(S, dtype=bool)
    index = np.full(picks, -1, dtype=np.int64)
    gain, vstar, xs = np.zeros(picks), np.zeros(picks), np.zeros((picks, nc))
    v = w = None
    u, a, d, wstar = np.zeros(nc), np.zeros(nc), 1.0, 0.0

    def downdate(v, w):
        p = X @ u
        v = v - p * p / d
        if ivr:
            q = X @ a
            w = w - 2.0 * p * q / d + p * p * wstar / (d * d)
        return v, w

    for k in range(picks):
        if k == 0 or (refresh_every > 0 and k % refresh_every == 0):
            v = quadratic_forms(X, C)
            w = quadratic_forms(X, K) if ivr else None
        else:
            v, w = downdate(v, w)
        with np.errstate(all='ignore'):
            crit = w / (1.0 + v) if ivr else v.copy()
        crit[mask | np.isnan(crit)] = -np.inf
        i = int(np.argmax(crit))                                 # the first of the largest: the lowest index
        gain[k] = crit[i]
        x = X[i] if crit[i] > -np.inf else np.zeros(nc)
        if crit[i] > -np.inf:
            index[k] = i
            if not replicates:
                mask[i] = True
        xs[k] = x
        u = C @ x
        vstar[k] = x @ u
        d = 1.0 + vstar[k]
        C = C - np.outer(u, u) / d
        if ivr:
            a = K @ x
            wstar = x @ a
            K = K - (np.outer(u, a) + np.outer(a, u)) / d + np.outer(u, u) * (wstar / (d * d))
    if keep:
        v, w = downdate(v, w)
    return dict(index=index, gain=gain, vstar=vstar, x=xs, v=v if keep else None, w=w if keep and ivr else None)


def information_inverse(G, inv_tausqd):
    """C0 = (G + I / tau^2)^-1 from the eigenpairs of G (``eigh_canonical``, as ``resample`` forms them)."""
    from .engine import eigh_canonical
    lamb, Q = eigh_canonical(np.asarray(G, dtype=np.float64))
    C0 = (Q / (lamb + inv_tausqd)) @ Q.T
    return 0.5 * (C0 + C0.T)


def _prepare(mtx, phis, kernel, inputs, pool, picks, criterion, target, inv_tausqd, sigsqd_mean, replicates, refresh_every,
             keep):
    """Every check of ``design`` / ``design_host`` (ValueError) and the arguments in the form both use.  Touches no device."""
    kid = _kernel_id(kernel)
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}")
    if keep not in (None, 'variance'):
        raise ValueError("keep must be None or 'variance'")
    if inv_tausqd is None:
        raise ValueError("design needs tau^2, the prior scale of the coefficients, and a fit alone keeps none: pass what "
                         "resample returned (post = model.resample(...); model.design(post, ...)) or tausqd= as a number")
    inv_tausqd = float(inv_tausqd)
    if not np.isfinite(inv_tausqd) or inv_tausqd <= 0.0:
        raise ValueError("tausqd must be positive and finite")
    sigsqd_mean = float(sigsqd_mean)
    if mtx is None:
        raise ValueError("design needs a fitted model: call fit first (there is no interaction matrix mtx)")
    if inputs is None:
        raise ValueError("design needs the fitted model's training inputs [n, M]")
    inputs = np.asarray(inputs, dtype=np.float64)
    if inputs.ndim == 1:
        inputs = inputs[:, np.newaxis]
    if inputs.ndim != 2 or inputs.shape[0] < 1:
        raise ValueError("the training inputs must be [n, M] with at least one row")
    M = inputs.shape[1]
    mtx = np.asarray(mtx)
    mtx = mtx.reshape(0, M) if mtx.size == 0 else np.atleast_2d(mtx)
    if mtx.ndim != 2 or mtx.shape[1] != M:
        raise ValueError(f"the training inputs have {M} columns, the interaction matrix has {mtx.shape[-1]}")
    if np.any(mtx < 0) or np.any(mtx > len(phis)):
        raise ValueError(f"the interaction matrix holds orders outside the table of {len(phis)} basis functions")
    nc = mtx.shape[0] + 1
    if nc > MAX_COLUMNS:
        raise ValueError(f"the model has {nc} columns (terms + 1), design takes at most {MAX_COLUMNS} (a 16-row tile of basis "
                         f"values in LDS: 96 KiB)")
    if pool is None:
        raise ValueError("pool [S, M] is needed: the candidate inputs to choose from")
    pool = np.asarray(pool, dtype=np.float64)
    if pool.ndim == 1:
        pool = pool[:, np.newaxis]
    if pool.ndim != 2 or pool.shape[0] < 1 or pool.shape[1] != M:
        raise ValueError(f"pool must be [S, {M}] with at least one row")
    S = pool.shape[0]
    if int(picks) != picks or int(picks) < 1:
        raise ValueError("picks must be an integer >= 1")
    picks = int(picks)
    if picks > S and not replicates:
        raise ValueError(f"{picks} picks from a pool of {S} rows: at most {S} without replicates=True")
    if int(refresh_every) != refresh_every or int(refresh_every) < 0:
        raise ValueError("refresh_every must be an integer >= 0 (0: never)")
    bad = ~np.isfinite(pool).all(axis=1)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} of the {S} pool rows are NaN or infinite (the first is row {int(np.flatnonzero(bad)[0])})")
    if not np.isfinite(inputs).all():
        raise ValueError("the training inputs must be finite")
    own_target = criterion == 'ivr' and target is None
    if criterion == 'ivr':
        if target is None:
            target = inputs
        target = np.asarray(target, dtype=np.float64)
        if target.ndim == 1 and target.size:
            target = target[:, np.newaxis]
        if target.size == 0 or target.shape[0] < 1:
            raise ValueError("criterion='ivr' needs a target population with at least one row (target=None: the training inputs)")
        if target.ndim != 2 or target.shape[1] != M or not np.isfinite(target).all():
            raise ValueError(f"target must be [rows, {M}] and finite")
    else:
        target = None
    splines = kid == getKernels.KERNEL_SPLINES
    for name, arr in (('pool', pool), ('target', target), ('training inputs', inputs)):
        if splines and arr is not None and (arr.min() < 0.0 or arr.max() > 1.0):
            raise ValueError(f"the {name} are not normalized correctly: they must lie in [0, 1] (clean=True normalises them)")
    cap = os.environ.get('FOKL_DESIGN_FREE_BYTES')
    need = 8 * S * (M + nc + 3) + 16 * nc * nc
    if cap is not None and need + SPARE_BYTES > int(cap):
        raise ValueError(f"a pool of {S} rows wants {need} bytes on the device (inputs, {nc} columns, v, w and the mask per row) "
                         f"and 64 MiB to spare, FOKL_DESIGN_FREE_BYTES counts {int(cap)} as free: select from the pool in parts")
    return dict(kid=kid, mtx=mtx.astype(np.int32), phis=phis, kernel=kernel, inputs=np.ascontiguousarray(inputs),
                pool=np.ascontiguousarray(pool), target=None if target is None else np.ascontiguousarray(target), S=S, M=M,
                nc=nc, picks=picks, own_target=own_target, criterion=criterion, ivr=criterion == 'ivr', inv_tausqd=inv_tausqd,
                sigsqd_mean=sigsqd_mean, replicates=bool(replicates), refresh_every=int(refresh_every), keep=keep)


class _HostSide:
    """Columns, Grams and the selection in numpy: what ``design_host`` puts in the place of the device."""

    def __init__(self, p):
        self.p = p

    def columns(self, x):
        p = self.p
        return basis_matrix(x, p['mtx'], p['phis'], p['kernel']) if p['mtx'].shape[0] else np.ones((x.shape[0], 1))

    def gram(self, x):
        X = self.columns(x)
        return X.T @ X

    def select(self, C0, CMC0):
        p = self.p
        return select_host(self.columns(p['pool']), C0, CMC0, p['picks'], p['replicates'], p['refresh_every'],
                           p['keep'] is not None)


class _DeviceSide:
    """Each population uploaded as a dataset, its columns built by K1, its Gram by K2; the pool last, for the selection."""

    def __init__(self, p, backend, grid_cap=0):
        self.p, self.backend, self.grid_cap = p, backend, grid_cap
        self.packed = getKernels.pack_phis(p['phis'], p['kid'])

    def _stage(self, x):
        from . import engine
        packed, nb, width = self.packed
        self.backend.upload(x, np.zeros(x.shape[0]), self.p['kid'], packed, nb, width)
        slots = [_capi.SLOT_ONES]
        terms = self.p['mtx'].shape[0]
        if terms:
            pool = engine.SlotPool(self.backend, initial=max(64, terms + 3))
            term_slots = pool.take(terms)
            self.backend.build_terms(self.p['mtx'], term_slots)
            slots = slots + term_slots
        return slots

    def gram(self, x):
        slots = self._stage(x)
        return np.array(self.backend.gram(slots, slots), dtype=np.float64)

    def select(self, C0, CMC0):
        p = self.p
        slots = self._stage(p['pool'])
        return self.backend.design_select(slots, C0, CMC0, p['picks'], p['replicates'], p['refresh_every'],
                                          p['keep'] is not None, self.grid_cap)


def _run(p, side):
    G = side.gram(p['inputs'])
    G = 0.5 * (G + G.T)
    C0 = information_inverse(G, p['inv_tausqd'])
    Mt = CMC0 = None
    if p['ivr']:
        Mt = G / p['inputs'].shape[0] if p['own_target'] else side.gram(p['target']) / p['target'].shape[0]
        Mt = 0.5 * (Mt + Mt.T)
        CMC0 = C0 @ Mt @ C0
        CMC0 = 0.5 * (CMC0 + CMC0.T)
    raw = side.select(C0, CMC0)
    if np.any(raw['index'] < 0):
        raise RuntimeError(f"design: pick {int(np.flatnonzero(raw['index'] < 0)[0])} found no row to take (every criterion was "
                           f"NaN or the pool was exhausted)")
    res = DesignResult(criterion=p['criterion'], picks=p['picks'], rows=p['S'], index=raw['index'],
                       x=p['pool'][raw['index']], x_basis=raw['x'], gain=raw['gain'], vstar=raw['vstar'],
                       logdet_gain=np.cumsum(np.log1p(raw['vstar'])), target_var=None, variance=None,
                       sigsqd_mean=p['sigsqd_mean'], inv_tausqd=p['inv_tausqd'], replicates=p['replicates'],
                       refresh_every=p['refresh_every'], gram=G, C0=C0, target_gram=Mt)
    if p['ivr']:
        tv0 = float(np.sum(Mt * C0))                             # trace(M C0)
        res['target_var'] = p['sigsqd_mean'] * (tv0 - np.concatenate([[0.0], np.cumsum(raw['gain'])]))
    if p['keep'] == 'variance':
        res['variance'] = raw['v']
    return res


_SIGNATURE = """
    mtx, phis, kernel : the fitted model's (``FoKL.design`` passes its own)
    inputs      : [n, M] the model's training inputs, NORMALISED as the model's inputs are: the Gram G of their columns
    pool        : [S, M] the candidates, normalised likewise (``FoKL.design(clean=True)`` normalises pool and target)
    picks       : how many rows to choose
    criterion   : 'variance' (greedy D-optimal) or 'ivr' (integrated variance reduction over ``target``)
    target      : [rows, M] the population over which predictions matter ('ivr'; None: the training inputs)
    inv_tausqd  : 1 / tau^2 (``FoKL.design``: the mean of 1 / post.tausqd, or 1 / tausqd=)
    sigsqd_mean : the posterior mean of sigma^2; scales ``target_var`` only
    replicates  : False masks a picked row; True lets a row be taken again
    refresh_every : recompute v and w from the matrices before the picks r, 2 r, ... (0: never)
    keep        : 'variance' also returns ``variance`` [S], x_s' C x_s of every pool row after the last pick

    Returns a ``DesignResult`` (a dict with attribute access): index [picks] rows of the pool in pick order, x [picks, M]
    those rows of ``pool`` and x_basis [picks, terms + 1] their columns, gain [picks] the criterion of each pick when it was
    taken, vstar [picks] its v, logdet_gain [picks] = cumsum(log1p(vstar)) = log det(A_k) - log det(A0) in nats, target_var
    ('ivr') [picks + 1] = sigsqd_mean x the mean over the target of x' C_k x before the first and after every pick,
    variance (keep), and gram, C0, target_gram as the call formed them."""


def design(mtx, phis, kernel, inputs, pool, picks=64, criterion='variance', target=None, inv_tausqd=None, sigsqd_mean=1.0,
           replicates=False, refresh_every=64, keep=None, device=None, grid_cap=0):
    """Which rows of ``pool`` to measure next, on the device.

    device      : device index (default: the process's device, as for ``fit``) or a backend.  The pool replaces the
                  dataset uploaded to that device's context, as ``evaluate`` and ``propagate`` do.
    grid_cap    : 0 the device's grids; a test hook (the result does not depend on it)"""
    p = _prepare(mtx, phis, kernel, inputs, pool, picks, criterion, target, inv_tausqd, sigsqd_mean, replicates, refresh_every,
                 keep)
    backend = device if hasattr(device, 'design_select') and hasattr(device, 'build_terms') else None
    if backend is None:
        from . import FoKLRoutines
        backend = FoKLRoutines.device_backend(device)
    return _run(p, _DeviceSide(p, backend, grid_cap))


def design_host(mtx, phis, kernel, inputs, pool, picks=64, criterion='variance', target=None, inv_tausqd=None,
                sigsqd_mean=1.0, replicates=False, refresh_every=64, keep=None):
    """``design`` with columns, Grams and selection in numpy on this host: the statement of the computation (module
    docstring), for tests and for reading.  Same arguments, same result fields."""
    p = _prepare(mtx, phis, kernel, inputs, pool, picks, criterion, target, inv_tausqd, sigsqd_mean, replicates, refresh_every,
                 keep)
    return _run(p, _HostSide(p))


design.__doc__ += _SIGNATURE
design_host.__doc__ += _SIGNATURE

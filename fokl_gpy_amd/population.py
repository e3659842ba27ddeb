"""
Propagate a population of inputs through every posterior draw: what does the model do over a sampled input distribution,
for each draw?

``evaluate`` looks at the posterior row by row (for each ROW the mean and two order statistics over the draws).  This
module reduces the same product ``Y = X betas'`` the other way: for each DRAW the mean, variance, range, exceedance
fractions and quantiles of the output over the ROWS, RMSE / R^2 against held-out data and, from the Gram of the
population's columns, the share of the output's variance each ANOVA component carries.  ``Y`` [rows, draws] is never kept.

The quantities, defined so that the device and the host statement agree:

  moments    one launch returns per draw sum(y - c), sum((y - c)^2), min, max and, with data, sum(e), sum(e^2), e = data - y.
             c is a per-draw shift close to the draw's mean (the first launch uses the intercept and yields the mean the
             later launches shift by), so ``var = sum((y - c)^2) / S - (sum(y - c) / S)^2`` is not a difference of two
             large sums.  ``var`` is the population variance over the rows (divisor S).
  counts     the only integer output: above[d, k] = number of rows with y_d > cuts[d, k], strictly, for per-draw cut points
             (at most 32 per launch).  ``thresholds`` are the case "every draw has the same cuts".
  quantiles  found from the counts, identically for host and device: the first pass places 32 cuts evenly inside
             (min_d, max_d), each later pass 32 // Q cuts evenly inside the current bracket of each requested quantile.
             With k = ceil(q S), the bracket (a, b] of quantile q is the narrowest pair of cuts with
             S - above(a) < k <= S - above(b) (to start with a = min_d, counted as below every row, and b = max_d): the order
             statistic y_(k) lies in [a, b].  The returned value interpolates linearly inside the bracket,
             a + (b - a) (k - below(a)) / (below(b) - below(a)).  Three passes resolve about 1 / 4 000 of the draw's range.
             Every pass is one more launch of the same kernel (the moments are simply recomputed).
  shares     no launch of their own kind: one Gram of the population's columns (ones first) gives the column sums and
             X'X; with C the centred Gram, shares[d, u] = beta_du' C[u, :] beta_d / (beta_d' C beta_d), beta_du the
             coefficients of component u's terms (the intercept belongs to none).  They sum to 1 per draw and equal the
             variance fractions var(f_u) / var(y) where the components are uncorrelated over the population (a
             full-factorial grid, independent uniform inputs in the limit); where they are not, the covariance between
             components is split evenly between the two, and a share may be negative.  ``var_gram`` = beta' C beta / S
             is the same variance the kernel accumulates row by row.

``propagate`` runs columns, launches and Gram on the device (``fokl_population_stats``, csrc/fokl_population.inc; without
the library or a gfx950 device it raises, there is no host fallback).  ``propagate_host`` is the same function in numpy with
no device: the STATEMENT the kernel is tested against.  They share ``_prepare`` (every check; touches no device), the pass
loop and the assembly, and differ only in who forms the columns and reduces them.
"""
import numpy as np

from . import _capi
from . import getKernels
from .GP_Integrate import bounds_cut
from .embedded import basis_matrix, _kernel_id

MAX_CUTS = _capi.POPULATION_MAX_CUTS
NEAR = 1e-11                # population_stats_host counts the values this close (relative to the draw's scale) to a cut
_PER_DRAW = ('mean', 'var', 'min', 'max', 'exceed', 'quantiles', 'sse', 'rmse', 'r2', 'shares', 'shares_by_input')


class PropagateResult(dict):
    """A dict whose entries are also attributes (``res.mean``, ``res['mean']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def components_of(mtx):
    """The ANOVA components of an interaction matrix [T, M]: sorted tuples of input indices, one per distinct non-zero
    pattern (main effects first, then by index), and for every term the index of its component."""
    mtx = np.atleast_2d(np.asarray(mtx))
    patterns = [tuple(int(j) for j in np.flatnonzero(row)) for row in mtx] if mtx.size else []
    comps = sorted({p for p in patterns if p}, key=lambda p: (len(p), p))
    index = {p: u for u, p in enumerate(comps)}
    return comps, np.array([index.get(p, -1) for p in patterns], dtype=int)


def _prepare(betas, mtx, phis, kernel, inputs, data, thresholds, quantiles, passes, draws):
    """Every check of ``propagate`` / ``propagate_host`` (ValueError) and the arguments in the form the passes use.
    Touches no device."""
    kid = _kernel_id(kernel)
    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim == 1:
        betas = betas[np.newaxis, :]
    if betas.ndim != 2 or betas.shape[0] < 1 or betas.shape[1] < 1:
        raise ValueError("betas must be [draws, terms + 1]")
    if inputs is None:
        raise ValueError("inputs [S, M] are needed: the population to propagate")
    inputs = np.asarray(inputs, dtype=np.float64)
    if inputs.ndim == 1:
        inputs = inputs[:, np.newaxis]
    if inputs.ndim != 2 or inputs.shape[0] < 1 or inputs.shape[1] < 1:
        raise ValueError("inputs must be [S, M] with at least one row")
    S, M = inputs.shape
    mtx = np.asarray(mtx)
    mtx = mtx.reshape(0, M) if mtx.size == 0 else np.atleast_2d(mtx)
    if mtx.ndim != 2 or mtx.shape[1] != M:
        raise ValueError(f"inputs have {M} columns, the interaction matrix has {mtx.shape[-1]}")
    if betas.shape[1] != mtx.shape[0] + 1:
        raise ValueError(f"betas have {betas.shape[1]} columns, the interaction matrix wants {mtx.shape[0] + 1} (terms + 1)")
    if np.any(mtx < 0) or np.any(mtx > len(phis)):
        raise ValueError(f"the interaction matrix holds orders outside the table of {len(phis)} basis functions")
    if not np.isfinite(inputs).all() or not np.isfinite(betas).all():
        raise ValueError("inputs and betas must be finite")
    if kid == getKernels.KERNEL_SPLINES and (inputs.min() < 0.0 or inputs.max() > 1.0):
        raise ValueError("Inputs are not normalized correctly: they must lie in [0, 1] (clean=True normalises them)")
    if draws is not None:
        if int(draws) != draws or not 1 <= int(draws) <= betas.shape[0]:
            raise ValueError(f"draws must be None (all) or an integer in 1..{betas.shape[0]}, the rows of betas")
        betas = betas[betas.shape[0] - int(draws):]
    if data is not None:
        data = np.asarray(data, dtype=np.float64).reshape(-1)
        if data.shape[0] != S or not np.isfinite(data).all():
            raise ValueError(f"data must hold one finite value per row of inputs ({S})")
    thresholds = np.zeros(0) if thresholds is None else np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    if thresholds.ndim != 1 or thresholds.shape[0] > MAX_CUTS:
        raise ValueError(f"at most {MAX_CUTS} thresholds")
    if not np.isfinite(thresholds).all():
        raise ValueError("thresholds must be finite")
    quantiles = np.zeros(0) if quantiles is None else np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if quantiles.ndim != 1 or quantiles.shape[0] > MAX_CUTS or not np.all((quantiles > 0.0) & (quantiles < 1.0)):
        raise ValueError(f"quantiles must lie strictly inside (0, 1), at most {MAX_CUTS} of them")
    if int(passes) != passes or int(passes) < 1:
        raise ValueError("passes must be an integer >= 1")
    return dict(kid=kid, betas=np.ascontiguousarray(betas), mtx=mtx.astype(np.int32), phis=phis, kernel=kernel,
                inputs=np.ascontiguousarray(inputs), data=data, thresholds=thresholds, quantiles=quantiles,
                passes=int(passes), S=S, M=M, E=betas.shape[0])


def population_stats_host(X, betas, shift, cuts=None, data=None):
    """The statement of ``fokl_population_stats``: Y = X betas' [S, E] reduced over the rows per draw ->
    (moments [E, 6] = sum(y - c), sum((y - c)^2), min, max, sum(e), sum(e^2); above [E, K] int64 = rows with y > cuts[d, k];
    near [E, K] = rows with |y - cuts[d, k]| <= NEAR * max|y_d|: the counts a differently rounded sum may move)."""
    X, betas, shift = (np.asarray(a, dtype=np.float64) for a in (X, betas, shift))
    S, E = X.shape[0], betas.shape[0]
    cuts = np.zeros((E, 0)) if cuts is None else np.asarray(cuts, dtype=np.float64)
    K = cuts.shape[1]
    mom = np.zeros((E, 6))
    mom[:, 2], mom[:, 3] = np.inf, -np.inf
    above, near = np.zeros((E, K), dtype=np.int64), np.zeros((E, K), dtype=np.int64)
    step = max(1, min(S, 4_000_000 // max(E, 1)))
    blocks = [(r0, min(S, r0 + step)) for r0 in range(0, S, step)]
    scale = np.zeros(E)
    for r0, r1 in blocks:                                        # the scale first: `near` is relative to it
        scale = np.maximum(scale, np.abs(X[r0:r1] @ betas.T).max(axis=0))
    for r0, r1 in blocks:
        Y = X[r0:r1] @ betas.T
        D = Y - shift
        mom[:, 0] += D.sum(axis=0)
        mom[:, 1] += (D * D).sum(axis=0)
        mom[:, 2] = np.minimum(mom[:, 2], Y.min(axis=0))
        mom[:, 3] = np.maximum(mom[:, 3], Y.max(axis=0))
        if data is not None:
            R = np.asarray(data, dtype=np.float64)[r0:r1, np.newaxis] - Y
            mom[:, 4] += R.sum(axis=0)
            mom[:, 5] += (R * R).sum(axis=0)
        for k in range(K):
            above[:, k] += (Y > cuts[:, k]).sum(axis=0)
            near[:, k] += (np.abs(Y - cuts[:, k]) <= NEAR * scale).sum(axis=0)
    return mom, above, near


class _HostColumns:
    """Columns and reductions in numpy: what ``propagate_host`` puts in the place of the device."""

    def __init__(self, p):
        self.X = basis_matrix(p['inputs'], p['mtx'], p['phis'], p['kernel']) if p['mtx'].shape[0] else np.ones((p['S'], 1))
        self.p = p

    def stats(self, shift, cuts):
        mom, above, _ = population_stats_host(self.X, self.p['betas'], shift, cuts, self.p['data'])
        return mom, above

    def gram(self):
        return self.X.T @ self.X


class _DeviceColumns:
    """The population uploaded as a dataset, its columns built by K1: as ``evaluate`` does."""

    def __init__(self, p, backend):
        from . import engine
        self.p, self.backend = p, backend
        packed, nb, width = getKernels.pack_phis(p['phis'], p['kid'])
        backend.upload(p['inputs'], p['data'] if p['data'] is not None else np.zeros(p['S']), p['kid'], packed, nb, width)
        self.slots = [_capi.SLOT_ONES]
        terms = p['mtx'].shape[0]
        if terms:
            pool = engine.SlotPool(backend, initial=max(64, terms + 3))
            term_slots = pool.take(terms)
            backend.build_terms(p['mtx'], term_slots)
            self.slots = self.slots + term_slots

    def stats(self, shift, cuts):
        return self.backend.population_stats(self.slots, self.p['betas'], shift, cuts, self.p['data'] is not None)

    def gram(self):
        return self.backend.gram(self.slots, self.slots)


def _quantile_passes(p, columns, lo, hi, shift):
    """The pass loop of the quantiles -> (values [E, Q], brackets [E, Q, 2], moments of the last launch)."""
    S, E, q = p['S'], p['E'], p['quantiles']
    Q = q.shape[0]
    k = np.clip(np.ceil(q * S), 1, S).astype(np.int64)                       # [Q]: the order statistic wanted
    a, b = np.repeat(lo[:, None], Q, axis=1), np.repeat(hi[:, None], Q, axis=1)
    below_a, below_b = np.zeros((E, Q), dtype=np.int64), np.full((E, Q), S, dtype=np.int64)
    rows = np.arange(E)
    mom = None
    for number in range(p['passes']):
        if number == 0:                                                      # 32 cuts evenly inside (min, max), for all
            per = MAX_CUTS
            frac = (np.arange(per) + 1.0) / (per + 1.0)
            cuts = lo[:, None] + (hi - lo)[:, None] * frac
            owner = [slice(0, per)] * Q
        else:                                                                # 32 // Q cuts inside each quantile's bracket
            per = MAX_CUTS // Q
            frac = (np.arange(per) + 1.0) / (per + 1.0)
            cuts = (a[:, :, None] + (b - a)[:, :, None] * frac).reshape(E, Q * per)
            owner = [slice(i * per, (i + 1) * per) for i in range(Q)]
        mom, above = columns.stats(shift, np.ascontiguousarray(cuts))
        below = S - above                                                    # rows with y <= cut
        for i in range(Q):
            c, n_below = cuts[:, owner[i]], below[:, owner[i]]
            first = (n_below < k[i]).sum(axis=1)                             # cuts are ascending, so are the counts
            has_a, has_b = first > 0, first < per
            ia, ib = np.maximum(first - 1, 0), np.minimum(first, per - 1)
            a[:, i] = np.where(has_a, c[rows, ia], a[:, i])
            below_a[:, i] = np.where(has_a, n_below[rows, ia], below_a[:, i])
            b[:, i] = np.where(has_b, c[rows, ib], b[:, i])
            below_b[:, i] = np.where(has_b, n_below[rows, ib], below_b[:, i])
    inside = np.maximum(below_b - below_a, 1)
    values = a + (b - a) * np.clip((k - below_a) / inside, 0.0, 1.0)
    return values, np.stack([a, b], axis=-1), mom


def _shares(p, columns):
    comps, of_term = components_of(p['mtx'])
    G = np.asarray(columns.gram(), dtype=np.float64)
    sums = G[0]                                                              # the ones column: column sums
    C = G - np.outer(sums, sums) / p['S']
    betas = p['betas']
    contrib = betas * (betas @ C)                                            # [E, nc]: beta_i (C beta)_i, no loop over draws
    member = np.zeros((len(comps), betas.shape[1]))
    for t, u in enumerate(of_term):
        if u >= 0:
            member[u, t + 1] = 1.0
    total = contrib.sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        shares = (contrib @ member.T) / total[:, None]
    contains = np.array([[1.0 if j in c else 0.0 for j in range(p['M'])] for c in comps]).reshape(len(comps), p['M'])
    return dict(components=comps, shares=shares, shares_by_input=shares @ contains, var_gram=total / p['S'])


def _run(p, columns, sensitivity, ReturnBounds):
    S, E, betas = p['S'], p['E'], p['betas']
    res = PropagateResult()
    # launch 1: the range, and the mean every later launch shifts by
    mom, _ = columns.stats(betas[:, 0].copy(), None)
    lo, hi = mom[:, 2].copy(), mom[:, 3].copy()
    shift = betas[:, 0] + mom[:, 0] / S
    launches = 1
    if p['thresholds'].shape[0]:
        mom, above = columns.stats(shift, np.ascontiguousarray(np.broadcast_to(p['thresholds'], (E, p['thresholds'].shape[0]))))
        res['exceed'] = above / S
        launches += 1
    else:
        res['exceed'] = np.zeros((E, 0))
    if p['quantiles'].shape[0]:
        res['quantiles'], res['quantile_brackets'], mom = _quantile_passes(p, columns, lo, hi, shift)
        launches += p['passes']
    else:
        res['quantiles'], res['quantile_brackets'] = np.zeros((E, 0)), np.zeros((E, 0, 2))
    if launches == 1:                                                        # the moments about the mean
        mom, _ = columns.stats(shift, None)
        launches += 1
    m1 = mom[:, 0] / S
    res.update(mean=shift + m1, var=np.maximum(mom[:, 1] / S - m1 * m1, 0.0), min=mom[:, 2], max=mom[:, 3], shift=shift,
               launches=launches, thresholds=p['thresholds'], quantile_levels=p['quantiles'])
    if p['data'] is not None:
        sst = float(np.sum((p['data'] - p['data'].mean()) ** 2))
        with np.errstate(divide='ignore', invalid='ignore'):
            res.update(sse=mom[:, 5].copy(), rmse=np.sqrt(mom[:, 5] / S), r2=1.0 - mom[:, 5] / sst,
                       bias=-mom[:, 4] / S)
    if sensitivity:
        res.update(_shares(p, columns))
    if ReturnBounds and E >= 2:
        cut = bounds_cut(E)
        for name in _PER_DRAW:
            if name in res:
                srt = np.sort(res[name], axis=0)
                res[name + '_mean'] = res[name].mean(axis=0)
                res[name + '_bounds'] = np.stack([srt[cut], srt[E - cut]], axis=-1)
    return res


def _backend_of(device):
    if hasattr(device, 'population_stats') and hasattr(device, 'build_terms') and hasattr(device, 'gram'):
        return device
    from . import FoKLRoutines
    return FoKLRoutines.device_backend(device)


_SIGNATURE = """
    betas       : [E_all, terms + 1], rows are draws as ``fit`` returns them (or [terms + 1]: one coefficient vector)
    mtx, phis, kernel : the model's (``FoKL.propagate`` passes its own)
    inputs      : [S, M] the population, NORMALISED as the model's inputs are (``FoKL.propagate(clean=True)`` normalises)
    data        : [S] held-out data at those rows -> sse, rmse, r2 (and bias = mean(y - data)) per draw
    thresholds  : at most 32 values in the output's scale -> exceed [E, K], the fraction of rows with y > threshold, strictly
    quantiles   : levels strictly inside (0, 1) -> quantiles [E, Q] and quantile_brackets [E, Q, 2]; passes >= 1 refines them
    sensitivity : also components (tuples of input indices), shares [E, U], shares_by_input [E, M], var_gram [E]
    draws       : None uses ALL rows of betas, an integer the last ``draws`` rows, in order.  Nothing is drawn at random:
                  numpy's random stream is not consumed and a model's ``setnos`` is neither read nor set (``evaluate``
                  chooses its draws as before).
    ReturnBounds : with at least two draws every per-draw quantity q also gets q_mean and q_bounds [..., 2] =
                  (sorted[cut], sorted[E - cut]) over the draws, cut = ``bounds_cut(E)`` as in ``evaluate`` and ``optimize``

    Returns a ``PropagateResult`` (a dict with attribute access), every per-draw array [E] or [E, .]: mean, var (population
    variance over the rows), min, max, exceed, quantiles, quantile_brackets, and what ``data`` / ``sensitivity`` add; the
    shares sum to 1 per draw, equal the variance fractions where the components are uncorrelated over the population and
    carry the covariance terms (they may be negative) where they are not."""


def propagate(betas, mtx, phis, kernel, inputs, data=None, thresholds=None, quantiles=(0.025, 0.5, 0.975), passes=3,
              sensitivity=False, draws=None, ReturnBounds=True, device=None):
    """What does the model do over a population of inputs, for every posterior draw?  On the device.

    device      : device index (default: the process's device, as for ``fit``) or a backend.  The population replaces the
                  dataset uploaded to that device's context, as ``evaluate`` does."""
    p = _prepare(betas, mtx, phis, kernel, inputs, data, thresholds, quantiles, passes, draws)
    return _run(p, _DeviceColumns(p, _backend_of(device)), sensitivity, ReturnBounds)


def propagate_host(betas, mtx, phis, kernel, inputs, data=None, thresholds=None, quantiles=(0.025, 0.5, 0.975), passes=3,
                   sensitivity=False, draws=None, ReturnBounds=True):
    """``propagate`` with columns and reductions in numpy on this host: the statement of the computation (module
    docstring), for tests and for reading.  Same arguments, same result fields."""
    p = _prepare(betas, mtx, phis, kernel, inputs, data, thresholds, quantiles, passes, draws)
    return _run(p, _HostColumns(p), sensitivity, ReturnBounds)


propagate.__doc__ += _SIGNATURE
propagate_host.__doc__ += _SIGNATURE

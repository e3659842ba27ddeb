"""
Score a fitted model pointwise: the log predictive density of every row over all posterior draws, WAIC and Pareto-smoothed
importance-sampling leave-one-out (PSIS-LOO; Vehtari, Gelman, Gabry 2017; Vehtari et al., "Pareto smoothed importance
sampling").  The search compares models by a BIC at the least-squares point; this compares FITS (kernels, tolerances, an
updated model against a refit), says which rows a model predicts badly and has an out-of-sample meaning.  It is the one
quantity that needs both beta and sigma^2 per draw, which ``resample`` keeps.

With X [S, nc] (ones first), y [S], betas [E, nc], sigsqd [E] > 0 and c_d = -log(2 pi sigsqd_d) / 2, h_d = 0.5 / sigsqd_d:

  ll[i, d]    = c_d - (y_i - X_i . beta_d)^2 h_d                     (never stored on the device)
  lppd_i      = logsumexp_d(ll) - log E
  ll_mean_i   = mean_d ll
  p_waic_i    = var_d ll, divisor E - 1, accumulated about ll[i, 0] so that it is not a difference of two large sums
  elpd_waic_i = lppd_i - p_waic_i

PSIS (E >= 25), M = min(E // 5, ceil(3 sqrt(E))):
  r_d = -ll[i, d], s = sort(r - max r) ascending; the cutoff u = max(s[E - M - 1], log(DBL_MIN)); the tail = the values
  among the last M of s STRICTLY above u, M' of them (ties at the cutoff keep their raw weights).  With M' <= 4, or when
  the exceedance at the tail's lower quartile is not positive, khat_i = +inf and the raw weights are used.  Otherwise the
  exceedances e_j = exp(t_j) - exp(u), ascending, are fitted by a generalised Pareto distribution with the Zhang-Stephens
  estimator (``gpd_fit``): m = 30 + floor(sqrt(M')) grid points b_j = [1 - sqrt(m / (j - 1/2))] / (3 e[floor(M'/4 + 1/2) - 1])
  + 1 / e[M' - 1], k_j = mean(log1p(-b_j e)), L_j = M' (log(-b_j / k_j) - k_j - 1), b = sum softmax(L)_j b_j,
  k = mean(log1p(-b e)), sigma = -k / b, khat = (M' k + 5) / (M' + 10).  The tail's log weights are replaced in rank order
  by min(log(exp(u) + sigma expm1(-khat log1p(-p_j)) / khat), 0), p_j = (j + 1/2) / M', and
  elpd_loo_i = logsumexp_d(w_d + ll_d) - logsumexp_d(w_d).

Totals are sums over the rows, standard errors sqrt(S var(pointwise)) (numpy's default divisor), p_loo = sum(lppd_i -
elpd_loo_i), khat_threshold = min(1 - 1 / log10(E), 0.7).

Under Student-t noise with ``nu`` degrees of freedom (finite nu >= 1: sigsqd_d is the squared SCALE, as ``resample_robust``
draws it) and / or known row precisions w_i (``weights``; sw_i = sqrt(w_i), lw_i = log(sw_i) = 0.5 log(w_i)) only ll changes:

  Student            ll[i, d] = c_d + lw_i - ((nu + 1) / 2) log1p((sw_i e)^2 g_d),   e = y_i - X_i . beta_d,
                     c_d = log(Gamma((nu + 1) / 2) / Gamma(nu / 2)) - 0.5 log(nu pi sigsqd_d)  (``student_constants``: the
                     ratio of the two Gammas is formed as ONE number, never as a difference of two lgamma), g_d = 1 / (nu sigsqd_d)
  weighted Gaussian  ll[i, d] = c_d + lw_i - (sw_i e)^2 h_d, with c_d and h_d as above

and everything after ll is the text above (``fokl_score_rows_noise``).  With nu = inf and no weights it IS the text above.

``score`` runs columns and reduction on the device (``fokl_score_rows``, csrc/fokl_score_device.inc; without the library or
a gfx950 device it raises, there is no host fallback).  ``score_host`` is the same function in numpy with no device: the
STATEMENT the kernel is tested against (``score_rows_host``).  They share ``_prepare`` (every check; touches no device) and
the assembly, and differ only in who forms the columns and reduces them.
"""
import math
import sys

import numpy as np

from . import _capi
from . import population as _population
from .embedded import basis_matrix, _kernel_id

MAX_TAIL = _capi.SCORE_MAX_TAIL             # entries (M + 1) of the device kernel's list per row
MIN_DRAWS = 25                              # PSIS: a tail of at least 5 draws
LOG_DBL_MIN = math.log(sys.float_info.min)
KHAT_ROWS_KEPT = 1000
METHODS = ('waic', 'loo', 'lpd')
STATS = ('lppd', 'll_mean', 'p_waic', 'elpd_loo', 'khat', 'sigma', 'max_r', 'tail')     # columns of score_rows_host


class ScoreResult(dict):
    """A dict whose entries are also attributes (``res.elpd_loo``, ``res['elpd_loo']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def tail_len(E):
    """M: the number of draws whose weights PSIS smooths."""
    return int(min(E // 5, math.ceil(3.0 * math.sqrt(E))))


def max_draws_loo():
    """The most draws 'loo' takes on the device: the largest E with tail_len(E) + 1 <= MAX_TAIL."""
    E = 1
    while tail_len(E + 1) + 1 <= MAX_TAIL:
        E += 1
    return E


def khat_threshold(E):
    return min(1.0 - 1.0 / math.log10(E), 0.7)


def likelihood_constants(sigsqd):
    """(c, h) with ll = c - (y - yhat)^2 h; the logarithm is libm's, as the native entry point forms it."""
    sigsqd = np.asarray(sigsqd, dtype=np.float64).reshape(-1)
    c = np.array([-0.5 * math.log(2.0 * math.pi * float(s)) for s in sigsqd])
    return c, 0.5 / sigsqd


def gamma_ratio(a):
    """Gamma(a + 1/2) / Gamma(a) for a >= 1/2: ``math.gamma`` twice below 80 (a few ulp), above it sqrt(a) times exp of the
    asymptotic series (-1 / 8 + 1 / (192 a^2) - 1 / (640 a^4) + 17 / (14336 a^6)) / a (the next term is below 1e-18 there).
    The difference of two ``lgamma`` loses every digit that their size has in front of the point (1e-6 at nu = 1e9); this
    does not.  The native entry points hold the same text."""
    a = float(a)
    if a < 80.0:
        return math.gamma(a + 0.5) / math.gamma(a)
    r = 1.0 / (a * a)
    return math.sqrt(a) * math.exp((-1.0 / 8.0 + (1.0 / 192.0 + (-1.0 / 640.0 + 17.0 / 14336.0 * r) * r) * r) / a)


def student_constants(sigsqd, nu):
    """(c, g, hp) with ll = c + lw - hp log1p((sw e)^2 g) under Student-t noise (module docstring)."""
    sigsqd = np.asarray(sigsqd, dtype=np.float64).reshape(-1)
    lead = math.log(gamma_ratio(0.5 * nu))
    c = np.array([lead - 0.5 * math.log(nu * math.pi * float(s)) for s in sigsqd])
    return c, 1.0 / (nu * sigsqd), 0.5 * (nu + 1.0)


def log_likelihood(X, y, betas, sigsqd, nu=np.inf, sw=None):
    """ll [S, E]: the matrix the device never stores.  ``nu`` finite: Student-t noise; ``sw`` [S]: sqrt of the row precisions."""
    e = np.asarray(y, dtype=np.float64).reshape(-1, 1) - np.asarray(X, dtype=np.float64) @ np.asarray(betas, dtype=np.float64).T
    if not np.isfinite(nu) and sw is None:
        c, h = likelihood_constants(sigsqd)
        return c - (e * e) * h
    sw = np.ones(e.shape[0]) if sw is None else np.asarray(sw, dtype=np.float64).reshape(-1)
    lw, e = np.log(sw)[:, None], sw[:, None] * e
    if np.isfinite(nu):
        c, g, hp = student_constants(sigsqd, nu)
        return (c + lw) - hp * np.log1p((e * e) * g)
    c, h = likelihood_constants(sigsqd)
    return (c + lw) - (e * e) * h


def _logsumexp(a):
    m = np.max(a)
    return m + math.log(np.sum(np.exp(a - m)))


def gpd_fit(e):
    """Zhang-Stephens fit of a generalised Pareto distribution to the exceedances ``e`` (ascending, positive) ->
    (k, sigma, khat): the raw shape, the scale and the shape regularised towards 0.5 with the weight of 10 values."""
    e = np.asarray(e, dtype=np.float64)
    n = e.shape[0]
    m = 30 + int(math.floor(math.sqrt(n)))
    j = np.arange(1, m + 1)
    b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * e[int(math.floor(n / 4.0 + 0.5)) - 1]) + 1.0 / e[n - 1]
    k = np.mean(np.log1p(-b[:, None] * e), axis=1)
    L = n * (np.log(-b / k) - k - 1.0)
    w = np.exp(L - L.max())
    w /= w.sum()
    bb = float(np.sum(w * b))
    kk = float(np.mean(np.log1p(-bb * e)))
    return kk, -kk / bb, (n * kk + 5.0) / (n + 10.0)


def psis_row(ll):
    """PSIS-LOO of one row from its ll [E] -> (elpd_loo, khat, sigma, max r, M', the sorted top M + 1 of r - max r)."""
    ll = np.asarray(ll, dtype=np.float64)
    E = ll.shape[0]
    M = tail_len(E)
    r = -ll
    rmax = r.max()
    order = np.argsort(r, kind='stable')
    s, llo = (r - rmax)[order], ll[order]
    u = max(s[E - M - 1], LOG_DBL_MIN)
    in_tail = np.zeros(E, dtype=bool)
    in_tail[E - M:] = s[E - M:] > u
    tail = s[in_tail]
    n_tail = tail.shape[0]
    lw = s.copy()
    khat, sigma = np.inf, 0.0
    if n_tail > 4:
        eu = math.exp(u)
        e = np.exp(tail) - eu
        if e[int(math.floor(n_tail / 4.0 + 0.5)) - 1] > 0.0:
            _, sigma, khat = gpd_fit(e)
            p = (np.arange(n_tail) + 0.5) / n_tail
            lw[in_tail] = np.minimum(np.log(eu + sigma * np.expm1(-khat * np.log1p(-p)) / khat), 0.0)
    return _logsumexp(lw + llo) - _logsumexp(lw), khat, sigma, rmax, n_tail, s[E - M - 1:]


def score_rows_host(X, y, betas, sigsqd, want_loo=True, want_tail=False, nu=np.inf, sw=None):
    """The statement of ``fokl_score_rows`` (and, with ``nu`` or ``sw``, of ``fokl_score_rows_noise``) -> stats [S, 8] (columns
    ``STATS``; 3 .. 7 are zero without ``want_loo``), with ``want_tail`` also tail [S, M + 1]."""
    ll = log_likelihood(X, y, betas, sigsqd, nu, sw)
    S, E = ll.shape
    stats = np.zeros((S, 8))
    m = ll.max(axis=1)
    stats[:, 0] = m + (np.log(np.exp(ll - m[:, None]).sum(axis=1)) - math.log(E))
    d = ll - ll[:, :1]
    s1, s2 = d.sum(axis=1), (d * d).sum(axis=1)
    stats[:, 1] = ll[:, 0] + s1 / E
    if E > 1:
        stats[:, 2] = np.maximum((s2 - s1 * s1 / E) / (E - 1.0), 0.0)
    tail = None
    if want_loo:
        if E < MIN_DRAWS:
            raise ValueError(f"PSIS needs at least {MIN_DRAWS} draws, there are {E}")
        tail = np.zeros((S, tail_len(E) + 1))
        for i in range(S):
            stats[i, 3], stats[i, 4], stats[i, 5], stats[i, 6], stats[i, 7], tail[i] = psis_row(ll[i])
    return (stats, tail) if want_tail else stats


def _methods(method):
    names = (method,) if isinstance(method, str) else tuple(method)
    if not names or any(name not in METHODS for name in names):
        raise ValueError(f"method must be one or several of {METHODS}")
    return tuple(name for name in METHODS if name in names)


def _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, method, draws, nu=np.inf, weights=None):
    """Every check of ``score`` / ``score_host`` (ValueError) and the arguments in the form both use.  Touches no device."""
    kid = _kernel_id(kernel)
    methods = _methods(method)
    try:
        nu = float(np.inf if nu is None else nu)
    except (TypeError, ValueError):
        raise ValueError(f"nu must be a number >= 1 or np.inf, it is {nu!r}") from None
    if not nu >= 1.0:
        raise ValueError(f"nu = {nu:g} is NaN or < 1: Student-t noise needs nu >= 1 (nu = np.inf is Gaussian noise)")
    if betas is None or sigsqd is None:
        raise ValueError("score needs betas [draws, terms + 1] AND sigsqd [draws]: a fit keeps no sigma^2 per draw, resample does")
    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim == 1:
        betas = betas[np.newaxis, :]
    if betas.ndim != 2 or betas.shape[0] < 1 or betas.shape[1] < 1:
        raise ValueError("betas must be [draws, terms + 1]")
    sigsqd = np.asarray(sigsqd, dtype=np.float64).reshape(-1)
    if sigsqd.shape[0] != betas.shape[0]:
        raise ValueError(f"sigsqd holds {sigsqd.shape[0]} values, betas has {betas.shape[0]} rows: one sigma^2 per draw is needed")
    if inputs is None or data is None:
        raise ValueError("inputs [S, M] and data [S] are needed: the rows to score")
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
    data = np.asarray(data, dtype=np.float64).reshape(-1)
    if data.shape[0] != S or not np.isfinite(data).all():
        raise ValueError(f"data must hold one finite value per row of inputs ({S})")
    if not np.isfinite(inputs).all():
        raise ValueError("inputs must be finite")
    sw = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != S:
            raise ValueError(f"weights must hold one value per row ({S}), there are {w.shape[0]}")
        if not np.isfinite(w).all() or np.any(w <= 0.0):
            raise ValueError("weights must be finite and > 0 (drop a row instead of giving it no weight)")
        sw = np.sqrt(w)
        if not np.isfinite(np.log(sw)).all() or np.any(sw <= 0.0):
            raise ValueError("weights must be finite and > 0 after their square root as well")
    if kid == _population.getKernels.KERNEL_SPLINES and (inputs.min() < 0.0 or inputs.max() > 1.0):
        raise ValueError("Inputs are not normalized correctly: they must lie in [0, 1] (clean=True normalises them)")
    if draws is not None:
        if np.ndim(draws) == 0:
            if int(draws) != draws or not 1 <= int(draws) <= betas.shape[0]:
                raise ValueError(f"draws must be None (all), an integer in 1..{betas.shape[0]} (the last rows of betas) or an "
                                 f"index array")
            index = np.arange(betas.shape[0] - int(draws), betas.shape[0])
        else:
            index = np.asarray(draws)
            if index.ndim != 1 or index.shape[0] < 1 or not np.issubdtype(index.dtype, np.integer) or \
                    index.min() < -betas.shape[0] or index.max() >= betas.shape[0]:
                raise ValueError(f"draws as an array must hold at least one integer index into the {betas.shape[0]} rows of betas")
        betas, sigsqd = betas[index], sigsqd[index]
    bad = ~(np.isfinite(betas).all(axis=1) & np.isfinite(sigsqd))
    if bad.any():
        raise ValueError(f"{int(bad.sum())} of the {betas.shape[0]} draws are NaN or infinite (the rows of a resample's flagged "
                         f"chains, res.flagged): drop them, e.g. with draws=np.flatnonzero(np.isfinite(res.sigsqd))")
    if not np.all(sigsqd > 0.0):
        raise ValueError("every sigsqd must be positive")
    E = betas.shape[0]
    if 'loo' in methods:
        if E < MIN_DRAWS:
            raise ValueError(f"'loo' needs at least {MIN_DRAWS} draws (a Pareto tail of 5), there are {E}")
        if tail_len(E) + 1 > MAX_TAIL:
            raise ValueError(f"'loo' over {E} draws wants a tail list of {tail_len(E) + 1} entries per row, the device kernel's "
                             f"holds FOKL_SCORE_MAX_TAIL = {MAX_TAIL} (at most {max_draws_loo()} draws: thin them with an index "
                             f"array; 'waic' and 'lpd' have no limit)")
    return dict(kid=kid, betas=np.ascontiguousarray(betas), sigsqd=np.ascontiguousarray(sigsqd), mtx=mtx.astype(np.int32),
                phis=phis, kernel=kernel, inputs=np.ascontiguousarray(inputs), data=data, methods=methods, S=S, M=M, E=E, nu=nu,
                sw=sw)


def _assemble(p, stats):
    """A ScoreResult from the per-row statistics [S, 8]."""
    S, E, methods = p['S'], p['E'], p['methods']
    se = lambda v: float(np.sqrt(S * np.var(v)))
    nu = p.get('nu', np.inf)
    res = ScoreResult(method=methods, rows=S, draws=E, pointwise=dict(lppd=stats[:, 0].copy()), nu=nu,
                      noise='student' if np.isfinite(nu) else 'gaussian', weighted=p.get('sw') is not None)
    pw = res['pointwise']
    res.update(lppd=float(pw['lppd'].sum()), se_lppd=se(pw['lppd']))
    if 'waic' in methods or 'loo' in methods:
        pw.update(ll_mean=stats[:, 1].copy(), p_waic=stats[:, 2].copy(), elpd_waic=stats[:, 0] - stats[:, 2])
        res.update(elpd_waic=float(pw['elpd_waic'].sum()), p_waic=float(pw['p_waic'].sum()), se_waic=se(pw['elpd_waic']),
                   waic=-2.0 * float(pw['elpd_waic'].sum()))
    if 'loo' in methods:
        pw.update(elpd_loo=stats[:, 3].copy(), khat=stats[:, 4].copy(), sigma=stats[:, 5].copy(), tail=stats[:, 7].astype(np.int64))
        thr = khat_threshold(E)
        over = np.flatnonzero(pw['khat'] > thr)
        res.update(elpd_loo=float(pw['elpd_loo'].sum()), p_loo=float((stats[:, 0] - stats[:, 3]).sum()), se_loo=se(pw['elpd_loo']),
                   looic=-2.0 * float(pw['elpd_loo'].sum()), khat=pw['khat'], khat_threshold=thr, khat_bad=int(over.shape[0]),
                   khat_bad_rows=over[:KHAT_ROWS_KEPT], tail_length=tail_len(E))
    return res


def compare(a, b):
    """Paired comparison of two scores of the SAME rows -> dict(measure, elpd_diff = a - b, se_diff, rows): the difference of
    the totals and its standard error from the pointwise differences (sqrt(S var(diff))).  The measure is 'elpd_loo' where
    both have it, else 'elpd_waic', else 'lppd'."""
    if a['rows'] != b['rows']:
        raise ValueError(f"compare needs scores of the same rows: {a['rows']} against {b['rows']}")
    for measure in ('elpd_loo', 'elpd_waic', 'lppd'):
        if measure in a['pointwise'] and measure in b['pointwise']:
            break
    diff = a['pointwise'][measure] - b['pointwise'][measure]
    return ScoreResult(measure=measure, elpd_diff=float(diff.sum()), se_diff=float(np.sqrt(diff.shape[0] * np.var(diff))),
                       rows=int(diff.shape[0]))


_SIGNATURE = """
    betas, sigsqd : [E_all, terms + 1] and [E_all]: the draws and their sigma^2, as ``resample`` returns them
    mtx, phis, kernel : the model's (``FoKL.score`` passes its own)
    inputs, data  : [S, M] NORMALISED as the model's inputs are (``FoKL.score(clean=True)`` normalises) and [S]: the rows
    method        : 'waic', 'loo', 'lpd' or several: 'lpd' is the log predictive density alone (held-out rows)
    draws         : None uses ALL rows of betas, an integer the last ``draws`` rows, an integer array those rows (rows of
                    several chains are chain-major, so thinning needs the array form).  Nothing is drawn at random.
    nu            : np.inf (default): Gaussian noise; finite nu >= 1: sigsqd is the squared SCALE of Student-t noise with nu
                    degrees of freedom, as ``resample_robust`` draws it
    weights       : None (ones) or [S] known relative precisions of the rows, finite and > 0: row i's noise has the scale
                    sqrt(sigsqd / w_i).  With nu = np.inf and no weights the call is today's, to the bit.

    Returns a ``ScoreResult`` (a dict with attribute access): rows, draws, method, lppd, se_lppd; with 'waic' elpd_waic,
    p_waic, se_waic, waic; with 'loo' elpd_loo, p_loo, se_loo, looic, khat [S], khat_threshold, khat_bad (rows above it),
    khat_bad_rows (their indices, at most 1 000), tail_length (M); ``pointwise`` holds the per-row arrays [S] by name; nu,
    noise ('gaussian' or 'student') and weighted say which likelihood was scored."""


def score(betas, sigsqd, mtx, phis, kernel, inputs, data, method=('waic', 'loo'), draws=None, device=None, nu=np.inf,
          weights=None):
    """Score every row over every draw on the device.

    device        : device index (default: the process's device, as for ``fit``) or a backend.  The rows replace the
                    dataset uploaded to that device's context, as ``evaluate`` and ``propagate`` do."""
    p = _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, method, draws, nu, weights)
    backend = device if hasattr(device, 'score_rows') and hasattr(device, 'build_terms') else None
    if backend is None:
        from . import FoKLRoutines
        backend = FoKLRoutines.device_backend(device)
    columns = _population._DeviceColumns(p, backend)
    if np.isfinite(p['nu']) or p['sw'] is not None:
        return _assemble(p, backend.score_rows_noise(columns.slots, p['betas'], p['sigsqd'], 'loo' in p['methods'], nu=p['nu'],
                                                     sw=p['sw']))
    return _assemble(p, backend.score_rows(columns.slots, p['betas'], p['sigsqd'], 'loo' in p['methods']))


def score_host(betas, sigsqd, mtx, phis, kernel, inputs, data, method=('waic', 'loo'), draws=None, nu=np.inf, weights=None):
    """``score`` with columns and reduction in numpy on this host: the statement of the computation (module docstring), for
    tests and for reading.  Same arguments, same result fields."""
    p = _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, method, draws, nu, weights)
    X = basis_matrix(p['inputs'], p['mtx'], p['phis'], p['kernel']) if p['mtx'].shape[0] else np.ones((p['S'], 1))
    return _assemble(p, score_rows_host(X, p['data'], p['betas'], p['sigsqd'], 'loo' in p['methods'], nu=p['nu'], sw=p['sw']))


score.__doc__ += _SIGNATURE
score_host.__doc__ += _SIGNATURE

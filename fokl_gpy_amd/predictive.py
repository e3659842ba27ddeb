"""
The posterior predictive DISTRIBUTION of every row: its CDF at the observed value (the probability integral transform, PIT),
its quantiles (prediction intervals for new measurements) and the coverage of those intervals.  ``evaluate(ReturnBounds=
True)`` and ``coverage3`` give a credible band of the MEAN, X betas', without the noise; ``score`` reduces the predictive
density.  For row i the predictive is the equal-weight mixture over the E draws of N(mu_id, sigsqd_d), mu_id = X_i . beta_d,
which needs both beta and sigma^2 per draw: ``resample`` keeps them.

With X [S, nc] (ones first), betas [E, nc], sd_d = sqrt(sigsqd_d), rinv_d = 1 / (sd_d sqrt(2)) (both formed on the host with
libm), y [S] or None, p [Q] (0 < p < 1, Q <= 8) and z [Q] the standard normal quantiles of p (formed on the host):

Pass 0, one walk over the draws, per row:
  s1 = sum_d (mu_d - mu_0), s2 = sum_d (mu_d - mu_0)^2          (about draw 0: the variance is no difference of large sums)
  mu_min = min_d mu_d, mu_max = max_d mu_d
  lo_j = min_d (mu_d + sd_d z_j), hi_j = max_d (mu_d + sd_d z_j)  (exact: every component's CDF at lo_j is <= p_j and at hi_j
                                                                 >= p_j, so the mixture's is too)
  with y: pit = (sum_d 0.5 erfc((mu_d - y) rinv_d)) / E
  mean = mu_0 + s1 / E, var = max((s2 - s1 s1 / E) / E, 0) + mean_d(sd_d sd_d)

First trial: q_j = mean + z_j sqrt(var) where lo_j < q_j < hi_j, else (lo_j + hi_j) / 2.  r_j = +inf, r_prev_j = +inf.

Passes k = 1 .. max_passes, each one walk over the draws; for every (row, quantile) that is not done:
  1. t_d = (q - mu_d) rinv_d
  2. F = (sum_d 0.5 erfc(-t_d)) / E                               (Phi as 0.5 erfc(-t), not 1 - ...: the lower tail)
  3. f = (sum_d exp(-t_d t_d) rinv_d) / (E sqrt(pi))
  4. r = F - p; r and the pass number k are recorded, q is the row's answer so far
  5. lo = q if r < 0, else hi = q
  6. done if |r| <= ftol or hi - lo <= xtol (mu_max - mu_min + max_d sd_d)
  7. else the Newton proposal q - r / f is taken if f > 0, lo < q - r / f < hi and |r| <= r_prev / 2, and then r_prev = |r|;
     otherwise the midpoint (lo + hi) / 2 is taken and r_prev = +inf.  (r_prev is the residual of the previous pass if that
     pass also took a Newton step: without the halving condition a mixture whose sd spread over four decades does not
     converge in 40 passes.)
A pair with |r| > ftol at the end is UNRESOLVED, whether it ran out of passes or stopped on the width test (where the CDF is
a staircase): it is counted and reported, not hidden.

Per row the rows-level functions return the block [S, 6 + 5 Q] = mu_0, s1, s2, mu_min, mu_max, pit (0 without y), then per
quantile q, r, lo, hi, passes (``COLUMNS``, ``QCOLUMNS``).

``predictive`` runs columns and passes on the device (``fokl_predictive_rows``, csrc/fokl_predictive_device.inc; without the
library or a gfx950 device it raises, there is no host fallback).  ``predictive_host`` is the same function in numpy with no
device: the STATEMENT the kernel is tested against (``predictive_rows_host``).  They share ``_prepare`` (every check; touches
no device) and ``_assemble``, and differ only in who forms the columns and walks the draws.
"""
import math

import numpy as np
from scipy.special import erfc as _erfc

from . import _capi
from . import population as _population
from . import score as _score
from .embedded import basis_matrix

MAX_QUANTILES = _capi.PREDICTIVE_MAX_QUANTILES
COLUMNS = ('mu0', 's1', 's2', 'mu_min', 'mu_max', 'pit')            # the first columns of the block
QCOLUMNS = ('q', 'r', 'lo', 'hi', 'passes')                          # ... and per quantile
MAX_PASSES, FTOL, XTOL = 32, 1e-13, 1e-15
PIT_BINS = 20
UNRESOLVED_ROWS_KEPT = 1000
DEFAULT_QUANTILES = (0.025, 0.5, 0.975)
_CHUNK = 1 << 22                                                     # values of a [rows, draws] slab of the host statement


class PredictiveResult(dict):
    """A dict whose entries are also attributes (``res.pit``, ``res['pit']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def normal_quantile(p):
    """z with 0.5 erfc(-z / sqrt(2)) = p, by Newton steps on log Phi with math.erfc (no dependency); the upper half by
    symmetry, 1 - p being exact there."""
    p = float(p)
    if p > 0.5:
        return -normal_quantile(1.0 - p)
    if p == 0.5:
        return 0.0
    z = -math.sqrt(-2.0 * math.log(p)) if p < 0.1 else 0.0          # left of the root for small p; log Phi is concave
    for _ in range(100):
        cdf = 0.5 * math.erfc(-z / math.sqrt(2.0))
        step = (math.log(cdf) - math.log(p)) * cdf / (math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))
        z -= step
        if abs(step) <= 1e-16 * max(abs(z), 1.0):
            break
    return z


def scales(sigsqd):
    """(sd, rinv) = (sqrt(sigsqd), 1 / (sd sqrt(2))) with libm, as both ``predictive`` and ``predictive_host`` pass them on."""
    sd = np.array([math.sqrt(float(s)) for s in np.reshape(sigsqd, -1)])
    rinv = np.array([1.0 / (float(s) * math.sqrt(2.0)) for s in sd])
    return sd, rinv



def mixture_cdf(mu, rinv, q):
    """F [S] of the mixtures with means mu [S, E] at q [S]: (sum_d 0.5 erfc(-(q - mu_d) rinv_d)) / E."""
    t = (np.reshape(q, (-1, 1)) - mu) * rinv
    return (0.5 * _erfc(-t)).sum(axis=1) / mu.shape[1]


def predictive_rows_from_means(mu, sd, rinv, y, p, z, max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL):
    """The statement from the means mu [S, E] = X betas' on: the block [S, 6 + 5 Q] (module docstring)."""
    S, E = mu.shape
    Q = p.shape[0]
    out = np.zeros((S, 6 + 5 * Q))
    d = mu - mu[:, :1]
    s1, s2 = d.sum(axis=1), (d * d).sum(axis=1)
    mu_min, mu_max = mu.min(axis=1), mu.max(axis=1)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = mu[:, 0], s1, s2, mu_min, mu_max
    if y is not None:
        out[:, 5] = (0.5 * _erfc((mu - y[:, None]) * rinv)).sum(axis=1) / E
    if not Q:
        return out
    mean = mu[:, 0] + s1 / E
    var = np.maximum((s2 - s1 * s1 / E) / E, 0.0) + np.mean(sd * sd)
    width = mu_max - mu_min + sd.max()
    for j in range(Q):
        c = mu + sd * z[j]
        lo, hi = c.min(axis=1), c.max(axis=1)
        q = mean + z[j] * np.sqrt(var)
        q = np.where((q > lo) & (q < hi), q, 0.5 * (lo + hi))        # the first trial
        answer, r, r_prev = q.copy(), np.full(S, np.inf), np.full(S, np.inf)
        passes, done = np.zeros(S), np.zeros(S, dtype=bool)
        for k in range(1, max_passes + 1):
            live = np.flatnonzero(~done)
            if not live.shape[0]:
                break
            ql = q[live]
            t = (ql[:, None] - mu[live]) * rinv
            F = (0.5 * _erfc(-t)).sum(axis=1) / E
            f = (np.exp(-t * t) * rinv).sum(axis=1) / (E * math.sqrt(math.pi))
            rl = F - p[j]
            r[live], passes[live], answer[live] = rl, k, ql
            below = rl < 0.0
            lo[live] = np.where(below, ql, lo[live])
            hi[live] = np.where(below, hi[live], ql)
            a, b = lo[live], hi[live]
            done[live] = (np.abs(rl) <= ftol) | (b - a <= xtol * width[live])
            with np.errstate(divide='ignore', invalid='ignore'):
                newton = ql - rl / f
            take = (f > 0.0) & (newton > a) & (newton < b) & (np.abs(rl) <= r_prev[live] / 2.0)
            r_prev[live] = np.where(take, np.abs(rl), np.inf)
            q[live] = np.where(take, newton, 0.5 * (a + b))
        base = 6 + 5 * j
        out[:, base], out[:, base + 1], out[:, base + 2], out[:, base + 3], out[:, base + 4] = answer, r, lo, hi, passes
    return out


def predictive_rows_host(X, betas, sd, rinv, y, p, z, max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL):
    """The statement of ``fokl_predictive_rows`` -> the block [S, 6 + 5 Q] (module docstring), in slabs of the rows."""
    X, betas = np.asarray(X, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    sd, rinv = np.asarray(sd, dtype=np.float64).reshape(-1), np.asarray(rinv, dtype=np.float64).reshape(-1)
    p, z = np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(z, dtype=np.float64).reshape(-1)
    y = None if y is None else np.asarray(y, dtype=np.float64).reshape(-1)
    step = max(1, _CHUNK // betas.shape[0])
    return np.concatenate([predictive_rows_from_means(X[i:i + step] @ betas.T, sd, rinv, None if y is None else y[i:i + step],
                                                      p, z, int(max_passes), float(ftol), float(xtol))
                           for i in range(0, X.shape[0], step)])


def _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, quantiles, draws, max_passes, ftol, xtol):
    """Every check of ``predictive`` / ``predictive_host`` (ValueError) and the arguments in the form both use.  Touches no
    device.  betas, sigsqd, mtx, inputs and draws are ``score._prepare``'s to check; ``data`` is optional here."""
    if betas is None or sigsqd is None:
        raise ValueError("predictive needs betas [draws, terms + 1] AND sigsqd [draws]: a fit keeps no sigma^2 per draw, "
                         "resample does")
    if inputs is None:
        raise ValueError("inputs [S, M] are needed: the rows whose predictive distribution is wanted")
    rows = np.asarray(inputs).shape[0] if np.ndim(inputs) else 0
    pr = _score._prepare(betas, sigsqd, mtx, phis, kernel, inputs, np.zeros(rows) if data is None else data, 'lpd', draws)
    if data is None:
        pr['data'] = None
    p = np.asarray(() if quantiles is None else quantiles, dtype=np.float64).reshape(-1)
    if p.shape[0] > MAX_QUANTILES:
        raise ValueError(f"{p.shape[0]} quantiles are asked for, one call takes at most {MAX_QUANTILES} "
                         f"(FOKL_PREDICTIVE_MAX_QUANTILES: they live in registers; call again for more)")
    if not np.isfinite(p).all() or np.any(p <= 0.0) or np.any(p >= 1.0):
        raise ValueError("every quantile must be finite and lie strictly inside (0, 1)")
    if np.unique(p).shape[0] != p.shape[0]:
        raise ValueError("the quantiles repeat a value: each must be asked for once")
    if int(max_passes) != max_passes or max_passes < 0:
        raise ValueError(f"max_passes must be an integer >= 0, it is {max_passes}")
    for name, value in (('ftol', ftol), ('xtol', xtol)):
        if not np.isfinite(value) or value < 0.0:
            raise ValueError(f"{name} must be finite and >= 0, it is {value}")
    if data is None and not p.shape[0]:
        raise ValueError("neither data nor quantiles: nothing would be computed (data gives the PIT, quantiles the intervals)")
    sd, rinv = scales(pr['sigsqd'])
    pr.update(p=p, z=np.array([normal_quantile(v) for v in p]), sd=sd, rinv=rinv, max_passes=int(max_passes), ftol=float(ftol),
              xtol=float(xtol))
    return pr


def pit_ks(pit):
    """max_i |sorted pit_i - (i + 1/2) / S| + 1 / (2 S): the Kolmogorov distance of the PIT values from the uniform."""
    S = pit.shape[0]
    return float(np.max(np.abs(np.sort(pit) - (np.arange(S) + 0.5) / S)) + 0.5 / S)


def _assemble(pr, block):
    """A PredictiveResult from the block [S, 6 + 5 Q]."""
    S, E, p, y = pr['S'], pr['E'], pr['p'], pr['data']
    Q = p.shape[0]
    mean = block[:, 0] + block[:, 1] / E
    var = np.maximum((block[:, 2] - block[:, 1] * block[:, 1] / E) / E, 0.0) + np.mean(pr['sd'] * pr['sd'])
    per = block[:, 6:].reshape(S, Q, 5)
    residual = per[:, :, 1].copy()
    bad = ~(np.abs(residual) <= pr['ftol'])
    res = PredictiveResult(rows=S, draws=E, p=p.copy(), mean=mean, sd=np.sqrt(var), quantiles=per[:, :, 0].copy(),
                           residual=residual, brackets=per[:, :, 2:4].copy(), passes=per[:, :, 4].astype(np.int64),
                           unresolved=int(bad.sum()), unresolved_rows=np.flatnonzero(bad.any(axis=1))[:UNRESOLVED_ROWS_KEPT])
    if y is not None:
        pit = block[:, 5].copy()
        hist = np.bincount(np.minimum((pit * PIT_BINS).astype(np.int64), PIT_BINS - 1), minlength=PIT_BINS) / S
        pairs = [(j, k) for j in range(Q) for k in range(Q) if p[j] < p[k] and p[j] + p[k] == 1.0]
        pairs.sort(key=lambda jk: p[jk[0]])
        q = res['quantiles']
        inside = np.zeros((S, len(pairs)), dtype=bool)
        for n, (j, k) in enumerate(pairs):
            inside[:, n] = (q[:, j] <= y) & (y <= q[:, k])
        coverage = [dict(lower=float(p[j]), upper=float(p[k]), nominal=float(p[k] - p[j]), observed=float(inside[:, n].mean()))
                    for n, (j, k) in enumerate(pairs)]
        res.update(pit=pit, pit_hist=hist, pit_ks=pit_ks(pit), coverage=coverage, inside=inside)
    return res


_SIGNATURE = """
    betas, sigsqd : [E_all, terms + 1] and [E_all]: the draws and their sigma^2, as ``resample`` returns them
    mtx, phis, kernel : the model's (``FoKL.predictive`` passes its own)
    inputs        : [S, M] NORMALISED as the model's inputs are (``FoKL.predictive(clean=True)`` normalises): the rows
    data          : [S] or None: the observed values; with them the PIT, its histogram, coverage and ``inside``
    quantiles     : at most 8 distinct probabilities in (0, 1); () with data gives the PIT only
    draws         : None uses ALL rows of betas, an integer the last ``draws`` rows, an integer array those rows, as
                    ``score``'s does.  Nothing is drawn at random.
    max_passes, ftol, xtol : the pass loop's bound and its two stopping tests (module docstring)

    Returns a ``PredictiveResult`` (a dict with attribute access): rows, draws, p; mean [S] and sd [S] of the predictive;
    quantiles [S, Q], residual [S, Q] (F(q) - p as last evaluated), brackets [S, Q, 2], passes [S, Q]; unresolved (pairs
    with |residual| > ftol) and unresolved_rows (at most 1 000 indices); with data pit [S], pit_hist (20 equal bins, shares
    of the rows), pit_ks, coverage (per pair p_j + p_k = 1: lower, upper, nominal, observed) and inside [S, pairs]."""


def predictive(betas, sigsqd, mtx, phis, kernel, inputs, data=None, quantiles=DEFAULT_QUANTILES, draws=None,
               max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL, device=None):
    """The predictive distribution of every row over every draw on the device.

    device        : device index (default: the process's device, as for ``fit``) or a backend.  The rows replace the
                    dataset uploaded to that device's context, as ``evaluate`` and ``score`` do."""
    pr = _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, quantiles, draws, max_passes, ftol, xtol)
    backend = device if hasattr(device, 'predictive_rows') and hasattr(device, 'build_terms') else None
    if backend is None:
        from . import FoKLRoutines
        backend = FoKLRoutines.device_backend(device)
    columns = _population._DeviceColumns(pr, backend)
    return _assemble(pr, backend.predictive_rows(columns.slots, pr['betas'], pr['sd'], pr['rinv'], pr['data'] is not None,
                                                 pr['p'], pr['z'], pr['max_passes'], pr['ftol'], pr['xtol']))


def predictive_host(betas, sigsqd, mtx, phis, kernel, inputs, data=None, quantiles=DEFAULT_QUANTILES, draws=None,
                    max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL):
    """``predictive`` with columns and passes in numpy on this host: the statement of the computation (module docstring),
    for tests and for reading.  Same arguments, same result fields."""
    pr = _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, quantiles, draws, max_passes, ftol, xtol)
    X = basis_matrix(pr['inputs'], pr['mtx'], pr['phis'], pr['kernel']) if pr['mtx'].shape[0] else np.ones((pr['S'], 1))
    return _assemble(pr, predictive_rows_host(X, pr['betas'], pr['sd'], pr['rinv'], pr['data'], pr['p'], pr['z'],
                                              pr['max_passes'], pr['ftol'], pr['xtol']))


predictive.__doc__ += _SIGNATURE
predictive_host.__doc__ += _SIGNATURE

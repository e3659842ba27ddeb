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

Under Student-t noise (``nu`` finite, 1 <= nu <= NU_MAX: sigsqd_d is the squared SCALE, as ``resample_robust`` draws it) and /
or known row precisions w_i (``weights``; sw_i = sqrt(w_i), isw_i = 1 / sw_i) the passes and the decision rule are the ones above
with these substitutions (``noise_rows_from_means``; ``fokl_predictive_rows_noise``):
  k_id = sw_i / sd_d, formed as (1 / sd_d) sw_i (Student), rinv_d sw_i (Gaussian), stands for rinv_d: t = (q - mu_d) k_id
  Student: F = (sum_d T_nu(t)) / E, f = (sum_d f_nu(t) k_id) / E, pit = (sum_d T_nu((y - mu_d) k_id)) / E; z_j are the quantiles of
  the standard t_nu (``student_quantile``: the root of this module's own CDF)
  Gaussian with weights: the erfc formulas above with k_id for rinv_d
  brackets lo_j = min_d (mu_d + (sd_d isw_i) z_j), hi_j = max_d likewise; the first trial uses var = var_mu + mean_d(sd_d sd_d)
  (isw_i isw_i) -- the scale, so that it exists for every nu; the width is mu_max - mu_min + max_d sd_d isw_i
T_nu and f_nu are ONE stated algorithm, ``student_terms``: the regularised incomplete beta function by its continued fraction,
evaluated by the fraction's forward recurrence (not modified Lentz: no division per step), the direct branch x = nu / (nu +
t^2) where x < (a + 1) / (a + b + 2), a = nu / 2, b = 1 / 2, the mirrored one y = t^2 / (nu + t^2) elsewhere, the lower tail
formed directly, one log1p and one exp serving prefactor and density, under the fixed bound STUDENT_ITERATIONS that the
kernel has too.  Against scipy.special.stdtr its absolute error is 1.1e-15 at most for nu in [1, NU_MAX] and |t| <= 1e6
(tests/test_student_host.py).  With nu = inf and no weights nothing of this is touched: the call is the text above, to the bit.

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
NU_MAX = _capi.PREDICTIVE_NU_MAX                                     # the largest finite nu ``predictive`` takes
STUDENT_ITERATIONS = _capi.PREDICTIVE_STUDENT_ITERATIONS             # the continued fraction's fixed bound, host and device
STUDENT_EPS = 2.0 ** -51                                             # its convergence test
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


gamma_ratio = _score.gamma_ratio


class _Student:
    """The constants of T_nu that the host forms once and the kernel is handed: a = nu / 2, inu = 1 / nu, hp = a + 1/2,
    cn = Gamma(a + 1/2) / (Gamma(a) sqrt(nu pi)) (the density at 0), xb = (a + 1) / (a + 5/2), ha = 0.5 / a and the
    continued fractions' coefficients without their argument, for m = 0 .. STUDENT_ITERATIONS:
      direct   (I_x(a, 1/2)):  even[m] = m (1/2 - m) / ((a + 2m - 1)(a + 2m)),  odd[m] = -(a + m)(a + 1/2 + m) / ((a + 2m)(a + 2m + 1))
      mirrored (I_y(1/2, a)):  even[m] = m (a - m) / ((2m - 1/2)(2m + 1/2)),    odd[m] = -(1/2 + m)(a + 1/2 + m) / ((2m + 1/2)(2m + 3/2))
    as ``table`` [4, STUDENT_ITERATIONS + 1] = direct even, direct odd, mirrored even, mirrored odd."""

    def __init__(self, nu):
        nu = float(nu)
        a = 0.5 * nu
        self.nu, self.a, self.inu, self.hp, self.ha = nu, a, 1.0 / nu, a + 0.5, 0.5 / a
        self.cn = gamma_ratio(a) / math.sqrt(nu * math.pi)
        self.xb = (a + 1.0) / (a + 2.5)
        m = np.arange(STUDENT_ITERATIONS + 1, dtype=np.float64)
        m2 = 2.0 * m
        with np.errstate(invalid='ignore'):                          # even[0] is 0 / 0 at nu = 2, and never read
            even = m * (0.5 - m) / ((a + m2 - 1.0) * (a + m2))
        even[0] = 0.0
        self.table = np.stack([even, -(a + m) * (a + 0.5 + m) / ((a + m2) * (a + m2 + 1.0)),
                               m * (a - m) / ((m2 - 0.5) * (m2 + 0.5)), -(0.5 + m) * (a + 0.5 + m) / ((m2 + 0.5) * (m2 + 1.5))])


_STUDENT = {}


def student_constants(nu):
    nu = float(nu)
    if nu not in _STUDENT:
        if len(_STUDENT) > 64:
            _STUDENT.clear()
        _STUDENT[nu] = _Student(nu)
    return _STUDENT[nu]


def student_terms(t, nu):
    """(T_nu(t), f_nu(t)): CDF and density of Student's t, the ONE algorithm that the kernel repeats to the operation
    (csrc/fokl_student.inc: student_terms).  With the constants of ``_Student``:
      r = (t t) inu; L = log1p(r); x = 1 / (1 + r); f = cn exp(-hp L)                 (x = nu / (nu + t^2), r x = t^2 / (nu + t^2))
      direct where x < xb: z = x, coefficients of I_x(a, 1/2); else mirrored: z = r x, coefficients of I_y(1/2, a)
      the continued fraction h = 1 / (1 + d_1 / (1 + d_2 / (1 + ...))), d_{2m+1} = odd[m] z, d_{2m} = even[m] z, by its forward
      recurrence (no division): (A0, B0) = (1, 1), (A1, B1) = (1, 1 + odd[0] z); for m = 1 .. STUDENT_ITERATIONS
          A2 = A1 + (even[m] z) A0, B2 likewise; A3 = A2 + (odd[m] z) A1, B3 likewise; (A0, B0, A1, B1) <- (A2, B2, A3, B3)
          converged, and frozen from here on, when |A3 B2 - A2 B3| <= STUDENT_EPS |A3 B2|
      h = A1 / B1; g = f t h
      direct: v = ha |g|, T = v for t < 0 and 1 - v otherwise (x^a y^(1/2) / B(a, 1/2) = f |t|: one exp serves both);
      mirrored: T = 0.5 + g.
    The lower tail is v itself, never 1 - something.  Every partial numerator is below 1 in size, so A and B stay within
    2^(2 STUDENT_ITERATIONS) and need no rescaling."""
    k = student_constants(nu)
    t = np.asarray(t, dtype=np.float64)
    shape = t.shape
    t = t.reshape(-1)
    r = (t * t) * k.inu
    L = np.log1p(r)
    x = 1.0 / (1.0 + r)
    f = k.cn * np.exp(-k.hp * L)
    direct = x < k.xb
    z = np.where(direct, x, r * x)
    even = lambda m: np.where(direct, k.table[0, m], k.table[2, m])
    odd = lambda m: np.where(direct, k.table[1, m], k.table[3, m])
    A0, B0, A1, B1 = np.ones_like(t), np.ones_like(t), np.ones_like(t), 1.0 + odd(0) * z
    live = np.ones(t.shape, dtype=bool)
    for m in range(1, STUDENT_ITERATIONS + 1):
        if not live.any():
            break
        dE, dO = even(m) * z, odd(m) * z
        A2, B2 = A1 + dE * A0, B1 + dE * B0
        A3, B3 = A2 + dO * A1, B2 + dO * B1
        A0, B0, A1, B1 = (np.where(live, new, old) for new, old in ((A2, A0), (B2, B0), (A3, A1), (B3, B1)))
        live &= ~(np.abs(A3 * B2 - A2 * B3) <= STUDENT_EPS * np.abs(A3 * B2))
    g = f * t * (A1 / B1)
    v = k.ha * np.abs(g)
    T = np.where(direct, np.where(t < 0.0, v, 1.0 - v), 0.5 + g)
    return T.reshape(shape), f.reshape(shape)


def student_cdf(t, nu):
    """T_nu(t) (``student_terms``)."""
    return student_terms(t, nu)[0]


def student_pdf(t, nu):
    """f_nu(t) = cn exp(-(nu + 1) / 2 log1p(t^2 / nu)) (``student_terms``)."""
    return student_terms(t, nu)[1]


def student_quantile(p, nu):
    """z with student_cdf(z, nu) = p as closely as ``student_cdf`` resolves it: bisection from a bracket that doubles, then
    safeguarded Newton steps on this module's own CDF and density (no scipy: the kernel's residual is measured with this
    CDF, so the quantile has to be ITS root); the upper half by symmetry, 1 - p being exact there."""
    p = float(p)
    if p > 0.5:
        return -student_quantile(1.0 - p, nu)
    if p == 0.5:
        return 0.0
    F = lambda v: float(student_cdf(v, nu))
    lo, hi = -1.0, 0.0
    while F(lo) > p:
        lo *= 2.0
    z, best, best_gap = 0.5 * (lo + hi), None, math.inf
    for _ in range(200):
        cdf, pdf = (float(v) for v in student_terms(z, nu))
        gap = abs(cdf - p)
        if gap < best_gap:
            best, best_gap = z, gap
        if cdf < p:
            lo = z
        else:
            hi = z
        if gap == 0.0 or not (lo < 0.5 * (lo + hi) < hi):
            break
        step = z - (cdf - p) / pdf if pdf > 0.0 else lo
        z = step if lo < step < hi else 0.5 * (lo + hi)
    return best


def scales(sigsqd):
    """(sd, rinv) = (sqrt(sigsqd), 1 / (sd sqrt(2))) with libm, as both ``predictive`` and ``predictive_host`` pass them on."""
    sd = np.array([math.sqrt(float(s)) for s in np.reshape(sigsqd, -1)])
    rinv = np.array([1.0 / (float(s) * math.sqrt(2.0)) for s in sd])
    return sd, rinv



def mixture_cdf(mu, rinv, q):
    """F [S] of the mixtures with means mu [S, E] at q [S]: (sum_d 0.5 erfc(-(q - mu_d) rinv_d)) / E."""
    t = (np.reshape(q, (-1, 1)) - mu) * rinv
    return (0.5 * _erfc(-t)).sum(axis=1) / mu.shape[1]


def noise_rows_from_means(mu, sd, rinv, y, p, z, max_passes, ftol, xtol, nu, sw):
    """``predictive_rows_from_means`` under Student-t noise (finite ``nu``) and / or row precisions (``sw`` [S] = sqrt(w), None:
    ones): the same passes and the same decision rule with the substitutions of the module docstring."""
    S, E = mu.shape
    Q = p.shape[0]
    student = bool(np.isfinite(nu))
    sw = np.ones(S) if sw is None else sw
    isw = 1.0 / sw
    k = (1.0 / sd if student else rinv)[None, :] * sw[:, None]       # [S, E]: what turns q - mu_d into the argument of the CDF
    out = np.zeros((S, 6 + 5 * Q))
    d = mu - mu[:, :1]
    s1, s2 = d.sum(axis=1), (d * d).sum(axis=1)
    mu_min, mu_max = mu.min(axis=1), mu.max(axis=1)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = mu[:, 0], s1, s2, mu_min, mu_max
    if y is not None:
        if student:
            out[:, 5] = student_terms((y[:, None] - mu) * k, nu)[0].sum(axis=1) / E
        else:
            out[:, 5] = (0.5 * _erfc((mu - y[:, None]) * k)).sum(axis=1) / E
    if not Q:
        return out
    mean = mu[:, 0] + s1 / E
    var = np.maximum((s2 - s1 * s1 / E) / E, 0.0) + np.mean(sd * sd) * (isw * isw)
    width = mu_max - mu_min + sd.max() * isw
    for j in range(Q):
        c = mu + (sd[None, :] * isw[:, None]) * z[j]
        lo, hi = c.min(axis=1), c.max(axis=1)
        q = mean + z[j] * np.sqrt(var)
        q = np.where((q > lo) & (q < hi), q, 0.5 * (lo + hi))        # the first trial
        answer, r, r_prev = q.copy(), np.full(S, np.inf), np.full(S, np.inf)
        passes, done = np.zeros(S), np.zeros(S, dtype=bool)
        for n in range(1, max_passes + 1):
            live = np.flatnonzero(~done)
            if not live.shape[0]:
                break
            ql, kl = q[live], k[live]
            t = (ql[:, None] - mu[live]) * kl
            if student:
                T, dens = student_terms(t, nu)
                F, f = T.sum(axis=1) / E, (dens * kl).sum(axis=1) / E
            else:
                F = (0.5 * _erfc(-t)).sum(axis=1) / E
                f = (np.exp(-t * t) * kl).sum(axis=1) / (E * math.sqrt(math.pi))
            rl = F - p[j]
            r[live], passes[live], answer[live] = rl, n, ql
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


def predictive_rows_from_means(mu, sd, rinv, y, p, z, max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL, nu=np.inf, sw=None):
    """The statement from the means mu [S, E] = X betas' on: the block [S, 6 + 5 Q] (module docstring)."""
    if np.isfinite(nu) or sw is not None:
        return noise_rows_from_means(mu, sd, rinv, y, p, z, max_passes, ftol, xtol, nu, sw)
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


def predictive_rows_host(X, betas, sd, rinv, y, p, z, max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL, nu=np.inf, sw=None):
    """The statement of ``fokl_predictive_rows`` (and, with ``nu`` or ``sw``, of ``fokl_predictive_rows_noise``) -> the block
    [S, 6 + 5 Q] (module docstring), in slabs of the rows."""
    X, betas = np.asarray(X, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    sd, rinv = np.asarray(sd, dtype=np.float64).reshape(-1), np.asarray(rinv, dtype=np.float64).reshape(-1)
    p, z = np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(z, dtype=np.float64).reshape(-1)
    y = None if y is None else np.asarray(y, dtype=np.float64).reshape(-1)
    sw = None if sw is None else np.asarray(sw, dtype=np.float64).reshape(-1)
    step = max(1, _CHUNK // betas.shape[0])
    return np.concatenate([predictive_rows_from_means(X[i:i + step] @ betas.T, sd, rinv, None if y is None else y[i:i + step],
                                                      p, z, int(max_passes), float(ftol), float(xtol), float(nu),
                                                      None if sw is None else sw[i:i + step])
                           for i in range(0, X.shape[0], step)])


def _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, quantiles, draws, max_passes, ftol, xtol, nu=np.inf, weights=None):
    """Every check of ``predictive`` / ``predictive_host`` (ValueError) and the arguments in the form both use.  Touches no
    device.  betas, sigsqd, mtx, inputs, draws, nu and weights are ``score._prepare``'s to check; ``data`` is optional here."""
    if betas is None or sigsqd is None:
        raise ValueError("predictive needs betas [draws, terms + 1] AND sigsqd [draws]: a fit keeps no sigma^2 per draw, "
                         "resample does")
    if inputs is None:
        raise ValueError("inputs [S, M] are needed: the rows whose predictive distribution is wanted")
    rows = np.asarray(inputs).shape[0] if np.ndim(inputs) else 0
    pr = _score._prepare(betas, sigsqd, mtx, phis, kernel, inputs, np.zeros(rows) if data is None else data, 'lpd', draws, nu,
                         weights)
    if data is None:
        pr['data'] = None
    nu = pr['nu']
    if np.isfinite(nu) and nu > NU_MAX:
        raise ValueError(f"nu = {nu:g} is beyond FOKL_PREDICTIVE_NU_MAX = {NU_MAX}, as far as the t CDF's continued fraction is "
                         f"bounded and tested (at such a nu the noise is Gaussian to 1 / (4 nu): resample_robust(nu=np.inf))")
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
    pr.update(p=p, z=np.array([student_quantile(v, nu) if np.isfinite(nu) else normal_quantile(v) for v in p]), sd=sd, rinv=rinv, max_passes=int(max_passes), ftol=float(ftol),
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
    var = np.maximum((block[:, 2] - block[:, 1] * block[:, 1] / E) / E, 0.0)
    nu, sw = pr.get('nu', np.inf), pr.get('sw')
    if np.isfinite(nu) or sw is not None:                            # the predictive's own variance: a t scale is none
        inflate = np.inf if nu <= 2.0 else nu / (nu - 2.0) if np.isfinite(nu) else 1.0
        var = var + np.mean(pr['sd'] * pr['sd']) * inflate / (1.0 if sw is None else sw * sw)
        if nu <= 1.0:
            mean = np.full(S, np.nan)
    else:
        var = var + np.mean(pr['sd'] * pr['sd'])
    per = block[:, 6:].reshape(S, Q, 5)
    residual = per[:, :, 1].copy()
    bad = ~(np.abs(residual) <= pr['ftol'])
    res = PredictiveResult(rows=S, draws=E, p=p.copy(), mean=mean, sd=np.sqrt(var), quantiles=per[:, :, 0].copy(),
                           residual=residual, brackets=per[:, :, 2:4].copy(), passes=per[:, :, 4].astype(np.int64),
                           unresolved=int(bad.sum()), unresolved_rows=np.flatnonzero(bad.any(axis=1))[:UNRESOLVED_ROWS_KEPT],
                           nu=nu, noise='student' if np.isfinite(nu) else 'gaussian', weighted=sw is not None)
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
    nu            : np.inf (default): Gaussian noise; finite, 1 <= nu <= NU_MAX: sigsqd is the squared SCALE of Student-t noise
                    with nu degrees of freedom, as ``resample_robust`` draws it
    weights       : None (ones) or [S] known relative precisions of the rows, finite and > 0: row i's noise has the scale
                    sqrt(sigsqd / w_i).  With nu = np.inf and no weights the call is today's, to the bit.

    Returns a ``PredictiveResult`` (a dict with attribute access): rows, draws, p; mean [S] and sd [S] of the predictive;
    quantiles [S, Q], residual [S, Q] (F(q) - p as last evaluated), brackets [S, Q, 2], passes [S, Q]; unresolved (pairs
    with |residual| > ftol) and unresolved_rows (at most 1 000 indices); with data pit [S], pit_hist (20 equal bins, shares
    of the rows), pit_ks, coverage (per pair p_j + p_k = 1: lower, upper, nominal, observed) and inside [S, pairs]; nu,
    noise ('gaussian' or 'student') and weighted.  Under t noise sd is the predictive's own, sqrt(var_mu + mean(sigsqd) nu /
    ((nu - 2) w_i)): inf for nu <= 2, and mean is NaN for nu <= 1."""


def predictive(betas, sigsqd, mtx, phis, kernel, inputs, data=None, quantiles=DEFAULT_QUANTILES, draws=None,
               max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL, device=None, nu=np.inf, weights=None):
    """The predictive distribution of every row over every draw on the device.

    device        : device index (default: the process's device, as for ``fit``) or a backend.  The rows replace the
                    dataset uploaded to that device's context, as ``evaluate`` and ``score`` do."""
    pr = _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, quantiles, draws, max_passes, ftol, xtol, nu, weights)
    backend = device if hasattr(device, 'predictive_rows') and hasattr(device, 'build_terms') else None
    if backend is None:
        from . import FoKLRoutines
        backend = FoKLRoutines.device_backend(device)
    columns = _population._DeviceColumns(pr, backend)
    args = (columns.slots, pr['betas'], pr['sd'], pr['rinv'], pr['data'] is not None, pr['p'], pr['z'], pr['max_passes'],
            pr['ftol'], pr['xtol'])
    if np.isfinite(pr['nu']) or pr['sw'] is not None:
        return _assemble(pr, backend.predictive_rows_noise(*args, nu=pr['nu'], sw=pr['sw']))
    return _assemble(pr, backend.predictive_rows(*args))


def predictive_host(betas, sigsqd, mtx, phis, kernel, inputs, data=None, quantiles=DEFAULT_QUANTILES, draws=None,
                    max_passes=MAX_PASSES, ftol=FTOL, xtol=XTOL, nu=np.inf, weights=None):
    """``predictive`` with columns and passes in numpy on this host: the statement of the computation (module docstring),
    for tests and for reading.  Same arguments, same result fields."""
    pr = _prepare(betas, sigsqd, mtx, phis, kernel, inputs, data, quantiles, draws, max_passes, ftol, xtol, nu, weights)
    X = basis_matrix(pr['inputs'], pr['mtx'], pr['phis'], pr['kernel']) if pr['mtx'].shape[0] else np.ones((pr['S'], 1))
    return _assemble(pr, predictive_rows_host(X, pr['betas'], pr['sd'], pr['rinv'], pr['data'], pr['p'], pr['z'],
                                              pr['max_passes'], pr['ftol'], pr['xtol'], pr['nu'], pr['sw']))


predictive.__doc__ += _SIGNATURE
predictive_host.__doc__ += _SIGNATURE

"""
A robust posterior of a fitted model: Gibbs chains under Student-t noise and given row weights, sampled on the device.

``fit`` and ``resample`` assume Gaussian noise with one variance for every row.  Here

    y_i = x_i . beta + eps_i,   eps_i | lam_i ~ N(0, sigsqd / (w_i lam_i)),   lam_i ~ Gamma(nu / 2, rate nu / 2)

so that eps_i is Student-t with ``nu`` degrees of freedom (scale mixture of normals); beta | sigsqd, tausqd ~ N(0, sigsqd
tausqd I); sigsqd and tausqd are inverse gammas with the fit's ``a, b, atau, btau`` exactly as ``resample`` reads them.  The
row weights ``w`` are given (default ones: averages of replicates, two instruments), ``nu`` is fixed (default 4;
``nu=np.inf`` means lam = 1: Gaussian noise, and with w = 1 exactly ``resample``'s posterior).  With per-row precisions
the Gram X' diag(w lam) X changes every iteration, so nothing of ``resample``'s eigenbasis survives: every iteration is a
weighted pass over all rows.  State (beta, sigsqd, tausqd); iteration k of chain c:

  1. row pass   k = 0 or nu = inf: lam_i = 1.  Otherwise r_i = y_i - x_i . beta, lam_i = g_i / ((nu + w_i r_i^2 / sigsqd) / 2)
                with g_i a standard gamma of shape (nu + 1) / 2 by Marsaglia-Tsang (``resample``'s constants and attempt cap; a
                row that exhausts the cap is NaN and flags the chain).  G = [1|X|y]' diag(w lam) [1|X|y] with the blocks
                G_xx, c = G_xy, G_yy.
  2. beta       A = G_xx + I / tausqd = L L' (Cholesky, no pivoting); L u = c; L' beta = u + sqrt(sigsqd) z, z ~ N(0, I)
                (beta = A^-1 c + sqrt(sigsqd) L^-T z).
  3. sigsqd     S = G_yy - 2 beta . c + beta' G_xx beta; bstar = b + (S + beta . beta / tausqd) / 2;
                sigsqd = 1 / Gamma(astar, 1 / bstar), astar = a + 1 + n / 2 + (P + 1) / 2 (FR:1508: the reference's convention,
                so that nu = inf, w = 1 targets ``resample``'s posterior).  bstar < 0 or a non-positive pivot flags the chain:
                it is NaN from there on and touches no other chain.
  4. tausqd     = 1 / Gamma(atau + P / 2, 1 / (beta . beta / (2 sigsqd) + btau)).

Random numbers: the fifth Philox family of csrc/fokl_philox.h, key (seed, chain), counter (iteration, purpose + 16 attempt,
index, 4), purposes ``_capi.ROB_*``: index = row for the normal and the uniform of a lam variate's attempt, index =
coordinate for z, index 0 for the two variates of sigsqd and tausqd.  ``_capi.robust_rng`` draws them on the host.  Nothing
depends on a stream position: chain c of many is chain c alone, ``thin`` only selects rows, numpy's stream is not touched.

On the device (csrc/fokl_robust_device.inc) an iteration is three kernels queued on the context's stream with no host round
trip: ``robust_pass_kernel`` (the hot path: residuals, lam and the weighted Gram on the fp64 matrix pipe), a reduce over the
workgroups' partial Grams in a fixed order, and ``robust_step_kernel`` (steps 2-4, one workgroup per chain).  Without the
library or a gfx950 device ``resample_robust`` raises; there is no host fallback.  ``pass_host``, ``step_host`` and
``robust_host`` are the same computation in numpy with the same Philox numbers: the STATEMENT the kernels are tested against.
"""
import numpy as np

from . import _capi
from . import getKernels
from . import resample as _rs
from .resample import ResampleResult, wave_sum, gamma_constants, split_rhat_from_sums, start_values

MAX_COLUMNS = _capi.ROBUST_MAX_COLUMNS            # P + 1 <= 127: [1 | X | y] fills eight 16-column blocks
ATTEMPT_CAP = _capi.RESAMPLE_ATTEMPT_CAP
FLAG_NONE, FLAG_BSTAR_NEGATIVE, FLAG_ATTEMPT_CAP, FLAG_PIVOT = 0, 1, 2, 3
_KEEP = ('betas', None)


# ---------------------------------------------------------------------------------------------------------
# the statement of the three kernels
# ---------------------------------------------------------------------------------------------------------

def hyper_of(a, b, atau, btau, n, P):
    """What a step needs of the hyper-parameters: dict(astar, atau_star, b, btau) (FR:1508-1510)."""
    return dict(astar=float(a) + 1 + n / 2 + (P + 1) / 2, atau_star=float(atau) + P / 2, b=float(b), btau=float(btau))


def row_gamma(shape, seed, chain, iteration, n, attempt_cap=0):
    """One standard gamma variate of ``shape`` >= 1 per row 0 .. n - 1 as the row pass of chain ``chain`` draws it at
    ``iteration`` -> (g [n], attempts [n] int32); NaN where ``attempt_cap`` attempts were rejected."""
    b, c = gamma_constants(shape)
    cap = int(attempt_cap) or ATTEMPT_CAP
    g = np.full(n, np.nan)
    attempts = np.zeros(n, dtype=np.int32)
    todo = np.ones(n, dtype=bool)
    with np.errstate(all='ignore'):
        for a in range(cap):
            if not todo.any():
                break
            attempts[todo] += 1
            x = _capi.robust_rng(seed, chain, iteration, _capi.ROB_LAM_NORMAL, n, attempt=a)
            u = _capi.robust_rng(seed, chain, iteration, _capi.ROB_LAM_UNIFORM, n, attempt=a)
            v1 = 1.0 + c * x
            v, x2 = (v1 * v1) * v1, x * x
            accept = (v1 > 0.0) & ((u < 1.0 - 0.0331 * (x2 * x2)) | (np.log(u) < 0.5 * x2 + b * ((1.0 - v) + np.log(v))))
            now = todo & accept
            g[now] = b * v[now]
            todo &= ~accept
    return g, attempts


def row_product(X, beta):
    """x_i . beta in the pass kernel's order: quarter q of the workgroup adds the columns q, q + 4, ... in ascending order,
    then (q0 + q1) + (q2 + q3)."""
    parts = np.zeros((4, X.shape[0]))
    for k in range(X.shape[1]):
        parts[k & 3] = parts[k & 3] + X[:, k] * beta[k]
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def pass_host(X, y, w, beta, sigsqd, nu, seed, chain, iteration, attempt_cap=0):
    """The statement of ``DeviceContext.robust_pass`` (step 1): X [n, P + 1] (the intercept's column included), y, w [n]
    (None: ones) -> (G [P + 2, P + 2], lam [n], attempts [n] int32).  ``beta`` and ``sigsqd`` are not read at iteration 0 or
    under nu = inf."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    if int(iteration) == 0 or np.isinf(nu):
        lam, attempts = np.ones(n), np.zeros(n, dtype=np.int32)
    else:
        g, attempts = row_gamma((float(nu) + 1.0) / 2.0, seed, chain, iteration, n, attempt_cap)
        r = y - row_product(X, np.asarray(beta, dtype=np.float64).reshape(-1))
        with np.errstate(all='ignore'):
            lam = g / (0.5 * (float(nu) + (w * (r * r)) / float(sigsqd)))
    Z = np.concatenate([X, y[:, None]], axis=1)
    with np.errstate(all='ignore'):
        G = Z.T @ (Z * (w * lam)[:, None])
    return G, lam, attempts


def _state_gamma(seed, chain, iteration, shape, pn, pu, attempt_cap):
    """One standard gamma variate of sigma^2 / tau^2 (index 0, the attempt in the purpose word) -> (value, attempts)."""
    b, c = gamma_constants(shape)
    cap = int(attempt_cap) or ATTEMPT_CAP
    for a in range(cap):
        x = float(_capi.robust_rng(seed, chain, iteration, pn, 1, attempt=a)[0])
        u = float(_capi.robust_rng(seed, chain, iteration, pu, 1, attempt=a)[0])
        v1 = 1.0 + c * x
        if v1 <= 0.0:
            continue
        v, x2 = (v1 * v1) * v1, x * x
        with np.errstate(divide='ignore'):
            if u < 1.0 - 0.0331 * (x2 * x2) or np.log(u) < 0.5 * x2 + b * ((1.0 - v) + np.log(v)):
                return b * v, a + 1
    return np.nan, cap


def cholesky_lower(A):
    """A = L L' without pivoting in the step kernel's order (right-looking: column j, then the trailing block less its outer
    product) -> (L, ok); a pivot that is not positive makes the column, and everything after it, NaN."""
    L = np.array(A, dtype=np.float64)
    p1 = L.shape[0]
    ok = True
    with np.errstate(all='ignore'):
        for j in range(p1):
            pivot = L[j, j]
            if not pivot > 0.0:
                ok, pivot = False, np.nan
            d = np.sqrt(pivot)
            L[j, j] = d
            L[j + 1:, j] = L[j + 1:, j] / d
            col = L[j + 1:, j]
            L[j + 1:, j + 1:] = L[j + 1:, j + 1:] - col[:, None] * col[None, :]
    return np.tril(L), ok


def residual_form(G, beta):
    """(S, beta . beta) with S = G_yy - 2 beta . c + beta' G_xx beta = sum_i w_i lam_i (y_i - x_i . beta)^2 from the Gram alone,
    in the step kernel's order: G_xx beta with the columns in ascending order, the three sums by ``resample.wave_sum``'s tree."""
    G = np.asarray(G, dtype=np.float64)
    p1 = G.shape[0] - 1
    Gxx, c, Gyy = G[:p1, :p1], G[:p1, p1], G[p1, p1]
    gb = np.zeros(p1)
    with np.errstate(all='ignore'):
        for j in range(p1):
            gb = gb + Gxx[:, j] * beta[j]
        q_bc, q_bgb, q_bb = (float(wave_sum(v[None, :])[0]) for v in (beta * c, beta * gb, beta * beta))
        return (Gyy - 2.0 * q_bc) + q_bgb, q_bb


def _step(G, sigsqd, tausqd, hyper, seed, chain, iteration, attempt_cap=0):
    G = np.triu(np.asarray(G, dtype=np.float64))                       # G is symmetric: its upper triangle is read
    G = G + np.triu(G, 1).T
    p1 = G.shape[0] - 1
    Gxx, c, Gyy = G[:p1, :p1], G[:p1, p1], G[p1, p1]
    with np.errstate(all='ignore'):
        gs, att_s = _state_gamma(seed, chain, iteration, hyper['astar'], _capi.ROB_SIG_NORMAL, _capi.ROB_SIG_UNIFORM, attempt_cap)
        gt, att_t = _state_gamma(seed, chain, iteration, hyper['atau_star'], _capi.ROB_TAU_NORMAL, _capi.ROB_TAU_UNIFORM,
                                 attempt_cap)
        z = _capi.robust_rng(seed, chain, iteration, _capi.ROB_BETA, p1)
        inv_tau, root_sig = 1.0 / tausqd, np.sqrt(sigsqd)
        A = Gxx.copy()
        A[np.diag_indices(p1)] = np.diag(Gxx) + inv_tau
        L, ok = cholesky_lower(A)
        u = c.copy()
        for j in range(p1):                                              # L u = c, column by column
            u[j] = u[j] / L[j, j]
            u[j + 1:] = u[j + 1:] - L[j + 1:, j] * u[j]
        rhs = u + root_sig * z
        beta = rhs
        for j in range(p1 - 1, -1, -1):                                  # L' beta = u + sqrt(sigsqd) z
            beta[j] = beta[j] / L[j, j]
            beta[:j] = beta[:j] - L[j, :j] * beta[j]
        S, q_bb = residual_form(G, beta)
        bstar = hyper['b'] + 0.5 * (S + q_bb / tausqd)
        negative = bstar < 0.0
        sig = np.nan if negative else 1.0 / ((1.0 / bstar) * gs)
        btau_star = (1.0 / (2.0 * sig)) * q_bb + hyper['btau']
        tau = 1.0 / ((1.0 / btau_star) * gt)
    flag = FLAG_NONE
    if negative:
        flag = FLAG_BSTAR_NEGATIVE
    elif np.isnan(gs) or np.isnan(gt) or np.isnan(Gyy):                # (a row of the pass met the cap: G is NaN)
        flag = FLAG_ATTEMPT_CAP
    elif not ok:
        flag = FLAG_PIVOT
    return beta, float(sig), float(tau), flag, att_s, att_t, S


def step_host(G, sigsqd, tausqd, hyper, seed, chain, iteration, attempt_cap=0):
    """The statement of ``DeviceContext.robust_step`` (steps 2-4) on a given G [P + 2, P + 2] -> (beta [P + 1], sigsqd,
    tausqd, flag); ``hyper`` is ``hyper_of``'s dict.  The flag is FLAG_BSTAR_NEGATIVE, FLAG_PIVOT (a pivot of the Cholesky
    factor was not positive) or FLAG_ATTEMPT_CAP (a gamma variate met the cap, here or in a row of the pass: G is NaN)."""
    return _step(G, sigsqd, tausqd, hyper, seed, chain, iteration, attempt_cap)[:4]


def robust_host(X, y, w, nu, hyper, shift, sigsqd0, tausqd0, burnin, draws, thin, seed, rows=True, attempt_cap=0,
                chain_ids=None):
    """The statement of ``DeviceContext.robust_chains`` (fokl_robust_chains): the loop over ``pass_host`` and ``step_host``
    with ``resample.chains_host``'s bookkeeping, same dict:

      betas [chains, kept, P + 1], sigsqd, tausqd [chains, kept]   the kept iterations' draws (None without ``rows``)
      attempts [chains, kept] int64                              Marsaglia-Tsang attempts of the row's iteration, lam's included
      sums [chains, 3, 2, P + 3]                                 as ``resample``'s, of beta - shift | sigsqd | tausqd
      counts [chains, 4]                                         first flagged iteration or -1, why (FLAG_*), attempts in all,
                                                                 the most one variate took
      lam_sum [chains, n]                                        the sum of lam_i over the passes of iterations >= burnin"""
    X = np.asarray(X, dtype=np.float64)
    n, p1 = X.shape
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    shift = np.asarray(shift, dtype=np.float64).reshape(-1)
    sig0 = np.array(np.reshape(sigsqd0, -1), dtype=np.float64)
    tau0 = np.array(np.reshape(tausqd0, -1), dtype=np.float64)
    chains = sig0.shape[0]
    ids = np.arange(chains) if chain_ids is None else np.asarray(chain_ids).reshape(-1)
    burnin, draws, thin = int(burnin), int(draws), int(thin)
    kept, half, total = -(-draws // thin), draws // 2, burnin + draws
    b_out = np.empty((chains, kept, p1)) if rows else None
    sig_out = np.empty((chains, kept)) if rows else None
    tau_out = np.empty((chains, kept)) if rows else None
    att_out = np.zeros((chains, kept), dtype=np.int64) if rows else None
    sums = np.zeros((chains, _capi.RESAMPLE_SEGMENTS, 2, p1 + 2))
    counts = np.zeros((chains, 4), dtype=np.int64)
    counts[:, 0] = -1
    lam_sum = np.zeros((chains, n))
    fixed = pass_host(X, y, w, None, 1.0, np.inf, seed, 0, 0)           # lam = 1: the Gram of iteration 0 and of nu = inf
    with np.errstate(all='ignore'):
        for c in range(chains):
            sig, tau, beta = sig0[c], tau0[c], None
            run = np.zeros((2, p1 + 2))
            for k in range(total):
                if k == 0 or np.isinf(nu):
                    G, lam, att = fixed
                else:
                    G, lam, att = pass_host(X, y, w, beta, sig, nu, seed, ids[c], k, attempt_cap)
                beta, sig, tau, flag, att_s, att_t, _ = _step(G, sig, tau, hyper, seed, ids[c], k, attempt_cap)
                if flag and counts[c, 0] < 0:
                    counts[c, 0], counts[c, 1] = k, flag
                spent = int(att.sum(dtype=np.int64)) + att_s + att_t
                counts[c, 2] += spent
                counts[c, 3] = max(counts[c, 3], att_s, att_t, int(att.max()) if n else 0)
                j = k - burnin
                if j < 0:
                    continue
                lam_sum[c] += lam
                if rows and j % thin == 0:
                    r = j // thin
                    b_out[c, r], sig_out[c, r], tau_out[c, r], att_out[c, r] = beta, sig, tau, spent
                dev = beta - shift
                run[0, :p1] += dev
                run[1, :p1] += dev * dev
                run[0, p1] += sig
                run[1, p1] += sig * sig
                run[0, p1 + 1] += tau
                run[1, p1 + 1] += tau * tau
                if j + 1 == half or j + 1 == 2 * half:
                    sums[c, 0 if j + 1 == half else 1] = run
                    run[:] = 0.0
            if draws & 1:
                sums[c, 2] = run
    return dict(betas=b_out, sigsqd=sig_out, tausqd=tau_out, attempts=att_out, sums=sums, counts=counts, lam_sum=lam_sum)


# ---------------------------------------------------------------------------------------------------------
# one call
# ---------------------------------------------------------------------------------------------------------

def _prepare(mtx, phis, kernel, inputs, data, a, b, atau, btau, nu, weights, chains, draws, burnin, thin, seed, init, keep):
    """Every check of ``resample_robust`` / ``resample_robust_host`` (ValueError).  Touches no device."""
    if keep not in _KEEP:
        raise ValueError(f"keep must be one of {_KEEP}")
    if mtx is not None and np.size(mtx) and np.atleast_2d(mtx).shape[0] + 1 > MAX_COLUMNS:
        raise ValueError(f"the model has {np.atleast_2d(mtx).shape[0] + 1} columns, the robust pass holds at most {MAX_COLUMNS} "
                         f"([1 | X | y] fills eight 16-column blocks of the weighted Gram)")
    p = _rs._prepare(mtx, phis, kernel, inputs, data, a, b, atau, btau, chains, draws, burnin, thin, seed, init, keep)
    try:
        nu = float(nu)
    except (TypeError, ValueError):
        raise ValueError("nu must be a number >= 1 (np.inf: Gaussian noise)") from None
    if not nu >= 1.0:
        raise ValueError(f"nu = {nu} < 1 or NaN: the gamma sampler of the latent precisions is Marsaglia-Tsang's for shapes "
                         f"(nu + 1) / 2 >= 1")
    n = p['n']
    if weights is None:
        w = np.ones(n)
    else:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != n:
            raise ValueError(f"weights must hold one value per row ({n}), there are {w.shape[0]}")
        if not np.isfinite(w).all() or not (w > 0.0).all():
            raise ValueError("weights must be finite and > 0 (drop a row instead of giving it no weight)")
    p.update(nu=nu, weights=np.ascontiguousarray(w), hyper=hyper_of(p['a'], p['b'], p['atau'], p['btau'], n, p['P']))
    return p


def _shift(p, G0):
    """The sums are accumulated about the conditional mean at the reference start, from the Gram with lam = 1."""
    p1 = p['P'] + 1
    return np.linalg.solve(G0[:p1, :p1] + np.eye(p1) * ((1.0 + p['atau']) / p['btau']), G0[:p1, p1])


def _assemble(p, raw, sig0, tau0, shift):
    chains, draws, keep, nu = p['chains'], p['draws'], p['keep'], p['nu']
    p1 = p['P'] + 1
    counts, sums = raw['counts'], raw['sums']
    good = counts[:, 0] < 0
    res = ResampleResult(chains=chains, draws=draws, burnin=p['burnin'], thin=p['thin'], seed=p['seed'], keep=keep,
                         kept=-(-draws // p['thin']), sigsqd0=sig0, tausqd0=tau0, flagged=~good, flagged_at=counts[:, 0].copy(),
                         flag_reason=counts[:, 1].copy(), attempts_total=int(counts[:, 2].sum()),
                         attempts_max=int(counts[:, 3].max()), sums=sums, shift=shift, astar=p['hyper']['astar'],
                         atau_star=p['hyper']['atau_star'], nu=nu, noise='gaussian' if np.isinf(nu) else 'student',
                         weights=p['weights'])
    with np.errstate(all='ignore'):
        s = (sums[:, 0, 0] + sums[:, 1, 0]) + sums[:, 2, 0]
        q = (sums[:, 0, 1] + sums[:, 1, 1]) + sums[:, 2, 1]
        mean = s / draws
        var = np.maximum(q / draws - mean * mean, 0.0) * (draws / (draws - 1) if draws > 1 else np.nan)
        res['weight_mean'] = (raw['lam_sum'][good] / draws).mean(axis=0) if good.any() else np.full(p['n'], np.nan)
    mean[:, :p1] += shift
    res['chain_mean'] = dict(betas=mean[:, :p1], sigsqd=mean[:, p1], tausqd=mean[:, p1 + 1])
    res['chain_var'] = dict(betas=var[:, :p1], sigsqd=var[:, p1], tausqd=var[:, p1 + 1])
    rh = split_rhat_from_sums(sums[good], draws)
    res['rhat'] = dict(betas=rh[:p1], sigsqd=float(rh[p1]), tausqd=float(rh[p1 + 1]))
    res['ess'] = None
    if keep is None:
        res.update(betas=None, sigsqd=None, tausqd=None, chain=None, attempts=None, noise_var=None)
        return res
    kept = res['kept']
    res.update(betas=raw['betas'].reshape(chains * kept, p1), sigsqd=raw['sigsqd'].reshape(-1), tausqd=raw['tausqd'].reshape(-1),
               attempts=raw['attempts'].reshape(-1), chain=np.repeat(np.arange(chains, dtype=np.int32), kept))
    factor = 1.0 if np.isinf(nu) else (nu / (nu - 2.0) if nu > 2.0 else np.inf)
    res['noise_var'] = res['sigsqd'] * factor
    res['ess'] = dict(betas=_rs._ess_chains(raw['betas'][good]), sigsqd=float(_rs._ess_chains(raw['sigsqd'][good][:, :, None])[0]),
                      tausqd=float(_rs._ess_chains(raw['tausqd'][good][:, :, None])[0]))
    return res


def _starts(p):
    return start_values(p['a'], p['b'], p['atau'], p['btau'], p['chains'], p['seed'], p['init'])


_SIGNATURE = """
    mtx, phis, kernel, inputs, data, a, b, atau, btau : as ``resample.resample`` takes them
    nu          : degrees of freedom of the noise, fixed, >= 1 (default 4); np.inf: Gaussian noise (lam = 1)
    weights     : [n] known relative precisions of the rows, finite and > 0 (default ones)
    chains, draws, burnin, thin, seed, init : as ``resample``'s; every iteration is a pass over all rows, so the defaults
                  are smaller
    keep        : 'betas' -> betas [chains kept, P + 1]; None -> no rows, only the per-chain moments, R-hat and weight_mean

    Returns a ``ResampleResult``.  Rows are chain-major, in iteration order:
      betas [chains kept, P + 1], sigsqd, tausqd, chain, attempts [chains kept]: as ``resample``'s, ready for
                ``evaluate(betas=)``, ``propagate(betas=)``, ``optimize`` and the dynamics' draws
      weight_mean [n]   the mean of lam_i over the post-burn-in passes and the good chains: how much each row was trusted
                (about 1 for a row the model explains, towards 0 for a gross error; ones under nu = inf)
      nu, noise ('student' | 'gaussian'), noise_var = sigsqd nu / (nu - 2) per row of betas (inf for nu <= 2): sigsqd is the
                SCALE of the t noise, not its variance
      rhat, ess   dicts 'betas' [P + 1], 'sigsqd', 'tausqd': split R-hat from the per-chain sums of every post-burn-in
                iteration; ESS (initial positive sequence) of the kept rows, None under keep=None
      chain_mean, chain_var   dicts with the same keys, per chain
      flagged [chains], flagged_at, flag_reason (FLAG_*), attempts_total, attempts_max, sigsqd0, tausqd0, sums, shift
    ``FoKL.score`` and ``FoKL.predictive`` assume a Gaussian likelihood and refuse a result whose ``nu`` is finite, unless
    they are called with ``likelihood='posterior'``, which reads ``nu`` and ``weights`` from the result.
    numpy's global random stream is not consumed and nothing of a model is changed."""


def resample_robust(mtx, phis, kernel, inputs, data, a, b, atau, btau, nu=4.0, weights=None, chains=4, draws=1000, burnin=200,
                    thin=1, seed=0, init='dispersed', keep='betas', device=None):
    """The posterior of a fitted model under Student-t noise and given row weights: ``chains`` Gibbs chains on the device,
    every iteration a weighted pass over all rows.

    device      : device index (default: the process's device, as for ``fit``) or a backend.  The training set replaces
                  the dataset uploaded to that device's context, as ``resample`` does."""
    from . import engine
    p = _prepare(mtx, phis, kernel, inputs, data, a, b, atau, btau, nu, weights, chains, draws, burnin, thin, seed, init, keep)
    backend = _rs._backend_of(device)
    ctx = getattr(backend, 'ctx', backend)
    packed, nb, width = getKernels.pack_phis(p['phis'], p['kid'])
    backend.upload(p['inputs'], p['data'], p['kid'], packed, nb, width)
    slots = [_capi.SLOT_ONES]
    if p['P']:
        pool = engine.SlotPool(backend, initial=max(64, p['P'] + 3))
        term_slots = pool.take(p['P'])
        backend.build_terms(p['mtx'], term_slots)
        slots = slots + term_slots
    G0 = ctx.robust_pass(slots, p['weights'], None, 1.0, np.inf, p['seed'], 0, 0)[0]
    shift = _shift(p, G0)
    sig0, tau0 = _starts(p)
    raw = ctx.robust_chains(slots, p['weights'], p['nu'], p['hyper'], shift, sig0, tau0, p['burnin'], p['draws'], p['thin'],
                            p['seed'], rows=p['keep'] is not None)
    return _assemble(p, raw, sig0, tau0, shift)


def resample_robust_host(mtx, phis, kernel, inputs, data, a, b, atau, btau, nu=4.0, weights=None, chains=4, draws=1000,
                         burnin=200, thin=1, seed=0, init='dispersed', keep='betas'):
    """``resample_robust`` with the columns, the passes and the steps in numpy on this host and the same Philox numbers: the
    statement of the computation (module docstring), for tests and for reading -- a Python loop over the iterations, not a
    fallback.  Same arguments, same result fields."""
    from .embedded import basis_matrix
    p = _prepare(mtx, phis, kernel, inputs, data, a, b, atau, btau, nu, weights, chains, draws, burnin, thin, seed, init, keep)
    X = basis_matrix(p['inputs'], p['mtx'], p['phis'], p['kernel']) if p['P'] else np.ones((p['n'], 1))
    G0 = pass_host(X, p['data'], p['weights'], None, 1.0, np.inf, p['seed'], 0, 0)[0]
    shift = _shift(p, G0)
    sig0, tau0 = _starts(p)
    raw = robust_host(X, p['data'], p['weights'], p['nu'], p['hyper'], shift, sig0, tau0, p['burnin'], p['draws'], p['thin'],
                      p['seed'], rows=p['keep'] is not None)
    return _assemble(p, raw, sig0, tau0, shift)


resample_robust.__doc__ += _SIGNATURE
resample_robust_host.__doc__ += _SIGNATURE

"""
Resample a fitted model's posterior: many independent Gibbs chains of the chosen model, with sigma^2 and tau^2 kept.

``fit`` leaves the ``draws`` rows of ONE chain, the search's own, which continues numpy's legacy stream bit for bit and is
serial for that reason.  Once the search has chosen ``mtx`` the model is conjugate in the eigenbasis of its Gram matrix and
the recursion (include/fokl_hip.h, fokl_gibbs_chain; FR:1519-1548) needs nothing of size N:

    d      = 1 / (lamb + 1 / tausqd)
    w      = d qty + sqrt(sigsqd) sqrt(d) z,  z ~ N(0, I)                     (beta = Q w)
    bstar  = b + (w' diag(lamb) w - 2 w' qty + dtd + w' w / tausqd) / 2
    sigsqd = 1 / Gamma(astar, 1 / bstar)       (NaN where bstar < 0: the chain is flagged, FR:1538-1541)
    tausqd = 1 / Gamma(atau_star, 1 / (w' w / (2 sigsqd) + btau))

with astar = a + 1 + n / 2 + (P + 1) / 2 and atau_star = atau + P / 2 (FR:1508-1510).  ``resample`` runs ``chains`` of them
side by side on the device, one wavefront each (``fokl_resample_chains``, csrc/fokl_resample_device.inc), every chain drawing
its own counter-based numbers: Philox 4x32-10 keyed by (seed, chain) with the counter (iteration, purpose, index), purposes
``_capi.RES_*``: the normal of eigen-coordinate ``index``; the normal and the uniform of attempt ``index`` of each of the two
gamma variates (Marsaglia-Tsang for shapes >= 1: v = (1 + c x)^3, accepted when u < 1 - 0.0331 x^4 or
ln u < x^2 / 2 + b (1 - v + ln v), b = shape - 1/3, c = 1 / sqrt(9 b)); the two uniforms of a dispersed start.  Nothing
depends on a stream position: chain c of a 64-chain run is chain c run alone, a ``thin=3`` run's rows are every third row of
the ``thin=1`` run, and numpy's global stream is never touched.

The pipeline of one call: the model's columns (K1) and one Gram of [1 | X | y] (K2) on the device as ``fit(update=True)``
forms them, ``eigh_canonical`` on the host, the chains on the device, ``betas = W Q'`` in numpy (the rows come back to the
host, where every consumer takes them from), diagnostics on the host from the per-chain sums the kernel leaves.
Without the library or a gfx950 device ``resample`` raises; there is no host fallback.  ``resample_host`` is the same function
in numpy with the same Philox numbers and the kernel's summation order: the STATEMENT the kernel is tested against.
"""
import numpy as np

from . import _capi
from . import getKernels
from .embedded import basis_matrix, _kernel_id

MAX_COLUMNS = _capi.RESAMPLE_MAX_COLUMNS
ATTEMPT_CAP = _capi.RESAMPLE_ATTEMPT_CAP
FLAG_NONE, FLAG_BSTAR_NEGATIVE, FLAG_ATTEMPT_CAP = 0, 1, 2
_KEEP = ('betas', 'w', None)
_INIT = ('reference', 'dispersed')


class ResampleResult(dict):
    """A dict whose entries are also attributes (``res.betas``, ``res['betas']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


# ---------------------------------------------------------------------------------------------------------
# the statement of fokl_resample_chains
# ---------------------------------------------------------------------------------------------------------

def gamma_constants(shape):
    """Marsaglia-Tsang's (b, c) of a shape >= 1, rounded as the native entry rounds them."""
    b = float(shape) - 1.0 / 3.0
    return b, 1.0 / np.sqrt(9.0 * b)


def standard_gamma(seed, chain, iteration, shape, which='sigsqd', attempt_cap=ATTEMPT_CAP):
    """One standard gamma variate of ``shape`` >= 1 as chain ``chain`` draws it at ``iteration`` for sigma^2 (``which`` =
    'sigsqd') or tau^2 ('tausqd') -> (value, attempts); NaN when ``attempt_cap`` attempts were rejected."""
    pn, pu = ((_capi.RES_SIG_NORMAL, _capi.RES_SIG_UNIFORM) if which == 'sigsqd'
              else (_capi.RES_TAU_NORMAL, _capi.RES_TAU_UNIFORM))
    b, c = gamma_constants(shape)
    cap = int(attempt_cap) or ATTEMPT_CAP
    x = u = None
    for a in range(cap):
        if a % 4 == 0:                                                   # attempts are indices of the counter: fetch a few
            count = min(cap, a + 4)
            x = _capi.embedded_rng(seed, chain, iteration, pn, count)
            u = _capi.embedded_rng(seed, chain, iteration, pu, count)
        v1 = 1.0 + c * x[a]
        if v1 <= 0.0:
            continue
        v, x2 = (v1 * v1) * v1, x[a] * x[a]
        with np.errstate(divide='ignore'):
            if u[a] < 1.0 - 0.0331 * (x2 * x2) or np.log(u[a]) < 0.5 * x2 + b * ((1.0 - v) + np.log(v)):
                return b * v, a + 1
    return np.nan, cap


def wave_sum(x):
    """The kernel's sum over the eigen-coordinates of x [chains, P + 1]: lane l adds its elements l, l + 64, ... in ascending
    order, then the 64 lanes are combined by a fixed tree (inside rows of 16: +8, +4, +2, +1; then (r0 + r1) + (r2 + r3))."""
    chains, p1 = x.shape
    T = -(-p1 // 64)
    padded = np.zeros((chains, T * 64))
    padded[:, :p1] = x
    padded = padded.reshape(chains, T, 64)
    lanes = np.zeros((chains, 64))
    for t in range(T):
        lanes = lanes + padded[:, t]
    r = lanes.reshape(chains, 4, 16)
    r = r[:, :, :8] + r[:, :, 8:]
    r = r[:, :, :4] + r[:, :, 4:]
    r = r[:, :, :2] + r[:, :, 2:]
    r = r[:, :, 0] + r[:, :, 1]
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def chains_host(lamb, qty, shift, astar, atau_star, b, btau, dtd, sigsqd0, tausqd0, burnin, draws, thin, seed, rows=True,
                attempt_cap=0, chain_ids=None, normals=None, gammas=None):
    """The statement of ``DeviceContext.resample_chains`` (fokl_resample_chains), same arguments and the same dict:

      w [chains, kept, P + 1], sigsqd, tausqd [chains, kept]   the kept iterations' draws (None without ``rows``)
      attempts [chains, kept]                                 Marsaglia-Tsang attempts of the row's two gamma variates
      sums [chains, 3, 2, P + 3]                              over the first half, the second half and the odd last of the
                                                              post-burn-in iterations: sum and sum of squares of
                                                              w - shift | sigsqd | tausqd, accumulated in iteration order
      counts [chains, 4]                                      first flagged iteration or -1, why (FLAG_*), attempts in all,
                                                              the most one variate took

    ``chain_ids``: the chain numbers that key the generator (default 0 .. chains - 1).  ``normals`` [iterations, P + 1] and
    ``gammas`` = (g_sigsqd [iterations], g_tausqd [iterations]) replace the generator for a single chain: the recursion fed
    somebody else's numbers."""
    lamb, qty, shift = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (lamb, qty, shift))
    sig = np.array(np.reshape(sigsqd0, -1), dtype=np.float64)
    tau = np.array(np.reshape(tausqd0, -1), dtype=np.float64)
    chains, p1 = sig.shape[0], lamb.shape[0]
    ids = np.arange(chains) if chain_ids is None else np.asarray(chain_ids).reshape(-1)
    burnin, draws, thin = int(burnin), int(draws), int(thin)
    kept, half, total = -(-draws // thin), draws // 2, burnin + draws
    fed = normals is not None
    if fed and (chains != 1 or gammas is None):
        raise ValueError("normals and gammas are given together, for one chain")
    w_out = np.empty((chains, kept, p1)) if rows else None
    sig_out = np.empty((chains, kept)) if rows else None
    tau_out = np.empty((chains, kept)) if rows else None
    att_out = np.zeros((chains, kept), dtype=np.int32) if rows else None
    sums = np.zeros((chains, _capi.RESAMPLE_SEGMENTS, 2, p1 + 2))
    counts = np.zeros((chains, 4), dtype=np.int64)
    counts[:, 0] = -1
    run = np.zeros((chains, 2, p1 + 2))

    def flush(segment):
        sums[:, segment] = run
        run[:] = 0.0

    z, gs, gt = np.empty((chains, p1)), np.empty(chains), np.empty(chains)
    att = np.zeros((chains, 2), dtype=np.int64)
    with np.errstate(all='ignore'):
        for k in range(total):
            if fed:
                z[0], gs[0], gt[0] = normals[k], gammas[0][k], gammas[1][k]
            else:
                for c in range(chains):
                    gs[c], att[c, 0] = standard_gamma(seed, ids[c], k, astar, 'sigsqd', attempt_cap)
                    gt[c], att[c, 1] = standard_gamma(seed, ids[c], k, atau_star, 'tausqd', attempt_cap)
                    z[c] = _capi.embedded_rng(seed, ids[c], k, _capi.RES_BETA, p1)
            inv_tau, root_sig = 1.0 / tau, np.sqrt(sig)
            d = 1.0 / (lamb[None, :] + inv_tau[:, None])
            w = d * qty + root_sig[:, None] * (np.sqrt(d) * z)
            ww = w * w
            q_lam, q_ty, q_ww = wave_sum(lamb * ww), wave_sum(w * qty), wave_sum(ww)
            bstar = b + 0.5 * (((q_lam - 2.0 * q_ty) + dtd) + q_ww / tau)
            negative = bstar < 0.0
            sig = np.where(negative, np.nan, 1.0 / ((1.0 / bstar) * gs))
            btau_star = (1.0 / (2.0 * sig)) * q_ww + btau
            tau = 1.0 / ((1.0 / btau_star) * gt)
            capped = np.isnan(gs) | np.isnan(gt)
            first = (negative | capped) & (counts[:, 0] < 0)
            counts[first, 0] = k
            counts[first, 1] = np.where(negative[first], FLAG_BSTAR_NEGATIVE, FLAG_ATTEMPT_CAP)
            counts[:, 2] += att.sum(axis=1)
            counts[:, 3] = np.maximum(counts[:, 3], att.max(axis=1))
            j = k - burnin
            if j < 0:
                continue
            if rows and j % thin == 0:
                r = j // thin
                w_out[:, r], sig_out[:, r], tau_out[:, r], att_out[:, r] = w, sig, tau, att.sum(axis=1)
            dev = w - shift
            run[:, 0, :p1] += dev
            run[:, 1, :p1] += dev * dev
            run[:, 0, p1] += sig
            run[:, 1, p1] += sig * sig
            run[:, 0, p1 + 1] += tau
            run[:, 1, p1 + 1] += tau * tau
            if j + 1 == half:
                flush(0)
            elif j + 1 == 2 * half:
                flush(1)
        if draws & 1:
            flush(2)
    return dict(w=w_out, sigsqd=sig_out, tausqd=tau_out, attempts=att_out, sums=sums, counts=counts)


# ---------------------------------------------------------------------------------------------------------
# diagnostics
# ---------------------------------------------------------------------------------------------------------

def split_rhat_from_sums(sums, draws):
    """Split R-hat (``embedded.split_rhat``'s definition) of every column of the kernel's per-chain sums
    [chains, 3, 2, K]: the two halves of every chain are the 2 x chains sequences of draws // 2 iterations."""
    sums = np.asarray(sums, dtype=np.float64)
    half = int(draws) // 2
    if half < 2 or sums.shape[0] < 1:
        return np.full(sums.shape[-1], np.nan)
    s = np.concatenate([sums[:, 0, 0], sums[:, 1, 0]], axis=0)           # [2 chains, K]
    q = np.concatenate([sums[:, 0, 1], sums[:, 1, 1]], axis=0)
    with np.errstate(all='ignore'):
        means = s / half
        variances = np.maximum(q - s * s / half, 0.0) / (half - 1)
        within = variances.mean(axis=0)
        between = half * means.var(axis=0, ddof=1)
        return np.sqrt(((half - 1) / half * within + between / half) / within)


def ess_ips(x):
    """Effective sample size of every column of one chain x [n, D] by Geyer's initial positive sequence estimator:
    n / (-1 + 2 sum_k (rho_2k + rho_2k+1)) over the leading pairs whose sum is positive."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, D = x.shape
    if n < 4:
        return np.full(D, float(n))
    xc = x - x.mean(axis=0)
    size = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(xc, n=size, axis=0)
    acov = np.fft.irfft(f * np.conj(f), n=size, axis=0)[:n] / n
    out = np.empty(D)
    for j in range(D):
        if not acov[0, j] > 0.0:
            out[j] = float(n) if acov[0, j] == 0.0 else np.nan
            continue
        rho = acov[:, j] / acov[0, j]
        pairs = rho[0:2 * (n // 2):2] + rho[1:2 * (n // 2):2]
        stop = np.flatnonzero(pairs <= 0.0)
        m = stop[0] if stop.size else pairs.shape[0]
        tau = -1.0 + 2.0 * pairs[:m].sum()
        out[j] = n / max(tau, 1.0 / np.log10(max(n, 10)))
    return out


def _ess_chains(x):
    """ess_ips summed over the chains of x [chains, n, D]."""
    return np.sum([ess_ips(c) for c in x], axis=0) if x.shape[0] else np.full(x.shape[2], np.nan)


# ---------------------------------------------------------------------------------------------------------
# one call
# ---------------------------------------------------------------------------------------------------------

def _prepare(mtx, phis, kernel, inputs, data, a, b, atau, btau, chains, draws, burnin, thin, seed, init, keep):
    """Every check of ``resample`` / ``resample_host`` (ValueError).  Touches no device."""
    kid = _kernel_id(kernel)
    if mtx is None or inputs is None or data is None:
        raise ValueError("resample needs a fitted model: its interaction matrix mtx and the cleaned training inputs / data")
    for name, value in (('a', a), ('b', b), ('atau', atau), ('btau', btau)):
        if value is None or not np.isfinite(float(value)):
            raise ValueError(f"resample needs a fitted model: the hyper-parameter {name} is not set (fit derives b and btau "
                             f"from the data)")
    inputs = np.asarray(inputs, dtype=np.float64)
    if inputs.ndim == 1:
        inputs = inputs[:, np.newaxis]
    if inputs.ndim != 2 or inputs.shape[0] < 1:
        raise ValueError("inputs must be [n, M] with at least one row")
    n, M = inputs.shape
    data = np.asarray(data, dtype=np.float64).reshape(-1)
    if data.shape[0] != n or not np.isfinite(data).all() or not np.isfinite(inputs).all():
        raise ValueError(f"data must hold one finite value per row of inputs ({n}), and the inputs must be finite")
    mtx = np.asarray(mtx)
    mtx = mtx.reshape(0, M) if mtx.size == 0 else np.atleast_2d(mtx)
    if mtx.ndim != 2 or mtx.shape[1] != M:
        raise ValueError(f"inputs have {M} columns, the interaction matrix has {mtx.shape[-1]}")
    if np.any(mtx < 0) or np.any(mtx > len(phis)):
        raise ValueError(f"the interaction matrix holds orders outside the table of {len(phis)} basis functions")
    P = mtx.shape[0]
    if P + 1 > MAX_COLUMNS:
        raise ValueError(f"the model has {P + 1} columns, the resampling kernel is instantiated for at most {MAX_COLUMNS} "
                         f"(12 eigen-coordinates per lane, the device chain engine's bar; not a register budget)")
    if float(atau) + P / 2 < 1:
        raise ValueError(f"atau + P / 2 = {float(atau) + P / 2} < 1: the gamma sampler is Marsaglia-Tsang's for shapes >= 1")
    for name, value, low in (('chains', chains, 1), ('draws', draws, 1), ('burnin', burnin, 0), ('thin', thin, 1)):
        if int(value) != value or int(value) < low:
            raise ValueError(f"{name} must be an integer >= {low}")
    if int(chains) > (1 << 20) or int(burnin) + int(draws) > (1 << 30):
        raise ValueError("at most 1 048 576 chains and 2^30 iterations per chain")
    if int(seed) != seed:
        raise ValueError("seed must be an integer")
    if init not in _INIT:
        raise ValueError(f"init must be one of {_INIT}")
    if keep not in _KEEP:
        raise ValueError(f"keep must be one of {_KEEP}")
    return dict(kid=kid, mtx=mtx.astype(np.int32), phis=phis, kernel=kernel, inputs=np.ascontiguousarray(inputs), data=data,
                n=n, P=P, a=float(a), b=float(b), atau=float(atau), btau=float(btau), chains=int(chains), draws=int(draws),
                burnin=int(burnin), thin=int(thin), seed=int(seed) & 0xFFFFFFFF, init=init, keep=keep)


def start_values(a, b, atau, btau, chains, seed, init):
    """Where the chains start -> (sigsqd0 [chains], tausqd0 [chains]).  'reference': b / (1 + a) and btau / (1 + atau)
    (FR:1371-1372) for every chain.  'dispersed': chain c multiplies the two by 10^(2 u - 1), u its two uniforms of purpose
    RES_START at iteration 0: factors spread log-uniformly over [0.1, 10]."""
    sig0 = np.full(chains, b / (1.0 + a))
    tau0 = np.full(chains, btau / (1.0 + atau))
    if init == 'dispersed':
        u = np.array([_capi.embedded_rng(seed, c, 0, _capi.RES_START, 2) for c in range(chains)])
        sig0, tau0 = sig0 * 10.0 ** (2.0 * u[:, 0] - 1.0), tau0 * 10.0 ** (2.0 * u[:, 1] - 1.0)
    return sig0, tau0


def spectrum(gram, n, a, atau):
    """From the Gram of [1 | X | y]: everything the recursion needs -> dict(lamb, Q, qty, dtd, astar, atau_star)."""
    from .engine import eigh_canonical
    gram = np.asarray(gram, dtype=np.float64)
    p1 = gram.shape[0] - 1
    lamb, Q = eigh_canonical(gram[:p1, :p1])
    return dict(lamb=lamb, Q=Q, qty=Q.T @ gram[:p1, p1], dtd=float(gram[p1, p1]), astar=a + 1 + n / 2 + p1 / 2,
                atau_star=atau + (p1 - 1) / 2)                          # FR:1508-1510


def _assemble(p, spec, raw, sig0, tau0, shift):
    chains, draws, keep = p['chains'], p['draws'], p['keep']
    p1 = p['P'] + 1
    counts, sums = raw['counts'], raw['sums']
    good = counts[:, 0] < 0
    res = ResampleResult(chains=chains, draws=draws, burnin=p['burnin'], thin=p['thin'], seed=p['seed'], keep=keep,
                         kept=-(-draws // p['thin']), sigsqd0=sig0, tausqd0=tau0, flagged=~good, flagged_at=counts[:, 0].copy(),
                         flag_reason=counts[:, 1].copy(), attempts_total=int(counts[:, 2].sum()),
                         attempts_max=int(counts[:, 3].max()), sums=sums, shift=shift, lamb=spec['lamb'], Q=spec['Q'],
                         astar=spec['astar'], atau_star=spec['atau_star'])
    # per-chain moments over all post-burn-in iterations (the three segments in their order)
    with np.errstate(all='ignore'):
        s = (sums[:, 0, 0] + sums[:, 1, 0]) + sums[:, 2, 0]
        q = (sums[:, 0, 1] + sums[:, 1, 1]) + sums[:, 2, 1]
        mean = s / draws
        var = np.maximum(q / draws - mean * mean, 0.0) * (draws / (draws - 1) if draws > 1 else np.nan)
    mean[:, :p1] += shift
    res['chain_mean'] = dict(w=mean[:, :p1], sigsqd=mean[:, p1], tausqd=mean[:, p1 + 1])
    res['chain_var'] = dict(w=var[:, :p1], sigsqd=var[:, p1], tausqd=var[:, p1 + 1])
    rh = split_rhat_from_sums(sums[good], draws)
    res['rhat'] = dict(w=rh[:p1], sigsqd=float(rh[p1]), tausqd=float(rh[p1 + 1]))
    res['ess'] = None
    if keep is None:
        res.update(betas=None, w=None, sigsqd=None, tausqd=None, chain=None, attempts=None)
        return res
    kept = res['kept']
    W = raw['w'].reshape(chains * kept, p1)
    res.update(sigsqd=raw['sigsqd'].reshape(-1), tausqd=raw['tausqd'].reshape(-1), attempts=raw['attempts'].reshape(-1),
               chain=np.repeat(np.arange(chains, dtype=np.int32), kept))
    rows = W @ spec['Q'].T                                               # betas = W Q'
    if keep == 'betas':
        res.update(betas=rows, w=None)
    else:
        res.update(betas=None, w=W)
    from .embedded import split_rhat
    by_chain = rows.reshape(chains, kept, p1)[good]
    res['rhat']['betas'] = split_rhat(by_chain) if by_chain.shape[0] else np.full(p1, np.nan)
    res['ess'] = dict(w=_ess_chains(raw['w'][good]), betas=_ess_chains(by_chain),
                      sigsqd=float(_ess_chains(raw['sigsqd'][good][:, :, None])[0]),
                      tausqd=float(_ess_chains(raw['tausqd'][good][:, :, None])[0]))
    return res


def _run(p, gram, run_chains):
    spec = spectrum(gram, p['n'], p['a'], p['atau'])
    sig0, tau0 = start_values(p['a'], p['b'], p['atau'], p['btau'], p['chains'], p['seed'], p['init'])
    # the sums are accumulated about a value close to every coordinate's posterior mean, so that their variances are not
    # differences of two large numbers: the conditional mean at the reference start
    shift = spec['qty'] / (spec['lamb'] + (1.0 + p['atau']) / p['btau'])
    raw = run_chains(spec['lamb'], spec['qty'], shift, spec['astar'], spec['atau_star'], p['b'], p['btau'], spec['dtd'], sig0,
                     tau0, p['burnin'], p['draws'], p['thin'], p['seed'], rows=p['keep'] is not None)
    return _assemble(p, spec, raw, sig0, tau0, shift)


def _backend_of(device):
    if hasattr(device, 'build_terms') and hasattr(device, 'gram') and hasattr(device, 'upload'):
        return device
    from . import FoKLRoutines
    return FoKLRoutines.device_backend(device)


def _device_gram(p, backend):
    """Upload, K1 on ``mtx``, one Gram of [1 | X | y] (K2): as ``update.fit_update_first`` forms it."""
    from . import engine
    packed, nb, width = getKernels.pack_phis(p['phis'], p['kid'])
    backend.upload(p['inputs'], p['data'], p['kid'], packed, nb, width)
    slots = [_capi.SLOT_ONES]
    if p['P']:
        pool = engine.SlotPool(backend, initial=max(64, p['P'] + 3))
        term_slots = pool.take(p['P'])
        backend.build_terms(p['mtx'], term_slots)
        slots = slots + term_slots
    slots = slots + [_capi.SLOT_Y]
    return np.array(backend.gram(slots, slots), dtype=np.float64)


def _host_gram(p):
    X = basis_matrix(p['inputs'], p['mtx'], p['phis'], p['kernel']) if p['P'] else np.ones((p['n'], 1))
    Xy = np.concatenate([X, p['data'][:, None]], axis=1)
    return Xy.T @ Xy


_SIGNATURE = """
    mtx, phis, kernel : the fitted model's (``FoKL.resample`` passes its own)
    inputs, data : the cleaned training set the model was fitted to, [n, M] and [n]
    a, b, atau, btau : the hyper-parameters the fit used (``fit`` leaves the data-driven b and btau on the model)
    chains      : independent chains, one wavefront each
    draws       : post-burn-in iterations per chain; ``burnin`` iterations before them are discarded
    thin        : every ``thin``-th post-burn-in iteration is a row: kept = ceil(draws / thin) rows per chain
    seed        : the generator's key is (seed, chain): the same seed gives the same bits, on any launch shape
    init        : 'reference' starts every chain at b / (1 + a), btau / (1 + atau) (FR:1371-1372); 'dispersed' multiplies each
                  chain's two starting values by factors spread log-uniformly over [0.1, 10], so that R-hat means something
    keep        : 'betas' -> betas [chains kept, P + 1], ready for ``evaluate(betas=...)``, ``propagate(betas=...)``,
                  ``optimize(betas=...)``, ``GP_Integrate_ensemble``; 'w' -> the eigenbasis rows w (betas = w Q'); None -> no rows
                  at all, only the per-chain moments and R-hat (so R-hat over 1e7 iterations costs no memory)

    Returns a ``ResampleResult`` (a dict with attribute access).  Rows are chain-major, in iteration order:
      betas | w [chains kept, P + 1], sigsqd, tausqd [chains kept] (the values the row's iteration drew), chain [chains kept]
      int32, attempts [chains kept] (Marsaglia-Tsang attempts of the row's two gamma variates); Q, lamb (the eigenbasis)
      rhat      dict: 'w' [P + 1], 'sigsqd', 'tausqd' -- split R-hat from the per-chain sums of every post-burn-in iteration,
                whatever is kept -- and 'betas' [P + 1] from the kept rows
      ess       dict with the same keys by the initial-positive-sequence estimator on the kept rows, summed over the
                chains; None under keep=None
      chain_mean, chain_var   dicts 'w' [chains, P + 1], 'sigsqd', 'tausqd' [chains]: per-chain moments of every iteration
      flagged [chains] bool, flagged_at (iteration or -1), flag_reason (FLAG_*): a chain that met bstar < 0 is NaN from that
                iteration on, as FR:1538-1541 leaves it, and is left out of rhat / ess
      attempts_total, attempts_max, sigsqd0, tausqd0 [chains], sums (the kernel's [chains, 3, 2, P + 3]), shift, astar, atau_star
    numpy's global random stream is not consumed and nothing of a model is changed."""


def resample(mtx, phis, kernel, inputs, data, a, b, atau, btau, chains=64, draws=10000, burnin=500, thin=1, seed=0,
             init='dispersed', keep='betas', device=None):
    """Resample the posterior of a fitted model: ``chains`` independent Gibbs chains on the device, sigma^2 and tau^2 kept.

    device      : device index (default: the process's device, as for ``fit``) or a backend.  The training set replaces
                  the dataset uploaded to that device's context, as ``evaluate`` and ``propagate`` do."""
    p = _prepare(mtx, phis, kernel, inputs, data, a, b, atau, btau, chains, draws, burnin, thin, seed, init, keep)
    backend = _backend_of(device)
    ctx = getattr(backend, 'ctx', backend)
    return _run(p, _device_gram(p, backend), ctx.resample_chains)


def resample_host(mtx, phis, kernel, inputs, data, a, b, atau, btau, chains=64, draws=10000, burnin=500, thin=1, seed=0,
                  init='dispersed', keep='betas'):
    """``resample`` with the columns, the Gram and the chains in numpy on this host, the same Philox numbers and the kernel's
    summation order: the statement of the computation (module docstring), for tests and for reading -- a Python loop over the
    iterations, not a fallback.  Same arguments, same result fields."""
    p = _prepare(mtx, phis, kernel, inputs, data, a, b, atau, btau, chains, draws, burnin, thin, seed, init, keep)
    return _run(p, _host_gram(p), chains_host)


resample.__doc__ += _SIGNATURE
resample_host.__doc__ += _SIGNATURE

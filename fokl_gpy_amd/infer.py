"""
Infer unknown inputs from observed outputs: "I measured these outputs; which inputs produced them, and how sure can I be?"
One affine-invariant ensemble sampler (Goodman & Weare 2010) of 64 walkers over the unknown inputs per posterior draw of
the model, all ensembles at once on the device.  One ensemble per draw marginalises the model's own uncertainty; pooled,
the walkers are draws of p(unknown inputs | observations).

The problem, in normalised coordinates.  A fitted 'Bernoulli Polynomials' model with m inputs, d of them unknown (1 <= d <=
16, shared by all observations) and m - d known per observation; K observations y_k.  For posterior draw e with
h_e = 0.5 / sigsqd_e:

    f_ek(theta) = sum_t (beta_e[t] * P[k, t]) * U_t(theta)          t = 0 .. T ascending; t = 0 the intercept (P = U = 1)
    lp_e(theta) = -h_e * sum_k (y_k - f_ek(theta))**2 - 0.5 * sum_i prec_i * (theta_i - mean_i)**2
                                                                      k ascending, then i ascending; each sum starts at 0

U_t is the product of term t's factors in the unknown inputs, in ascending input order from the left, each factor by
Horner from the coefficient table (``getKernels.pack_phis``), once per point and distinct (input, order).  P[k, t] is the
product of term t's factors in the known inputs at observation k: ``_prepare`` forms it once from the host basis
evaluation, it does not depend on the draw, and the sampler never sees a known input.  Outside the box lo < theta < hi
(default the training range; ``bounds`` narrows it) lp = -inf.  prec_i = 0: no prior beyond the box.

The sampler.  W = 64 walkers per draw.  Starts: ``optimize.start_points(64, lo, hi)``, the same for every draw, or user
starts [64, d] strictly inside the box.  Iteration t = 0, 1, ... (burn-in included) updates half 0 (walkers 0..31), then
half 1 (walkers 32..63); a moving walker w of half hf reads the OTHER half as it stands at that moment (half 1 sees half 0
already moved).  With the uniforms u1, u2, u3 of walker w at iteration t:

  stretch move (Goodman-Weare, a = 2)     j = 32 (1 - hf) + floor(32 u1);  z = (1 + u2)**2 / 2;  y = x_j + z (x_w - x_j);
                                          log_ratio = (d - 1) log z + lp(y) - lp(x_w)
  jump move (differential evolution, gamma = 1; lets walkers change modes), when jump_every > 0 and t % jump_every ==
  jump_every - 1                          a = floor(32 u1), b = (a + 1 + floor(31 u2)) mod 32, both in the other half;
                                          y_i = x_w,i + (x_a,i - x_b,i) + 1e-5 (hi_i - lo_i) n_i;  log_ratio = lp(y) - lp(x_w)
  acceptance                              a proposal outside the box is rejected without an evaluation; otherwise it is
                                          accepted iff log(u3) < log_ratio

Random numbers: Philox 4x32-10 (``csrc/fokl_philox.h``), key (seed, draw id), counter (t, purpose, index, 1); purposes 0, 1,
2 are u1, u2, u3 with index = walker, 3 the jitter normal n_i (Box-Muller) with index 64 i + w; the host reads them through
``_capi.infer_rng``.  The draw id is the draw's row in ``betas``.  Counter-based numbers make ensemble e of an E-draw run
the ensemble run alone, a thin = 3 run's rows every third row of the thin = 1 run, and the result independent of how the
draws are sliced over launches -- bit for bit.

Kept: row r is the state after both halves of iteration burnin + r thin, r < ceil(draws / thin); per walker and half of the
post-burn-in iterations (the first draws // 2, then the rest) the sum and the sum of squares of theta_i - (lo_i + hi_i) / 2
in iteration order; per walker the accepted stretch and jump moves; per draw the target evaluations.

``infer_inputs`` runs the ensembles on the device (``fokl_infer_inputs``, csrc/fokl_infer_device.inc: one wavefront per
draw, lane = walker; without the library or a gfx950 device it raises, there is no host fallback).  ``infer_inputs_host``
is the same function in numpy with no device (``sample_host``): the STATEMENT the kernel is tested against.  They share
``_prepare`` (every check, P; touches no device) and the assembly.  The device's log and cosine may differ from numpy's in
the last bit, which can flip an acceptance: compare flags, and states where the flags agree.

Limits, checked before anything is launched and again by the native entry point: 1 to 16 unknowns; 3 x distinct (unknown
input, order) factors + 4 d values per walker within the 144 KB of LDS a wavefront gets (288); orders within the table; the
kept rows within the device's free memory.  The draws are sliced over launches of at most 2**33 term evaluations by a
wavefront (``_capi.INFER_TERM_CAP``).
"""
import numpy as np

from . import _capi
from . import getKernels
from . import optimize as _optimize
from .GP_Integrate import bounds_cut, _device_context
from .embedded import basis_matrix

WALKERS = _capi.INFER_WALKERS
HALF = WALKERS // 2
MAX_UNKNOWN = _optimize.MAX_INPUTS
LDS_ROWS = _optimize.LDS_ROWS
JITTER = 1e-5


class InferResult(dict):
    """A dict whose entries are also attributes (``res.x``, ``res['x']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def _index_of(name, names, what):
    if isinstance(name, (int, np.integer)) and not isinstance(name, bool):
        if not 0 <= int(name) < len(names):
            raise ValueError(f"{what}: input index {name} outside 0..{len(names) - 1}")
        return int(name)
    if str(name) not in names:
        raise ValueError(f"{what}: '{name}' is not an input of the model ({list(names)})")
    return names.index(str(name))


def _prepare(betas, sigsqd, mtx, phis, minmax, kernel, unknown, known, data, clean=False, prior=None, bounds=None, noise=None,
             starts=None, burnin=300, draws=200, thin=10, jump_every=8, seed=0, keep='x', objective='draws', posterior=None,
             xvars=None):
    """Every check of ``infer_inputs`` / ``infer_inputs_host`` (ValueError) and every array both need, in normalised
    coordinates, P among them.  Touches no device."""
    if kernel in (0, 'Cubic Splines'):
        raise ValueError("infer_inputs handles the 'Bernoulli Polynomials' kernel only: a 'Cubic Splines' model is piecewise "
                         "and is not inverted")
    if kernel not in (1, 'Bernoulli Polynomials') or (len(phis) > 0 and np.ndim(phis[0][0]) != 0):
        raise ValueError("infer_inputs needs the 'Bernoulli Polynomials' kernel and its coefficient table in phis")
    if objective not in ('draws', 'mean'):
        raise ValueError("objective must be 'draws' (one ensemble per posterior draw) or 'mean' (one, on the mean betas)")
    if keep not in ('x', None):
        raise ValueError("keep must be 'x' (the kept rows) or None (sums, acceptance and R-hat only)")
    mtx = np.asarray(mtx)
    if mtx.ndim == 1:
        mtx = mtx[np.newaxis, :]
    if mtx.ndim != 2 or mtx.shape[1] == 0:
        raise ValueError("mtx must be [terms, inputs]")
    mtx = np.ascontiguousarray(mtx, dtype=np.int32)
    T, m = mtx.shape
    if mtx.min(initial=0) < 0 or mtx.max(initial=0) > len(phis):
        raise ValueError("mtx holds an order outside the coefficient table")
    if betas is None:
        raise ValueError("infer_inputs needs betas [draws, terms + 1]")
    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim == 1:
        betas = betas[np.newaxis, :]
    if betas.ndim != 2 or betas.shape[0] == 0 or betas.shape[1] != T + 1:
        raise ValueError(f"betas must be [draws, {T + 1}] (terms + 1)")
    if noise is not None:
        if not (np.ndim(noise) == 0 and float(noise) > 0 and np.isfinite(float(noise))):
            raise ValueError("noise must be a positive number: the standard deviation of the measurement")
        sigsqd = np.full(betas.shape[0], float(noise) * float(noise))
    if sigsqd is None:
        raise ValueError("infer_inputs needs sigma^2 for every draw and a fit keeps the betas only: draw both with "
                         "post = model.resample(...) and pass post, or give the measurement's own noise= (a standard deviation)")
    sigsqd = np.asarray(sigsqd, dtype=np.float64).reshape(-1)
    if sigsqd.shape[0] != betas.shape[0]:
        raise ValueError(f"sigsqd holds {sigsqd.shape[0]} values, betas has {betas.shape[0]} rows: one sigma^2 per draw is needed")
    index = np.arange(betas.shape[0])
    if posterior is not None:
        if np.ndim(posterior) == 0:
            if int(posterior) != posterior or not 1 <= int(posterior) <= betas.shape[0]:
                raise ValueError(f"posterior must be None (all), an integer in 1..{betas.shape[0]} (the last rows of betas) or "
                                 f"an index array")
            index = index[betas.shape[0] - int(posterior):]
        else:
            pick = np.asarray(posterior)
            if pick.ndim != 1 or pick.shape[0] < 1 or not np.issubdtype(pick.dtype, np.integer) or \
                    pick.min() < -betas.shape[0] or pick.max() >= betas.shape[0]:
                raise ValueError(f"posterior as an array must hold at least one integer index into the {betas.shape[0]} rows "
                                 f"of betas")
            index = index[pick]
    betas, sigsqd = betas[index], sigsqd[index]
    if not (np.isfinite(betas).all() and np.isfinite(sigsqd).all()):
        raise ValueError("betas and sigsqd must be finite (drop the rows of a resample's flagged chains with posterior=)")
    if not np.all(sigsqd > 0):
        raise ValueError("every sigsqd must be positive")
    if objective == 'mean':
        betas, sigsqd, index = betas.mean(axis=0, keepdims=True), sigsqd.mean(keepdims=True), np.zeros(1, dtype=np.int64)

    # ---- which inputs are unknown ----
    names = [str(v) for v in xvars] if xvars is not None else [f"x{j + 1}" for j in range(m)]
    if len(names) != m or len(set(names)) != m:
        raise ValueError(f"xvars must name the model's {m} inputs, each once")
    if unknown is None or np.ndim(unknown) == 0:
        unknown = [unknown]
    cols = [_index_of(u, names, 'unknown') for u in unknown if u is not None]
    d = len(cols)
    if d < 1 or d > MAX_UNKNOWN or len(set(cols)) != d:
        raise ValueError(f"unknown must list 1 to {MAX_UNKNOWN} different inputs, by name or index")
    rest = [j for j in range(m) if j not in cols]
    if len(minmax) != m:
        raise ValueError(f"minmax describes {len(minmax)} inputs, mtx {m}")
    low = np.array([float(minmax[j][0]) for j in range(m)])
    span = np.array([float(minmax[j][1]) for j in range(m)]) - low
    if not np.all(span > 0):
        raise ValueError("minmax must have max > min for every input")
    low_u, span_u = low[cols], span[cols]

    # ---- the observations: y, the known inputs, P ----
    if data is None:
        raise ValueError("data [K] is needed: the observed outputs")
    y = np.asarray(data, dtype=np.float64).reshape(-1)
    K = y.shape[0]
    if K < 1 or not np.isfinite(y).all():
        raise ValueError("data must hold at least one observation, all finite")
    full = np.zeros((K, m))
    if rest:
        if known is None:
            raise ValueError(f"known [K, {len(rest)}] is needed: the inputs {[names[j] for j in rest]} at every observation")
        kn = np.asarray(known, dtype=np.float64)
        if kn.ndim == 1:
            kn = kn[:, np.newaxis] if len(rest) == 1 else kn[np.newaxis, :]
        if kn.shape != (K, len(rest)) or not np.isfinite(kn).all():
            raise ValueError(f"known must be finite numbers [{K}, {len(rest)}]: one row per observation, the columns "
                             f"{[names[j] for j in rest]}")
        if clean in (True, 'True', 'true', 1):
            kn = (kn - low[rest]) / span[rest]
        if kn.min() < -1e-12 or kn.max() > 1 + 1e-12:
            raise ValueError("known inputs reach outside the training range: the model is not extrapolated "
                             "(clean=True normalises true-scale values)")
        full[:, rest] = np.clip(kn, 0.0, 1.0)
    elif known is not None and np.size(known) > 0:
        raise ValueError("every input is unknown: known must be None")
    mtx_known = mtx.copy()
    mtx_known[:, cols] = 0
    P = basis_matrix(full, mtx_known, phis, kernel) if T else np.ones((K, 1))
    mtx_u = np.ascontiguousarray(mtx[:, cols])

    # ---- the box, the prior, the starts ----
    lo, hi = np.zeros(d), np.ones(d)
    box = np.stack([low_u, low_u + span_u], axis=1)
    if bounds is not None:
        if isinstance(bounds, dict):
            for key, pair in bounds.items():
                j = _index_of(key, names, 'bounds')
                if j not in cols:
                    raise ValueError(f"bounds: '{names[j]}' is not an unknown input")
                box[cols.index(j)] = [box[cols.index(j), s] if pair[s] is None else float(pair[s]) for s in (0, 1)]
        else:
            box = np.array(bounds, dtype=np.float64)
        if box.shape != (d, 2) or not np.isfinite(box).all():
            raise ValueError(f"bounds must be {{unknown: (lo, hi)}} or [{d}, 2] finite numbers (true scale)")
        lo, hi = (box[:, 0] - low_u) / span_u, (box[:, 1] - low_u) / span_u
        if np.any(lo < -1e-12) or np.any(hi > 1 + 1e-12):
            raise ValueError("bounds reach outside the training range (minmax): the model is not extrapolated")
        lo, hi = np.clip(lo, 0.0, 1.0), np.clip(hi, 0.0, 1.0)
        if not np.all(lo < hi):
            raise ValueError("bounds: lo < hi is needed for every unknown (a fixed input is a known input)")
    mean_n, prec_n = np.zeros(d), np.zeros(d)
    for key, pair in dict(prior or {}).items():
        j = _index_of(key, names, 'prior')
        if j not in cols:
            raise ValueError(f"prior: '{names[j]}' is not an unknown input")
        mu, sd = float(pair[0]), float(pair[1])
        if not (np.isfinite(mu) and sd > 0 and np.isfinite(sd)):
            raise ValueError(f"prior['{key}'] must be (mean, sd) with a finite mean and sd > 0 (true scale)")
        i = cols.index(j)
        mean_n[i], prec_n[i] = (mu - low_u[i]) / span_u[i], (span_u[i] / sd) ** 2
    if starts is None:
        x0 = _optimize.start_points(WALKERS, lo, hi)
    else:
        user = np.array(starts, dtype=np.float64)
        if user.shape != (WALKERS, d) or not np.isfinite(user).all():
            raise ValueError(f"starts must be finite numbers [{WALKERS}, {d}] (true scale)")
        x0 = (user - low_u) / span_u
    if not np.all((x0 > lo) & (x0 < hi)):
        raise ValueError("every start must lie strictly inside the box")
    for name, value, least in (('burnin', burnin, 0), ('draws', draws, 1), ('thin', thin, 1), ('jump_every', jump_every, 0)):
        if isinstance(value, str) or int(value) != value or int(value) < least:
            raise ValueError(f"{name} must be an integer >= {least}")
    table, n_basis, width = getKernels.pack_phis(phis, getKernels.KERNEL_BERNOULLI)
    n_factors = len({(j, int(o)) for row in mtx_u for j, o in enumerate(row) if o})
    if 3 * n_factors + 4 * d > LDS_ROWS:
        raise ValueError(f"the problem needs {3 * n_factors + 4 * d} values per walker in LDS (3 x {n_factors} distinct (unknown "
                         f"input, order) factors + 4 x {d}), a wavefront's {LDS_ROWS * 512 // 1024} KB hold {LDS_ROWS}")
    return dict(d=d, K=K, T=T, E=betas.shape[0], cols=cols, names=[names[j] for j in cols], mtx_u=mtx_u,
                betas=np.ascontiguousarray(betas), sigsqd=np.ascontiguousarray(sigsqd), h=np.ascontiguousarray(0.5 / sigsqd),
                draw_ids=np.ascontiguousarray(index, dtype=np.uint32), table=table, n_basis=n_basis, width=width,
                lo=np.ascontiguousarray(lo), hi=np.ascontiguousarray(hi), prior_mean=mean_n, prior_prec=prec_n, y=y,
                P=np.ascontiguousarray(P), starts=np.ascontiguousarray(x0), burnin=int(burnin), draws=int(draws),
                thin=int(thin), jump_every=int(jump_every), seed=int(seed) & 0xFFFFFFFF, keep=keep, low=low_u, span=span_u,
                box=box)


# ---------------------------------------------------------------------------------------------------------
# the host statement
# ---------------------------------------------------------------------------------------------------------

def unknown_products(tt, table, theta):
    """U [T, ...] at theta [..., d]: per term the product of its factors in the unknown inputs (``optimize.TermTable`` of
    the unknown columns: ascending input order, from the left), each factor by Horner."""
    shape = theta.shape[:-1]
    fac = np.ones((tt.n_slots + 1,) + shape)
    for s in range(tt.n_slots):
        c, order, x = table[tt.order[s] - 1], tt.order[s], theta[..., tt.src[s]]
        value = np.full(shape, c[order])
        for k in range(order - 1, -1, -1):
            value = value * x + c[k]
        fac[s] = value
    A = fac[tt.slots]                                                  # [T, width, ...]
    product = A[:, 0].copy()
    for i in range(1, tt.width):
        product = product * A[:, i]
    return product


def log_target(tt, table, theta, w, h, y, prior_mean, prior_prec, reverse_terms=False, parts=False):
    """lp [E, n] at theta [E, n, d] with w [E, K, T + 1] = betas x P: the module docstring's sums, in its order
    (``reverse_terms``: the terms after the intercept in descending order, for the tests).  ``parts``: also the scale
    h sum_k (|y_k| + sum_t |term|)**2 + the prior's magnitude, what rounding is measured against."""
    U = unknown_products(tt, table, theta)                             # [T, E, n]
    f = np.repeat(w[:, np.newaxis, :, 0], theta.shape[1], axis=1)      # [E, n, K]
    mag = np.abs(f) if parts else None
    order = range(U.shape[0] - 1, -1, -1) if reverse_terms else range(U.shape[0])
    for t in order:
        term = w[:, np.newaxis, :, t + 1] * U[t][..., np.newaxis]
        f = f + term
        if parts:
            mag = mag + np.abs(term)
    ss = np.zeros(theta.shape[:2])
    big = np.zeros(theta.shape[:2])
    for k in range(y.shape[0]):
        r = y[k] - f[..., k]
        ss = ss + r * r
        if parts:
            big = big + (abs(y[k]) + mag[..., k]) ** 2
    pp = np.zeros(theta.shape[:2])
    for i in range(theta.shape[2]):
        dl = theta[..., i] - prior_mean[i]
        pp = pp + prior_prec[i] * (dl * dl)
    lp = -h[:, np.newaxis] * ss - 0.5 * pp
    return (lp, h[:, np.newaxis] * big + 0.5 * pp) if parts else lp


def sample_host(mtx_u, betas, h, table, lo, hi, prior_mean, prior_prec, y, known_prod, starts, burnin, draws, thin,
                jump_every, seed, draw_ids=None, rows=True, reverse_terms=False, flags=False):
    """Every ensemble in normalised coordinates -- the arguments and the results of ``DeviceContext.infer_inputs``: x [E,
    kept, 64, d], lp [E, kept, 64] (None without ``rows``), sums [E, 64, 2, 2, d], accepted [E, 64, 2], evaluations [E].
    ``flags``: also every accept flag [E, iterations, 64] and every state [E, iterations, 64, d]."""
    mtx_u = np.ascontiguousarray(mtx_u, dtype=np.int32)
    tt = _optimize.TermTable(mtx_u)
    E, d, K = betas.shape[0], mtx_u.shape[1], y.shape[0]
    w = betas[:, np.newaxis, :] * known_prod[np.newaxis, :, :]         # [E, K, T + 1]
    ids = np.arange(E) if draw_ids is None else np.asarray(draw_ids)
    target = lambda theta: log_target(tt, table, theta, w, h, y, prior_mean, prior_prec, reverse_terms)
    x = np.broadcast_to(starts, (E, WALKERS, d)).copy()
    lp = target(x)
    iterations, first_half, kept = burnin + draws, draws // 2, -(-draws // thin)
    x_rows = np.empty((E, kept, WALKERS, d)) if rows else None
    lp_rows = np.empty((E, kept, WALKERS)) if rows else None
    sums = np.zeros((E, WALKERS, 2, 2, d))
    acc = np.zeros((E, WALKERS, 2, d))
    accepted = np.zeros((E, WALKERS, 2), dtype=np.int32)
    evaluations = np.full(E, WALKERS, dtype=np.int64)
    flag_rows = np.zeros((E, iterations, WALKERS), dtype=bool) if flags else None
    state_rows = np.zeros((E, iterations, WALKERS, d)) if flags else None
    shift = 0.5 * (lo + hi)
    rng = lambda t, purpose, count: np.stack([_capi.infer_rng(seed, ids[e], t, purpose, count) for e in range(E)])
    for t in range(iterations):
        jump = jump_every > 0 and t % jump_every == jump_every - 1
        u1, u2, u3 = (rng(t, purpose, WALKERS) for purpose in (_capi.INFER_U1, _capi.INFER_U2, _capi.INFER_U3))
        if jump:
            normal = rng(t, _capi.INFER_JITTER, WALKERS * d).reshape(E, d, WALKERS)
        for half in (0, 1):
            mv = slice(HALF * half, HALF * half + HALF)
            other = HALF * (1 - half)
            xw = x[:, mv]
            take = lambda j: np.take_along_axis(x, j[..., np.newaxis], axis=1)
            if not jump:
                j = other + np.minimum((32.0 * u1[:, mv]).astype(np.int64), HALF - 1)
                z = ((1.0 + u2[:, mv]) * (1.0 + u2[:, mv])) * 0.5
                xj = take(j)
                prop = xj + z[..., np.newaxis] * (xw - xj)
                log_z = (d - 1.0) * np.log(z)
            else:
                a = np.minimum((32.0 * u1[:, mv]).astype(np.int64), HALF - 1)
                b = (a + 1 + np.minimum((31.0 * u2[:, mv]).astype(np.int64), HALF - 2)) % HALF
                n = normal[:, :, mv].transpose(0, 2, 1)
                prop = (xw + (take(other + a) - take(other + b))) + (JITTER * (hi - lo)) * n
                log_z = 0.0
            inside = ((prop > lo) & (prop < hi)).all(axis=-1)
            lp_y = target(np.where(inside[..., np.newaxis], prop, xw))
            with np.errstate(divide='ignore', invalid='ignore'):
                accept = inside & (np.log(u3[:, mv]) < (log_z + lp_y) - lp[:, mv])
            x[:, mv] = np.where(accept[..., np.newaxis], prop, xw)
            lp[:, mv] = np.where(accept, lp_y, lp[:, mv])
            evaluations += inside.sum(axis=1)
            accepted[:, mv, 1 if jump else 0] += accept
            if flags:
                flag_rows[:, t, mv] = accept
        if flags:
            state_rows[:, t] = x
        if t < burnin:
            continue
        r = t - burnin
        if r == first_half and first_half > 0:
            sums[:, :, 0] = acc
            acc[:] = 0.0
        c = x - shift
        acc[:, :, 0] = acc[:, :, 0] + c
        acc[:, :, 1] = acc[:, :, 1] + c * c
        if rows and r % thin == 0:
            x_rows[:, r // thin], lp_rows[:, r // thin] = x, lp
    sums[:, :, 1] = acc
    out = (x_rows, lp_rows, sums, accepted, evaluations)
    return out + (flag_rows, state_rows) if flags else out


def split_rhat(sums, draws, shift):
    """Split R-hat per draw and unknown [E, d] from the per-walker sums [E, 64, 2, 2, d]: 128 chains, the walkers' first
    draws // 2 post-burn-in iterations and their rest; also the pooled mean and standard deviation [E, d] (normalised)."""
    n = np.array([draws // 2, draws - draws // 2], dtype=np.float64)[np.newaxis, np.newaxis, :, np.newaxis]
    s1, s2 = sums[:, :, :, 0], sums[:, :, :, 1]
    total = float(draws * sums.shape[1])
    mean = s1.sum(axis=(1, 2)) / total
    var = np.maximum(s2.sum(axis=(1, 2)) / total - mean * mean, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        chain_mean = s1 / n
        chain_var = (s2 - s1 * s1 / n) / (n - 1.0)
        W = chain_var.reshape(sums.shape[0], -1, sums.shape[-1]).mean(axis=1)
        B_n = chain_mean.reshape(sums.shape[0], -1, sums.shape[-1]).var(axis=1, ddof=1)
        length = float(draws // 2)
        rhat = np.sqrt(((length - 1.0) / length * W + B_n) / W)
    if draws < 4:
        rhat = np.full_like(rhat, np.nan)
    return rhat, mean + shift, np.sqrt(var)


def _assemble(p, out):
    """An InferResult from the sampler's outputs: true-scale rows, pooled summaries, per-draw diagnostics."""
    x, lp, sums, accepted, evaluations = out
    E, d, span, low = p['E'], p['d'], p['span'], p['low']
    iterations = p['burnin'] + p['draws']
    n_jump = sum(1 for t in range(iterations) if p['jump_every'] > 0 and t % p['jump_every'] == p['jump_every'] - 1)
    tried = np.array([iterations - n_jump, n_jump], dtype=np.float64) * WALKERS
    with np.errstate(divide='ignore', invalid='ignore'):
        accept = accepted.sum(axis=1) / tried
    rhat, mean_e, sd_e = split_rhat(sums, p['draws'], 0.5 * (p['lo'] + p['hi']))
    res = InferResult(unknown=list(p['names']), draws=E, walkers=WALKERS, accept=accept, rhat=rhat,
                      rhat_max=float(np.nanmax(rhat)) if np.isfinite(rhat).any() else float('nan'), evals=evaluations,
                      mean_per_draw=low + mean_e * span, sd_per_draw=sd_e * span, draw_ids=p['draw_ids'].astype(np.int64))
    total = sums[:, :, :, 0].sum(axis=(0, 1, 2)) / float(E * WALKERS * p['draws'])
    res['mean'] = low + (total + 0.5 * (p['lo'] + p['hi'])) * span
    res.update(x=None, lp=None, draw=None, cov=None, quantiles=None)
    if x is not None:
        flat = x.reshape(-1, d)
        rows = low + flat * span
        n = rows.shape[0]
        cut = bounds_cut(n)
        srt = np.sort(rows, axis=0)
        res.update(x=rows, lp=lp.reshape(-1), draw=np.repeat(p['draw_ids'].astype(np.int64), x.shape[1] * WALKERS),
                   mean=rows.mean(axis=0), cov=np.atleast_2d(np.cov(rows, rowvar=False)) if n > 1 else None,
                   quantiles=np.stack([srt[min(cut, n - 1)], srt[max(n - cut, 0)]], axis=1))
    return res


_SIGNATURE = """
    betas, sigsqd : [E_all, terms + 1] and [E_all]: the draws and their sigma^2, as ``resample`` returns them; sigsqd may be
                    None with ``noise``
    mtx, phis, minmax, kernel : the model's (``FoKL.infer_inputs`` passes its own); 'Bernoulli Polynomials' only
    unknown       : the unknown inputs, by name (``xvars``; default 'x1' .. 'xm') or 0-based index; 1 to 16 of them
    known         : [K, m - d] the other inputs at every observation, columns in ascending input order; normalised as the
                    model's inputs are, or in true scale with ``clean=True``
    data          : [K] the observed outputs
    prior         : {unknown: (mean, sd)} independent normal priors in true scale; none: flat inside the box
    bounds        : {unknown: (lo, hi)} or [d, 2] in true scale, inside the training range (the default box)
    noise         : a standard deviation that replaces every draw's sigma^2 by noise**2 (another instrument's measurement)
    starts        : None -- ``optimize.start_points(64, lo, hi)`` -- or [64, d] in true scale, strictly inside the box
    burnin, draws, thin : iterations dropped, iterations after them, every ``thin``-th of those is kept
    jump_every    : a jump move instead of the stretch move at every ``jump_every``-th iteration; 0: never
    seed          : of the counter-based random numbers; numpy's stream is not touched
    keep          : 'x' the kept rows; None sums, acceptance and R-hat only
    objective     : 'draws' one ensemble per row of betas; 'mean' one ensemble on the mean betas and the mean sigma^2
    posterior     : which rows of betas: None all, an integer the last rows, an integer array those rows.  A draw's random
                    stream belongs to its row, so a subset reproduces those ensembles of the full run

    Returns an ``InferResult`` (a dict with attribute access): x [E * kept * 64, d] in true scale (draw-major, then kept
    row, then walker), lp and draw [E * kept * 64] (the row of betas a sample came from); pooled over the draws mean [d],
    cov [d, d], quantiles [d, 2] = (sorted[cut], sorted[n - cut]) with ``evaluate``'s cut = floor(0.025 n) + 1; per draw
    accept [E, 2] (stretch, jump acceptance rates), rhat [E, d] (split R-hat over the 64 walkers' halves) and rhat_max,
    evals [E] target evaluations, mean_per_draw, sd_per_draw [E, d].  With keep=None x, lp, draw, cov and quantiles are None
    and mean comes from the sums."""


def infer_inputs(betas, sigsqd, mtx, phis, minmax, kernel, unknown, known, data, device=None, **kwargs):
    """Which inputs produced these outputs?  One ensemble of 64 walkers per posterior draw, on the device.

    device        : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare(betas, sigsqd, mtx, phis, minmax, kernel, unknown, known, data, **kwargs)
    ctx = _device_context(device)
    out = ctx.infer_inputs(p['mtx_u'], p['betas'], p['h'], p['table'], p['lo'], p['hi'], p['prior_mean'], p['prior_prec'],
                           p['y'], p['P'], p['starts'], p['burnin'], p['draws'], p['thin'], p['jump_every'], p['seed'],
                           draw_ids=p['draw_ids'], rows=p['keep'] == 'x')
    return _assemble(p, out)


def infer_inputs_host(betas, sigsqd, mtx, phis, minmax, kernel, unknown, known, data, **kwargs):
    """``infer_inputs`` with the ensembles in numpy on this host: the statement of the algorithm (module docstring), for
    tests and for reading.  Same arguments, same result fields."""
    p = _prepare(betas, sigsqd, mtx, phis, minmax, kernel, unknown, known, data, **kwargs)
    out = sample_host(p['mtx_u'], p['betas'], p['h'], p['table'], p['lo'], p['hi'], p['prior_mean'], p['prior_prec'], p['y'],
                      p['P'], p['starts'], p['burnin'], p['draws'], p['thin'], p['jump_every'], p['seed'],
                      draw_ids=p['draw_ids'], rows=p['keep'] == 'x')
    return _assemble(p, out)


infer_inputs.__doc__ += _SIGNATURE
infer_inputs_host.__doc__ += _SIGNATURE

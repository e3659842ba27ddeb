"""
Simulate a dynamic system whose right-hand sides are fitted models, for every posterior draw at once, on the device.

``simulate(models, states, inputs, forcing, y0, t, ...)`` integrates d(states[k])/dt = models[k](its inputs) with the
classical Runge-Kutta scheme, one trajectory ("member") per posterior draw and / or initial state, and returns the mean
and the order-statistic band over the members.  It is to ``GP_Integrate_ensemble`` what ``optimize_system`` is to
``optimize``: the fitted models as they are, wired by variable names.

  * either kernel, also mixed in one system; a cubic-spline model is evaluated on the fit's own 499 pieces (FR:570-589),
    so a trajectory is a trajectory of what ``evaluate`` returns;
  * ``inputs[k]`` names model k's input columns in the order of its ``mtx`` columns: states and forcing keys, any order,
    any subset;
  * states, ``y0``, forcing and ``bounds`` are in true scale; every model normalises each of its inputs with its own
    ``minmax`` row of that column;
  * a member that runs into the edge of the training range is clamped as in the reference (GI:204-269), and
    ``first_saturation`` says at which step that first happened.

``GP_Integrate`` and ``GP_Integrate_ensemble`` stay what they are: the reference's integrator, statement for statement.

The arithmetic (``simulate_host`` is its statement in numpy, the device kernel follows it operation for operation; only
+ - * /, ceil and comparisons, nothing fused, so the two agree bit for bit):

  normalisation   v = (x - lo) / (hi - lo); v > 1 -> 1; v < 0 -> 0                       (lo, hi: the model's minmax row)
  spline order o  p = ceil(499 v); p += (p == 0); p -= 1; s = 499 v - p; c0 + s (c1 + s (c2 + s c3)) of piece p
  Bernoulli o     Horner over phis[o - 1][0 .. o], highest coefficient first
  term            the product of its factors in column order
  model           0 + betas[1] term_1 + betas[2] term_2 + ... (top to bottom), then + betas[0], then * h
  slope rule      the stage's slope of state k is set to zero where the stage point is >= the box's upper edge and the
                  slope is > 0, or <= the lower edge and the slope is < 0
  step            stage points y, y + d1 / 2, y + d2 / 2, y + d3; y += (((d1 + 2 d2) + 2 d3) + d4) / 6
  forcing         row s of every forcing array serves the four stages of step s (zero-order hold, GI:187)

Step s takes point s of ``t`` to point s + 1.  ``first_saturation[e]`` is the first s in which, for member e, a
normalised input (a state's or a forcing value's) was clamped or the slope rule changed a slope; -1 if none did.

``assimilate(models, states, inputs, ..., observe, data, ...)`` filters the same system against measurements: a bootstrap
particle filter of 64 particles per posterior draw, every draw at once on the device.  It returns the filtered states
(per draw and pooled over the draws), and per draw the log marginal likelihood of the measurements, which normalised
over the draws re-weights the model's posterior without a refit.  ``assimilate_host`` is its statement in numpy.

The filter's arithmetic, per draw e with id ``draw_ids[e]`` (the selected row of ``betas``, so a subset of the draws
reproduces the full run), per particle (lane) i:

  start           y_j = y0_j + y0_sd_j normal(step 0, purpose INIT, index 64 j + i); W_i = 1 / 64
  step s          one step of ``simulate`` above, operation for operation, with the draw's coefficients (point s -> s + 1)
  process noise   y_j = y_j + q_j normal(step s + 1, purpose j, index i), q_j = process_sd_j sqrt(h) formed once; nothing
                  is drawn or added where q_j == 0
  weighting       at a point that carries row r of ``data``, over the present (not NaN) entries o in the order of ``observe``:
                  lw_i = -0.5 (0 + ((data_o - y_obs(o)) / obs_sd_o)^2 + ...); m = max_i lw_i; g_i = W_i exp(lw_i - m);
                  G = sum_i g_i; the log evidence grows by (m + log G) - sum_o log(obs_sd_o sqrt(2 pi)); W_i = g_i / G.
                  A row without a present entry changes neither weights nor evidence and does not resample
  statistics      taken there, before resampling: ESS = 1 / sum_i W_i^2, mu_j = sum_i W_i y_ij,
                  var_j = sum_i W_i ((y_ij - mu_j) (y_ij - mu_j))
  resampling      if ESS < resample_below 64: u = uniform(step = the point, purpose RESAMPLE, index 0), c = the inclusive
                  prefix sum of W, particle i takes the ancestor a_i = min(63, #{k : c_k <= (i + u) / 64 c_63}); the
                  states are gathered and W_i = 1 / 64
  collapse        if G is not a positive finite number, or m < -745 (exp(m) is no positive double: every particle is
                  impossibly far from the row) or m is NaN: the row's increment is -inf, so the draw's evidence is -inf
                  from there on; W_i = 1 / 64; ``collapsed[e]`` keeps the first such row.  No other draw is touched
  saturation      ``first_saturation[e]`` is the first step in which a clamp or the slope rule acted for any particle of e

Sums and maxima over the 64 lanes are the xor butterfly with offsets 32, 16, 8, 4, 2, 1: lane i combines its value with
lane i ^ offset's (``lane_sum``, ``lane_max``; the maximum is fmax, which passes over a NaN).  The prefix sum is the
Hillis-Steele scan with offsets 1, 2, 4, 8, 16, 32: c_i += c_(i - offset) for i >= offset (``lane_scan``).  The random
numbers are Philox 4x32-10 (csrc/fokl_philox.h) with key (seed, draw id) and counter (step, purpose, index, 2), drawn
on the host through ``_capi.assimilate_rng``; normals are Box-Muller, one per counter.  Without noise a particle is
``simulate_host``'s member bit for bit; weights, evidence and normals pass through exp / log / cos and agree between the
device and this host to the two maths libraries' last bits.

Pooling over the draws at observation k: draw e weighs exp(log_evidence[e, k]) normalised over the draws (uniform if all
are -inf); ``mean`` is the weighted mean of ``draw_mean``, ``sd`` the root of the weighted within-draw variance plus
the weighted squared distance of ``draw_mean`` to ``mean``.
"""
import numpy as np

from . import _capi
from . import getKernels
from .GP_Integrate import bounds_cut, _device_context
from .optimize import _model_fields

MAX_STATES = 8
MAX_BAND_MEMBERS = 16384
LANES = 64
LDS_BUDGET = 144 * 1024                   # bytes of LDS a wavefront of the kernel may ask for
LDS_ROWS = LDS_BUDGET // (LANES * 8)      # values per member: 1 + factors + normalised states + coefficients
PIECES = getKernels.N_PIECE
SPLINE, BERNOULLI = getKernels.KERNEL_SPLINES, getKernels.KERNEL_BERNOULLI
BERNOULLI_WIDTH = 21                      # coefficients of the highest shipped order (20)


class SimulateResult(dict):
    """A dict whose entries are also attributes (``res.mean``, ``res['mean']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


# ---------------------------------------------------------------------------------------------------------
# the two basis functions as the integrator evaluates them
# ---------------------------------------------------------------------------------------------------------

def spline_value(pieces, v):
    """One cubic-spline basis at normalised v (array): ``pieces`` [499, 4] holds c0 .. c3 of every piece."""
    v = np.asarray(v, dtype=np.float64)
    p = np.ceil(v * 499.0)
    p = p + (p == 0)
    p = p - 1
    s = 499.0 * v - p
    index = np.clip(np.where(np.isfinite(p), p, 0.0), 0, PIECES - 1).astype(np.intp)   # (a NaN reads piece 0, as the kernel)
    c = pieces[index]
    return c[..., 0] + s * (c[..., 1] + s * (c[..., 2] + s * c[..., 3]))


def bernoulli_value(c, v):
    """One Bernoulli basis at normalised v (array): ``c`` its coefficients, lowest power first (a row of ``phis``)."""
    v = np.asarray(v, dtype=np.float64)
    value = np.full(v.shape, float(c[len(c) - 1]))
    for k in range(len(c) - 2, -1, -1):
        value = value * v + float(c[k])
    return value


def spline_pieces(phis, order):
    """Order ``order`` (1-based) of a cubic-spline ``phis`` as [499, 4]."""
    return np.ascontiguousarray(np.stack([np.asarray(phis[order - 1][q], dtype=np.float64) for q in range(4)], axis=1))


# ---------------------------------------------------------------------------------------------------------
# checks and the plan both sides run
# ---------------------------------------------------------------------------------------------------------

def _select(betas, draws, k):
    if draws is None:
        return betas
    if isinstance(draws, str):
        if draws != 'mean':
            raise ValueError("draws must be None (all rows), an integer (the last rows), an index array or 'mean'")
        return np.mean(betas, axis=0, keepdims=True)
    if np.ndim(draws) == 0:
        if int(draws) != draws or not 1 <= int(draws) <= betas.shape[0]:
            raise ValueError(f"draws must be None (all), an integer in 1..{betas.shape[0]} (the last rows of models[{k}]'s "
                             f"betas), an index array or 'mean'")
        return betas[betas.shape[0] - int(draws):]
    index = np.asarray(draws)
    if index.ndim != 1 or index.shape[0] == 0 or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"draws as an array must hold at least one integer index into the {betas.shape[0]} rows of betas")
    return betas[index]


def _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, lds_per_member=True):
    """Every check and every array ``_run_host`` and the device need; touches no device.  ``lds_per_member``: refuse a
    system whose values per member exceed ``simulate``'s LDS (``assimilate`` holds the coefficients once and checks its
    own need)."""
    if models is None or len(models) == 0:
        raise ValueError("simulate needs at least one fitted model (models is empty)")
    models = [_model_fields(model, k) for k, model in enumerate(models)]
    K = len(models)
    states = [str(name) for name in states]
    if len(states) != K or len(inputs) != K:
        raise ValueError(f"states and inputs need one entry per model: {K} models, {len(states)} states, {len(inputs)} input lists")
    if len(set(states)) != K:
        raise ValueError(f"states: every model integrates a state of its own, got {states}")
    if K > MAX_STATES:
        raise ValueError(f"simulate integrates at most {MAX_STATES} states, the system has {K}")
    if keep not in (None, 'members'):
        raise ValueError("keep must be None or 'members'")
    forcing = {str(name): np.asarray(values, dtype=np.float64) for name, values in dict(forcing or {}).items()}
    both = [name for name in forcing if name in states]
    if both:
        raise ValueError(f"forcing: {both} are states")

    start, stop, h = (float(v) for v in t)
    if not (np.isfinite([start, stop, h]).all() and h > 0):
        raise ValueError("t = (start, stop, h) needs finite numbers and h > 0")
    T = np.arange(start, stop + h, h)
    n_steps = len(T) - 1
    if n_steps < 0:
        raise ValueError("t = (start, stop, h) holds no point")
    for name, values in forcing.items():
        if values.ndim != 1:
            raise ValueError(f"forcing['{name}'] must be [steps]")
        if values.shape[0] < n_steps:
            raise ValueError(f"forcing['{name}'] has {values.shape[0]} values but {n_steps} steps are integrated")
        if np.isnan(values[:n_steps]).any():
            raise ValueError(f"forcing['{name}'] holds NaN")

    # ---- the models: kernel, orders, coefficients, and the normalisation of every input column ----
    state_of = {name: j for j, name in enumerate(states)}
    forcing_cols = []                                                 # forcing names some model reads, first seen first
    norms, norm_of = [], {}                                           # (source, lo, hi): source >= 0 a state, -(c + 1) forcing column c
    factors, factor_of = [], {}                                       # (norm, kind, order)
    tables = {}                                                       # (kind, order) -> coefficients
    range_lo, range_hi = np.full(K, -np.inf), np.full(K, np.inf)
    mtxs, betas, term_factors = [], [], []
    for k, model in enumerate(models):
        kernel, phis = model['kernel'], model['phis']
        if kernel in (0, 'Cubic Splines'):
            kind = SPLINE
            if len(phis) == 0 or np.ndim(phis[0][0]) != 1 or len(phis[0]) != 4 or len(phis[0][0]) != PIECES:
                raise ValueError(f"models[{k}]: a 'Cubic Splines' model needs phis of {PIECES} pieces x 4 coefficients per order")
        elif kernel in (1, 'Bernoulli Polynomials'):
            kind = BERNOULLI
            if len(phis) == 0 or np.ndim(phis[0][0]) != 0:
                raise ValueError(f"models[{k}]: a 'Bernoulli Polynomials' model needs its coefficient table in phis")
        else:
            raise ValueError(f"models[{k}]: the kernel {kernel!r} is not supported")
        mtx = np.asarray(model['mtx'])
        if mtx.ndim == 1:
            mtx = mtx[np.newaxis, :]
        if mtx.ndim != 2:
            raise ValueError(f"models[{k}]: mtx must be [terms, inputs]")
        mtx = np.ascontiguousarray(mtx, dtype=np.int32)
        names = [str(name) for name in inputs[k]]
        if len(names) != mtx.shape[1]:
            raise ValueError(f"models[{k}] has {mtx.shape[1]} input columns (mtx.shape[1]), inputs[{k}] names {len(names)}")
        for name in names:
            if name not in state_of and name not in forcing:
                raise ValueError(f"inputs[{k}]: '{name}' is neither a state ({states}) nor a forcing key ({list(forcing)})")
        if mtx.min(initial=0) < 0 or mtx.max(initial=0) > len(phis):
            raise ValueError(f"models[{k}]: mtx holds an order outside the coefficient table")
        if kind == BERNOULLI and mtx.max(initial=0) >= BERNOULLI_WIDTH:
            raise ValueError(f"models[{k}]: Bernoulli orders above {BERNOULLI_WIDTH - 1} are not handled")
        b = np.asarray(model['betas'], dtype=np.float64)
        if b.ndim == 1:
            b = b[np.newaxis, :]
        if b.ndim != 2 or b.shape[0] == 0:
            raise ValueError(f"models[{k}]: betas must be [draws, terms + 1] or [terms + 1]")
        if b.shape[1] != mtx.shape[0] + 1:
            raise ValueError(f"models[{k}]: betas has {b.shape[1]} coefficients per draw, mtx describes {mtx.shape[0]} "
                             f"terms + the constant")
        b = _select(b, draws, k)
        minmax = model['minmax']
        if len(minmax) != mtx.shape[1]:
            raise ValueError(f"models[{k}]: minmax describes {len(minmax)} inputs, mtx {mtx.shape[1]}")
        low = np.array([float(minmax[j][0]) for j in range(mtx.shape[1])])
        high = np.array([float(minmax[j][1]) for j in range(mtx.shape[1])])
        if not np.all(high - low > 0):
            raise ValueError(f"models[{k}]: minmax must have max > min for every input")
        for j, name in enumerate(names):
            if name in state_of:
                source = state_of[name]
                range_lo[source], range_hi[source] = max(range_lo[source], low[j]), min(range_hi[source], high[j])
        rows, checked = [], set()
        for i in range(mtx.shape[0]):
            row = []
            for j in range(mtx.shape[1]):
                order = int(mtx[i, j])
                if order == 0:
                    continue
                if order not in checked:                              # once per model and order
                    checked.add(order)
                    c = spline_pieces(phis, order) if kind == SPLINE else np.array(phis[order - 1][:order + 1], dtype=np.float64)
                    if kind == BERNOULLI and c.shape[0] != order + 1:
                        raise ValueError(f"models[{k}]: order {order} of its Bernoulli table has {c.shape[0]} coefficients, "
                                         f"not {order + 1}")
                    if not np.array_equal(tables.setdefault((kind, order), c), c):
                        raise ValueError(f"models[{k}]: its coefficient table (phis) differs from another model's of the "
                                         f"same kernel")
                name = names[j]                                       # a column is normalised where a factor reads it
                if name in state_of:
                    source = state_of[name]
                else:
                    if name not in forcing_cols:
                        forcing_cols.append(name)
                    source = -(forcing_cols.index(name) + 1)
                norm = norm_of.setdefault((source, low[j], high[j]), len(norm_of))
                if norm == len(norms):
                    norms.append((source, low[j], high[j]))
                key = (norm, kind, order)
                if key not in factor_of:
                    factor_of[key] = len(factors)
                    factors.append(key)
                row.append(factor_of[key])
            rows.append(row)
        mtxs.append(mtx)
        betas.append(np.ascontiguousarray(b))
        term_factors.append(rows)

    # ---- members ----
    counts = [b.shape[0] for b in betas]
    if len(set(counts)) > 1:
        raise ValueError(f"member e uses selected row e of every model's betas, but the models select {counts} rows: the "
                         f"counts must agree (thin them with draws=)")
    y0 = np.asarray(y0, dtype=np.float64)
    if y0.ndim not in (1, 2) or y0.shape[-1] != K:
        raise ValueError(f"y0 must be [{K}] (one value per state) or [members, {K}]")
    if np.isnan(y0).any():
        raise ValueError("y0 holds NaN")
    E = counts[0]
    if y0.ndim == 2:
        if y0.shape[0] == 0 or (E != 1 and y0.shape[0] != E):
            raise ValueError(f"y0 has {y0.shape[0]} rows but the models select {E} draws: an initial-condition sweep needs one "
                             f"row per member (or one draw, which is shared)")
        E = y0.shape[0]
    cut = bounds_cut(E)
    if ReturnBounds and not 1 <= cut < E:
        raise ValueError(f"bounds (sorted[{cut}], sorted[{E} - {cut}]) need at least 2 members, there "
                         f"{'is' if E == 1 else 'are'} {E}: pass ReturnBounds=False")
    if ReturnBounds and E > MAX_BAND_MEMBERS:
        raise ValueError(f"bounds are formed over at most {MAX_BAND_MEMBERS} members, there are {E}: pass ReturnBounds=False "
                         f"or thin the draws")

    # ---- the box ----
    if bounds is None:
        box = np.stack([range_lo, range_hi], axis=1)
    else:
        box = np.array(bounds, dtype=np.float64)
        if box.shape != (K, 2) or np.isnan(box).any():
            raise ValueError(f"bounds must be [{K}, 2] numbers (true scale): a lower and an upper edge per state")
    for k, name in enumerate(states):
        if not box[k, 0] < box[k, 1]:
            raise ValueError(f"state '{name}': its box is empty (lower {box[k, 0]}, upper {box[k, 1]})" +
                             ("" if bounds is not None else ": the training ranges of the models that read it have no "
                                                            "interval in common"))

    # ---- order: forcing before state (those by state), splines before Bernoulli; slot 0 of the factor values holds 1.0 ----
    norm_order = sorted(range(len(norms)), key=lambda n: (norms[n][0] >= 0, max(norms[n][0], 0), n))
    norm_slot = {n: i for i, n in enumerate(norm_order)}
    n_norm_forcing = sum(1 for n in norms if n[0] < 0)
    fac_order = sorted(range(len(factors)), key=lambda f: (norms[factors[f][0]][0] >= 0, factors[f][1] != SPLINE, f))
    fac_slot = {f: i for i, f in enumerate(fac_order)}
    used = {kind: sorted(o for (kd, o) in tables if kd == kind) for kind in (SPLINE, BERNOULLI)}
    spline_table = np.zeros((len(used[SPLINE]), PIECES, 4))
    for i, order in enumerate(used[SPLINE]):
        spline_table[i] = tables[(SPLINE, order)]
    bern_table = np.zeros((len(used[BERNOULLI]), BERNOULLI_WIDTH))
    for i, order in enumerate(used[BERNOULLI]):
        bern_table[i, :order + 1] = tables[(BERNOULLI, order)]
    fac_norm = np.array([norm_slot[factors[f][0]] for f in fac_order], dtype=np.int32)
    fac_kind = np.array([factors[f][1] for f in fac_order], dtype=np.int32)
    fac_row = np.array([used[factors[f][1]].index(factors[f][2]) for f in fac_order], dtype=np.int32)
    fac_degree = np.array([factors[f][2] if factors[f][1] == BERNOULLI else 3 for f in fac_order], dtype=np.int32)
    n_forcing_factors = int(sum(1 for f in fac_order if norms[factors[f][0]][0] < 0))
    n_coef = int(sum(m.shape[0] + 1 for m in mtxs))
    n_norm_state = len(norms) - n_norm_forcing
    need = 1 + len(factors) + n_norm_state + n_coef
    if lds_per_member and need > LDS_ROWS:
        raise ValueError(f"the system needs {need} values per member in LDS (1 + {len(factors)} factors + {n_norm_state} "
                         f"normalised states + {n_coef} coefficients), a wavefront's {LDS_BUDGET // 1024} KB hold {LDS_ROWS}")

    # ---- terms as 16-byte entries {slot, slot, slot, coefficient}: a fourth factor continues in the next entry ----
    entries, entry_begin, entry_count, constant = [], [], [], []
    coef = np.empty((n_coef, E))
    at = 0
    for k in range(K):
        constant.append(at)
        entry_begin.append(len(entries))
        for i, row in enumerate(term_factors[k]):
            slots = [fac_slot[f] + 1 for f in row]
            while len(slots) > 3:
                entries.append(slots[:3] + [-1])
                slots = slots[3:]
            entries.append(slots + [0] * (3 - len(slots)) + [at + 1 + i])
        entry_count.append(len(entries) - entry_begin[-1])
        coef[at:at + mtxs[k].shape[0] + 1] = np.broadcast_to(betas[k], (E, betas[k].shape[1])).T
        at += mtxs[k].shape[0] + 1
    F = np.zeros((n_steps, len(forcing_cols)))
    for c, name in enumerate(forcing_cols):
        F[:, c] = forcing[name][:n_steps]
    return dict(
        K=K, E=E, n_steps=n_steps, T=T, h=h, states=states, forcing=np.ascontiguousarray(F), cut=cut,
        norm_src=np.array([norms[n][0] for n in norm_order], dtype=np.int32),
        norm_lo=np.array([norms[n][1] for n in norm_order], dtype=np.float64),
        norm_span=np.array([norms[n][2] - norms[n][1] for n in norm_order], dtype=np.float64),
        n_norm_forcing=n_norm_forcing, n_forcing_factors=n_forcing_factors, fac_norm=fac_norm, fac_kind=fac_kind,
        fac_row=fac_row, fac_degree=fac_degree, spline_table=np.ascontiguousarray(spline_table),
        bern_table=np.ascontiguousarray(bern_table),
        entries=np.ascontiguousarray(np.array(entries, dtype=np.int32).reshape(-1, 4)),
        entry_begin=np.array(entry_begin, dtype=np.int32), entry_count=np.array(entry_count, dtype=np.int32),
        constant=np.array(constant, dtype=np.int32), coef=np.ascontiguousarray(coef),
        y0=np.ascontiguousarray(np.broadcast_to(y0, (E, K)).T), box=np.ascontiguousarray(box),
        want_bounds=bool(ReturnBounds), want_members=keep == 'members', lds_rows=need)


# ---------------------------------------------------------------------------------------------------------
# the statement in numpy, vectorised over members
# ---------------------------------------------------------------------------------------------------------

def _clamped(v):
    acted = (v > 1.0) | (v < 0.0)
    v = np.where(v > 1.0, 1.0, v)
    return np.where(v < 0.0, 0.0, v), acted


def _factor_values(p, fac, xn, first, last):
    for f in range(first, last):
        v = xn[p['fac_norm'][f]]
        if p['fac_kind'][f] == SPLINE:
            fac[f + 1] = spline_value(p['spline_table'][p['fac_row'][f]], v)
        else:
            fac[f + 1] = bernoulli_value(p['bern_table'][p['fac_row'][f], :p['fac_degree'][f] + 1], v)


def _stage(p, fac, xn, at):
    """h * model_k(at) of every state k [K, E] after the slope rule, and per member whether a clamp or the rule acted."""
    K, E = at.shape
    acted = np.zeros(E, dtype=bool)
    for n in range(p['n_norm_forcing'], p['norm_src'].shape[0]):
        xn[n], clamp = _clamped((at[p['norm_src'][n]] - p['norm_lo'][n]) / p['norm_span'][n])
        acted |= clamp
    _factor_values(p, fac, xn, p['n_forcing_factors'], p['fac_norm'].shape[0])
    dy = np.empty((K, E))
    for k in range(K):
        delta, phi = np.zeros(E), np.ones(E)
        for a, b, c, w in p['entries'][p['entry_begin'][k]:p['entry_begin'][k] + p['entry_count'][k]]:
            phi = phi * fac[a]
            phi = phi * fac[b]
            phi = phi * fac[c]
            if w >= 0:
                delta = delta + p['coef'][w] * phi
                phi = np.ones(E)
        s = (delta + p['coef'][p['constant'][k]]) * p['h']
        out = ((at[k] >= p['box'][k, 1]) & (s > 0)) | ((at[k] <= p['box'][k, 0]) & (s < 0))
        dy[k] = np.where(out, 0.0, s)
        acted |= out
    return dy, acted


def _step(p, fac, xn, y, s):
    """Step s of every member: y [K, E] at point s -> (y at point s + 1, per member whether a clamp or the slope rule acted)."""
    E = y.shape[1]
    acted = np.zeros(E, dtype=bool)
    for n in range(p['n_norm_forcing']):
        x = np.full(E, p['forcing'][s, -(p['norm_src'][n] + 1)])
        xn[n], clamp = _clamped((x - p['norm_lo'][n]) / p['norm_span'][n])
        acted |= clamp
    _factor_values(p, fac, xn, 0, p['n_forcing_factors'])
    dy = total = None
    for st in range(4):
        reach, weight = (1.0 if st == 3 else 0.5), (2.0 if st in (1, 2) else 1.0)
        at = y if st == 0 else y + dy * reach
        dy, stage_acted = _stage(p, fac, xn, at)
        total = dy if st == 0 else total + weight * dy
        acted |= stage_acted
    return y + total / 6, acted


def _run_host(p):
    """-> (members [E, K, P], first_saturation [E] int32)"""
    K, E, S = p['K'], p['E'], p['n_steps']
    y = p['y0'].copy()
    members = np.empty((E, K, S + 1))
    members[:, :, 0] = y.T
    first = np.full(E, -1, dtype=np.int32)
    fac = np.ones((1 + p['fac_norm'].shape[0], E))
    xn = np.zeros((p['norm_src'].shape[0], E))
    for s in range(S):
        y, acted = _step(p, fac, xn, y, s)
        members[:, :, s + 1] = y.T
        first = np.where((first < 0) & acted, np.int32(s), first).astype(np.int32)
    return members, first


def _assemble(p, mean, bounds, members, first):
    res = SimulateResult(t=p['T'], mean=mean, first_saturation=first, saturated_fraction=float(np.mean(first >= 0)),
                         states=list(p['states']))
    if p['want_bounds']:
        res['bounds'] = bounds
    if p['want_members']:
        res['members'] = members
    return res


_SIGNATURE = """
    models      : fitted ``FoKL`` objects, or dicts with betas, mtx, phis, minmax, kernel; model k is d(states[k])/dt.
                  'Cubic Splines' and 'Bernoulli Polynomials' models may be mixed
    states      : the names of the integrated states, one per model
    inputs      : per model the names its input columns read, in the order of its ``mtx`` columns: states or keys of
                  ``forcing``, any order, any subset
    forcing     : {name: [steps]} in true scale; value s serves the four stages of step s
    y0          : [n_states], or [E, n_states] for an initial-condition sweep (true scale)
    t           : (start, stop, h): the points are np.arange(start, stop + h, h)
    draws       : None uses every row of each model's betas, an integer the last rows, an index array those rows
                  (``score``'s convention); member e uses selected row e of every model, so the counts must agree.
                  'mean' runs one member on every model's mean coefficients.  One selected row is shared by the members
                  of an initial-condition sweep
    bounds      : [n_states, 2] the box of the states in true scale; default: per state the intersection of the training
                  ranges (minmax) of the models that read it, unbounded if none does
    ReturnBounds: also the band over the members, ``evaluate``'s order statistics: cut = floor(0.025 E) + 1, lower =
                  sorted[cut], upper = sorted[E - cut] (needs 2 <= E <= 16 384)
    keep        : 'members' also returns every member's trajectory

    Returns a ``SimulateResult`` (a dict with attribute access): t [P], mean [n_states, P], bounds [n_states, P, 2],
    members [E, n_states, P], first_saturation [E] int32 (the first step in which a clamp or the slope rule acted for
    that member, -1: never), saturated_fraction.  Nothing is drawn at random; numpy's stream and the fit are left alone."""


def simulate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True, keep=None,
             device=None):
    """Simulate a system of fitted models over every posterior draw, on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep)
    ctx = _device_context(device)
    return _assemble(p, *ctx.simulate_ensemble(p))


def simulate_host(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True,
                  keep=None):
    """``simulate`` in numpy on this host, vectorised over members: the statement the kernel is tested against (module
    docstring), not a fallback.  Same arguments, same result fields."""
    p = _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep)
    members, first = _run_host(p)
    mean = np.mean(members, axis=0)
    band = None
    if p['want_bounds']:
        srt = np.sort(members, axis=0)
        band = np.stack([srt[p['cut']], srt[p['E'] - p['cut']]], axis=-1)
    return _assemble(p, mean, band, members, first)


simulate.__doc__ += _SIGNATURE
simulate_host.__doc__ += _SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# assimilate: a bootstrap particle filter per posterior draw (module docstring)
# ---------------------------------------------------------------------------------------------------------

PARTICLES = _capi.ASSIMILATE_PARTICLES
LW_FLOOR = -745.0                         # below it exp() of the best particle's log weight is no positive double
_LANES = np.arange(PARTICLES)


def lane_sum(v):
    """The sum over the last axis (64 lanes) as the xor butterfly forms it: every lane's value, all the same bits."""
    v = np.array(v, dtype=np.float64)
    for offset in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ offset]
    return v[..., 0]


def lane_max(v):
    """The maximum over the last axis (64 lanes) by the same butterfly; fmax passes over a NaN."""
    v = np.array(v, dtype=np.float64)
    for offset in (32, 16, 8, 4, 2, 1):
        v = np.fmax(v, v[..., _LANES ^ offset])
    return v[..., 0]


def lane_scan(v):
    """The inclusive prefix sum over the last axis (64 lanes) as the Hillis-Steele scan forms it."""
    v = np.array(v, dtype=np.float64)
    for offset in (1, 2, 4, 8, 16, 32):
        v = np.concatenate([v[..., :offset], v[..., offset:] + v[..., :-offset]], axis=-1)
    return v


def systematic_ancestors(W, u):
    """W [..., 64] weights, u [...] in [0, 1) -> the ancestor of every particle [..., 64] (module docstring)."""
    c = lane_scan(W)
    target = (_LANES + np.asarray(u, dtype=np.float64)[..., np.newaxis]) / float(PARTICLES) * c[..., PARTICLES - 1:]
    count = np.sum(c[..., np.newaxis, :] <= target[..., :, np.newaxis], axis=-1)
    return np.minimum(count, PARTICLES - 1)


def _draw_ids(n_rows, draws, E):
    if draws is None:
        ids = np.arange(n_rows)
    elif isinstance(draws, str):
        ids = np.zeros(1, dtype=np.int64)
    elif np.ndim(draws) == 0:
        ids = np.arange(n_rows - int(draws), n_rows)
    else:
        ids = np.asarray(draws) % n_rows
    if ids.shape[0] != E:                                             # one draw shared by an initial-condition sweep
        ids = np.arange(E)
    return ids.astype(np.uint32)


def _per(name, values, count, what):
    try:
        out = np.array(np.broadcast_to(np.asarray(values, dtype=np.float64), (count,)))
    except ValueError:
        raise ValueError(f"{name} needs one value per {what} ({count}), got shape {np.shape(values)}") from None
    return out


def _prepare_assimilate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, observe=None, data=None,
                        obs_points=None, every=None, obs_sd=None, process_sd=None, y0_sd=None, resample_below=0.5, seed=0,
                        keep=None):
    """``_prepare`` and what the filter adds; touches no device."""
    if keep not in (None, 'particles'):
        raise ValueError("keep must be None or 'particles'")
    p = _prepare(models, states, inputs, forcing, y0, t, draws, bounds, False, None, lds_per_member=False)
    K, E, P = p['K'], p['E'], p['n_steps'] + 1
    names = [str(name) for name in (observe if observe is not None else [])]
    if not names:
        raise ValueError("observe must name at least one measured state")
    for name in names:
        if name not in p['states']:
            raise ValueError(f"observe: '{name}' is not a state ({p['states']})")
    if len(set(names)) != len(names):
        raise ValueError(f"observe names a state twice: {names}")
    if (obs_points is None) == (every is None):
        raise ValueError("give either obs_points (indices into t) or every (points k, 2k, ...): exactly one of the two")
    if every is not None:
        if np.ndim(every) != 0 or int(every) != every or int(every) < 1:
            raise ValueError("every must be a positive integer")
        points = np.arange(int(every), P, int(every))
    else:
        points = np.asarray(obs_points)
        if points.ndim != 1 or (points.size and not np.issubdtype(points.dtype, np.integer)):
            raise ValueError("obs_points must be a list of integer indices into t")
        if points.size and (points.min() < 0 or points.max() > P - 1):
            raise ValueError(f"obs_points must lie in 0 .. {P - 1} (the points of t)")
        if np.any(np.diff(points) <= 0):
            raise ValueError("obs_points must be strictly increasing")
    if points.size == 0:
        raise ValueError(f"no observation: no observation point on the {P} points of t")
    data = np.asarray(data if data is not None else [], dtype=np.float64)
    if data.shape != (points.shape[0], len(names)):
        raise ValueError(f"data must be [{points.shape[0]}, {len(names)}] (observation points x observed states), got "
                         f"{list(data.shape)}")
    if np.isinf(data).any():
        raise ValueError("data holds an infinite value (a missing measurement is NaN)")
    if np.isnan(data).all():
        raise ValueError("no observation: every entry of data is NaN")
    obs_sd = _per('obs_sd', obs_sd if obs_sd is not None else [], len(names), 'observed state')
    if not np.all(np.isfinite(obs_sd) & (obs_sd > 0)):
        raise ValueError(f"obs_sd must be positive and finite, got {obs_sd.tolist()}")
    process_sd = _per('process_sd', 0.0 if process_sd is None else process_sd, K, 'state')
    if not np.all(np.isfinite(process_sd) & (process_sd >= 0)):
        raise ValueError(f"process_sd must be non-negative and finite, got {process_sd.tolist()}")
    y0_sd = _per('y0_sd', 0.0 if y0_sd is None else y0_sd, K, 'state')
    if not np.all(np.isfinite(y0_sd) & (y0_sd >= 0)):
        raise ValueError(f"y0_sd must be non-negative and finite, got {y0_sd.tolist()}")
    if not 0.0 <= float(resample_below) <= 1.0:
        raise ValueError(f"resample_below must lie in [0, 1] (a fraction of the {PARTICLES} particles), got {resample_below}")
    if int(seed) != seed:
        raise ValueError("seed must be an integer")
    n_lane_rows = 1 + p['fac_norm'].shape[0] + (p['norm_src'].shape[0] - p['n_norm_forcing'])
    n_coef = p['coef'].shape[0]
    lds_bytes = (n_lane_rows + 1) * LANES * 8 + n_coef * 8
    if lds_bytes > LDS_BUDGET:
        raise ValueError(f"the system needs {lds_bytes} bytes of LDS (({n_lane_rows} factor and state rows + the exchange "
                         f"row) x {LANES} x 8 + {n_coef} coefficients x 8), a wavefront has {LDS_BUDGET}")
    obs_row = np.full(P, -1, dtype=np.int32)
    obs_row[points] = np.arange(points.shape[0], dtype=np.int32)
    log_scale = [float(np.log(sd * np.sqrt(2.0 * np.pi))) for sd in obs_sd]
    obs_const = np.zeros(points.shape[0])
    for r in range(points.shape[0]):
        for o in range(len(names)):
            if not np.isnan(data[r, o]):
                obs_const[r] = obs_const[r] + log_scale[o]
    n_rows = np.atleast_2d(np.asarray(_model_fields(models[0], 0)['betas'])).shape[0]
    p.update(obs_state=np.array([p['states'].index(name) for name in names], dtype=np.int32), obs_sd=obs_sd,
             obs_points=points.astype(np.int64), obs_row=obs_row, data=np.ascontiguousarray(data), obs_const=obs_const,
             process_q=process_sd * np.sqrt(p['h']), y0_sd=y0_sd, threshold=float(resample_below) * PARTICLES,
             seed=int(seed) & 0xFFFFFFFF, draw_ids=_draw_ids(n_rows, draws, E), want_particles=keep == 'particles',
             lds_bytes=lds_bytes)
    return p


def _run_assimilate_host(p, normal_hook=None):
    """-> (stats [E, n_obs, 2 K + 3], particles [E, n_obs, 64, K], weights [E, n_obs, 64], first_saturation, collapsed):
    the rows of fokl_assimilate_ensemble.  ``normal_hook`` (tests) maps every array of normals before it is used."""
    K, E, S, N = p['K'], p['E'], p['n_steps'], PARTICLES
    ids, seed = p['draw_ids'], p['seed']
    n_obs = p['data'].shape[0]
    wide = dict(p, coef=np.repeat(p['coef'], N, axis=1))              # member e * 64 + i is particle i of draw e
    normals = (lambda z: z) if normal_hook is None else normal_hook
    z = normals(_capi.assimilate_rng(seed, ids, 0, _capi.ASSIMILATE_INIT, N * K)).reshape(E, K, N)
    y = np.ascontiguousarray((p['y0'][:, :, np.newaxis] + p['y0_sd'][:, np.newaxis, np.newaxis] * z.transpose(1, 0, 2))
                             .reshape(K, E * N))
    W = np.full((E, N), 1.0 / N)
    stats = np.zeros((E, n_obs, 2 * K + 3))
    particles, weights = np.empty((E, n_obs, N, K)), np.empty((E, n_obs, N))
    first, collapsed = np.full(E, -1, dtype=np.int32), np.full(E, -1, dtype=np.int32)
    fac = np.ones((1 + p['fac_norm'].shape[0], E * N))
    xn = np.zeros((p['norm_src'].shape[0], E * N))

    def observe(point, r, W, collapsed):
        Y = y.reshape(K, E, N)                                        # a view: the gather below writes the particles
        row = p['data'][r]
        present = np.flatnonzero(~np.isnan(row))
        increment, alive = np.zeros(E), np.ones(E, dtype=bool)
        if present.size:
            ss = np.zeros((E, N))
            for o in present:
                dev = (row[o] - Y[p['obs_state'][o]]) / p['obs_sd'][o]
                ss = ss + dev * dev
            lw = -0.5 * ss
            m = lane_max(lw)
            with np.errstate(all='ignore'):
                g = W * np.exp(lw - m[:, np.newaxis])
                G = lane_sum(g)
                alive = (G > 0.0) & (G < np.inf) & (m >= LW_FLOOR)
                W = np.where(alive[:, np.newaxis], g / G[:, np.newaxis], 1.0 / N)
                increment = np.where(alive, (m + np.log(G)) - p['obs_const'][r], -np.inf)
            collapsed = np.where((collapsed < 0) & ~alive, np.int32(r), collapsed).astype(np.int32)
        with np.errstate(all='ignore'):
            ess = 1.0 / lane_sum(W * W)
            for j in range(K):
                mu = lane_sum(W * Y[j])
                dev = Y[j] - mu[:, np.newaxis]
                stats[:, r, j], stats[:, r, K + j] = mu, lane_sum(W * (dev * dev))
        particles[:, r], weights[:, r] = Y.transpose(1, 2, 0), W
        resample = alive & (ess < p['threshold']) if present.size else np.zeros(E, dtype=bool)
        stats[:, r, 2 * K], stats[:, r, 2 * K + 1], stats[:, r, 2 * K + 2] = ess, increment, resample
        if resample.any():
            u = _capi.assimilate_rng(seed, ids, point, _capi.ASSIMILATE_RESAMPLE, 1)[:, 0]
            ancestors = systematic_ancestors(W, u)
            W = W.copy()
            for e in np.flatnonzero(resample):
                Y[:, e, :] = Y[:, e, ancestors[e]]
                W[e] = 1.0 / N
        return W, collapsed

    if p['obs_row'][0] >= 0:
        W, collapsed = observe(0, p['obs_row'][0], W, collapsed)
    for s in range(S):
        with np.errstate(all='ignore'):
            y, acted = _step(wide, fac, xn, y, s)
        y = np.ascontiguousarray(y)
        for j in range(K):
            if p['process_q'][j] != 0.0:
                z = normals(_capi.assimilate_rng(seed, ids, s + 1, j, N))
                y[j] = y[j] + (p['process_q'][j] * z).reshape(E * N)
        first = np.where((first < 0) & acted.reshape(E, N).any(axis=1), np.int32(s), first).astype(np.int32)
        if p['obs_row'][s + 1] >= 0:
            W, collapsed = observe(s + 1, p['obs_row'][s + 1], W, collapsed)
    return stats, particles, weights, first, collapsed


def _draw_weights(log_evidence):
    """exp(log_evidence) normalised over the draws (axis 0); uniform where every draw is -inf."""
    top = np.max(log_evidence, axis=0, keepdims=True)
    with np.errstate(all='ignore'):
        w = np.exp(log_evidence - np.where(np.isfinite(top), top, 0.0))
        total = np.sum(w, axis=0, keepdims=True)
        return np.where(total > 0, w / total, 1.0 / log_evidence.shape[0])


def _assemble_assimilate(p, stats, particles, weights, first, collapsed):
    K, E = p['K'], p['E']
    draw_mean, draw_var = stats[:, :, :K].transpose(0, 2, 1).copy(), stats[:, :, K:2 * K].transpose(0, 2, 1).copy()
    ess, increment, resampled = stats[:, :, 2 * K].copy(), stats[:, :, 2 * K + 1], stats[:, :, 2 * K + 2] != 0
    log_evidence = np.cumsum(increment, axis=1)                       # in observation order; -inf stays -inf
    running = _draw_weights(log_evidence)                             # [E, n_obs]
    w = running[:, np.newaxis, :]
    with np.errstate(all='ignore'):
        mean = np.sum(np.where(w > 0, w * draw_mean, 0.0), axis=0)
        spread = draw_var + (draw_mean - mean[np.newaxis]) * (draw_mean - mean[np.newaxis])
        sd = np.sqrt(np.sum(np.where(w > 0, w * spread, 0.0), axis=0))
    final = running[:, -1].copy()
    u = float(_capi.assimilate_rng(p['seed'], np.zeros(1, dtype=np.uint32), 0, _capi.ASSIMILATE_DRAW_INDEX, 1)[0, 0])
    c = np.cumsum(final)
    chosen = np.minimum(np.searchsorted(c, (np.arange(E) + u) / E * c[-1], side='right'), E - 1)
    res = SimulateResult(t_obs=p['T'][p['obs_points']], mean=mean, sd=sd, draw_mean=draw_mean, draw_var=draw_var,
                         log_evidence=log_evidence, weights=final, ess_draws=float(1.0 / np.sum(final * final)),
                         draw_index=p['draw_ids'][chosen].astype(np.int64), ess=ess, resampled=resampled,
                         first_saturation=first, collapsed=collapsed, states=list(p['states']))
    if p['want_particles']:
        res['particles'], res['particle_weights'] = particles, weights
        n_obs = particles.shape[1]
        band = np.empty((K, n_obs, 2))
        for k in range(n_obs):
            joint = (running[:, k, np.newaxis] * weights[:, k]).ravel()
            for j in range(K):
                values = particles[:, k, :, j].ravel()
                order = np.argsort(values, kind='stable')
                cumulative = np.cumsum(joint[order])
                cumulative = cumulative / cumulative[-1]
                for side, level in enumerate((0.025, 0.975)):
                    band[j, k, side] = values[order[min(int(np.searchsorted(cumulative, level)), values.shape[0] - 1)]]
        res['bounds'] = band
    return res


_ASSIMILATE_SIGNATURE = """
    models, states, inputs, forcing, y0, t, draws, bounds : as for ``simulate``.  Draw e's random numbers are keyed by the
                  row of ``betas`` it selects, so a subset of the draws reproduces the full run's ('mean': id 0; the
                  members of an initial-condition sweep of one draw: 0 .. E - 1)
    observe     : the names of the measured states
    data        : [n_obs, len(observe)] in true scale; NaN is a missing measurement, a row of NaN weighs nothing
    obs_points  : strictly increasing indices into the points of ``t`` (0 .. P - 1), one per row of ``data``; or
    every       : k, for the points k, 2k, ... -- exactly one of the two
    obs_sd      : the measurement noise's standard deviation per observed state (positive)
    process_sd  : per state and per square root of a time unit: a step adds process_sd[j] sqrt(h) z (default 0)
    y0_sd       : per state, the spread of the particles at point 0 (default 0)
    resample_below : resample where the particles' ESS falls below this fraction of 64 (0: never, 1: wherever ESS < 64)
    seed        : of the filter's own counter-based random numbers; numpy's stream, ``setnos`` and the fits are left alone
    keep        : 'particles' also returns the particles and their weights (before resampling) and ``bounds``

    Returns a ``SimulateResult`` (a dict with attribute access): t_obs [n_obs]; mean, sd [n_states, n_obs] pooled over the
    draws with the running draw weights; draw_mean, draw_var [E, n_states, n_obs]; log_evidence [E, n_obs] cumulative;
    weights [E] = exp(log_evidence[:, -1]) normalised, ess_draws = 1 / sum(weights^2); draw_index [E] rows of ``betas``
    drawn proportional to ``weights`` (systematic, from ``seed``), usable as ``draws=``; ess [E, n_obs] before resampling,
    resampled [E, n_obs] bool; first_saturation [E] int32 (the first step in which a clamp or the slope rule acted for any
    particle, -1: never), collapsed [E] int32 (the first observation at which no particle had a positive weight, -1:
    never); with keep='particles' particles [E, n_obs, 64, n_states], particle_weights [E, n_obs, 64] and bounds
    [n_states, n_obs, 2], the weighted 2.5 % / 97.5 % quantiles over (draw, particle)."""


def assimilate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, observe=None, data=None,
               obs_points=None, every=None, obs_sd=None, process_sd=None, y0_sd=None, resample_below=0.5, seed=0, keep=None,
               device=None):
    """Filter a system of fitted models against measurements, one particle filter per posterior draw, on the device
    (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_assimilate(models, states, inputs, forcing, y0, t, draws, bounds, observe, data, obs_points, every, obs_sd,
                            process_sd, y0_sd, resample_below, seed, keep)
    ctx = _device_context(device)
    return _assemble_assimilate(p, *ctx.assimilate_ensemble(p))


def assimilate_host(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, observe=None, data=None,
                    obs_points=None, every=None, obs_sd=None, process_sd=None, y0_sd=None, resample_below=0.5, seed=0,
                    keep=None, normal_hook=None):
    """``assimilate`` in numpy on this host, vectorised over (draws, particles): the statement the kernel is tested
    against (module docstring), not a fallback.  Same arguments, same result fields; ``normal_hook`` (tests) maps every
    array of normals before it is used."""
    p = _prepare_assimilate(models, states, inputs, forcing, y0, t, draws, bounds, observe, data, obs_points, every, obs_sd,
                            process_sd, y0_sd, resample_below, seed, keep)
    return _assemble_assimilate(p, *_run_assimilate_host(p, normal_hook))


assimilate.__doc__ += _ASSIMILATE_SIGNATURE
assimilate_host.__doc__ += _ASSIMILATE_SIGNATURE

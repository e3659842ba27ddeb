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


def _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep):
    """Every check and every array ``_run_host`` and the device need; touches no device."""
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
    if need > LDS_ROWS:
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
        y = y + total / 6
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

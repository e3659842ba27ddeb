"""
Choose the next measurements to find a better optimum: expected improvement and probability of improvement over a pool of
candidate inputs, as a greedy batch.

``design`` picks the rows that teach most about the MODEL and never looks at ``betas``; ``optimize`` finds one continuous
optimum per draw.  ``acquire`` answers the question a surrogate is most often built for: of a pool of experiments that can
be run, which q should be run next to find a better optimum?  There is no closed form as for a classical GP: the posterior
of the fitted function IS the draws.

  f_sd = x_s . beta_d          the fitted function of draw d at pool row s (x_s: the row's basis values, ones first).  There
                               is no noise term: the improvement is in the latent function.
  b_d                          the incumbent of draw d: the best value the draw is known to reach already
  sense='max' works on f; sense='min' is the same computation on -betas and -incumbent (negation is exact), and the
  incumbents reported are flipped back.

  criterion   gain of row s                         after picking s*
  'ei'        (sum_d max(f_sd - b_d, 0)) / E        b_d <- max(b_d, f_s*d)
  'pi'        (sum_d [f_sd > b_d]) / E              b_d <- +inf where f_s*d > b_d, else unchanged

(a row with an f that is not finite has the gain NaN under both.)  A pick is the arg-max over the rows not yet picked; ties
go to the lowest pool index; NaN never wins; a row is taken once (the function is noiseless: a second visit gains 0).  Two
facts follow:

  joint batch   cumsum(gain)[k] is the joint q-EI of the first k + 1 picks formed from scratch,
                mean_d max(max_{s in batch} f_sd - b0_d, 0); for 'pi' the probability that the batch improves.
  greedy bound  both set functions are monotone submodular, so the greedy batch is within 1 - 1 / e of the best batch.

Lazy evaluation (``lazy=True``).  Gains only fall as b rises, and EXACTLY so in floating point: the subtraction, the
comparison with 0, the sum of non-negative terms in a fixed order and the division by E are monotone under correct
rounding, and f_sd is recomputed by the same instructions each time.  So a row's gain of an earlier pick bounds its gain
now, and every pick after the first
  1. finds the un-picked row with the largest stale gain (lowest index on ties),
  2. evaluates that row's 16-row tile fresh; tau is the largest fresh gain among the tile's un-picked rows,
  3. skips every tile whose un-picked rows ALL have a stale gain strictly below tau (a NaN never compares below: such a
     tile is evaluated),
  4. evaluates the other tiles fresh and stores their gains,
  5. takes the arg-max (skipped rows stand in it with their stale gain, which is below a gain that exists).
The index and the gain bits are those of evaluating everything (``lazy=False``), and the set of evaluated tiles follows
from the values alone.  When tau is 0 the batch already covers everything and the pick evaluates every tile.

``incumbent``: 'training' (default) is, per draw, the best value of that draw over the training inputs -- ``propagate``'s
per-draw max (min for sense='min'); a number serves every draw; an [E] array one each; 'none' is -inf ('pi' only: 'ei'
would be infinite).

``acquire`` runs the columns (K1), the training extremes (``fokl_population_stats``) and the selection
(``fokl_acquire_select``, csrc/fokl_acquire_device.inc: the rows x draws product on the fp64 matrix pipe, no host round
trip between the picks) on the device; without the library or a gfx950 device it raises, there is no host fallback.
``acquire_host`` is the same function in numpy with no device: the STATEMENT the kernels are tested against
(``select_host``).  They share ``_prepare`` (every check; touches no device) and ``_run`` and differ only in who forms
the columns and who selects.  Nothing is drawn at random.

Under output limits (``acquire_system``).  Model 0 is the objective, models 1..K (K in 1..7) are constraint models with
limits lo_k <= hi_k, either of which may be infinite.  The draws are paired: member d uses row d of every model's betas.

  g_ksd = xk_s . betak_d       constraint model k of draw d at pool row s
  ok_sd                        every k has g_ksd >= lo_k and g_ksd <= hi_k (a NaN g is therefore infeasible)

  criterion   gain of row s                                    after picking s*
  'ei'        (sum_d ok_sd ? max(f_sd - b_d, 0) : 0.0) / E     b_d <- max(b_d, f_s*d) where ok_s*d
  'pi'        (sum_d ok_sd ? [f_sd > b_d] : 0.0) / E           b_d <- +inf where ok_s*d and f_s*d > b_d

An infeasible draw contributes exactly 0.0 whatever f is; in a feasible draw an f that is not finite makes the gain NaN.
The arg-max, the ties, the mask, ``sense`` and the five-step lazy rule are the ones above, word for word: the criterion
is still monotone submodular and a gain still only falls as b rises, exactly so in floating point (ok_sd does not depend
on b).  cumsum(gain) is mean_d max(max_{s in batch, ok_sd} f_sd - b0_d, 0).  The incumbent 'measured' is, per draw, the
best f over the FEASIBLE rows of ``measured`` (-inf where there is none).  ``select_system_host`` is the statement of
``fokl_acquire_system_select`` and ``incumbent_system_host`` that of ``fokl_acquire_system_incumbent``
(csrc/fokl_acquire_system_device.inc); ``acquire_system_host`` is ``acquire_system`` in numpy, not a fallback.
"""
import os

import numpy as np

from . import _capi
from . import getKernels
from .embedded import basis_matrix, _kernel_id
from .population import population_stats_host

MAX_COLUMNS = _capi.ACQUIRE_MAX_COLUMNS
CRITERIA = ('ei', 'pi')
SENSES = ('max', 'min')
TILE = 16
SPARE_BYTES = 64 << 20


class AcquireResult(dict):
    """A dict whose entries are also attributes (``res.index``, ``res['index']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def gain_rows(F, b, criterion):
    """The gain of every row of F [rows, E] against the incumbent b [E]."""
    with np.errstate(invalid='ignore'):
        if criterion == 'ei':
            t = F - b
            terms = np.where(t <= 0.0, 0.0, t)                  # NaN is not <= 0: it stays
        else:
            terms = np.where(F > b, 1.0, F - F)                 # 0.0, or NaN where f is not finite
        return terms.sum(axis=1) / F.shape[1]


def joint_value(F, b0, batch, criterion):
    """The value of a batch of rows formed from scratch: mean_d max(max_{s in batch} f_sd - b0_d, 0) for 'ei', the share
    of the draws on which some row of the batch is above b0 for 'pi'.  F [S, E] = X betas'."""
    top = F[np.asarray(batch, dtype=int)].max(axis=0)
    return float(np.mean(np.maximum(top - b0, 0.0)) if criterion == 'ei' else np.mean(top > b0))


def select_host(X, betas, b0, picks=1, criterion='ei', lazy=True, trace_pick=-1):
    """The statement of ``fokl_acquire_select``: X [S, nc] the pool's columns, betas [E, nc], b0 [E] (finite or -inf),
    sense 'max' -> dict(index [picks] int64, gain [picks], incumbent_after [E], tiles_evaluated [picks] int64 (16-row tiles
    whose gains were formed for the pick; without ``lazy`` all of them), and with ``trace_pick=k`` trace_g [S], every row's
    gain as it stood when pick k was taken (a skipped tile's rows hold their stale gain), and trace_eval [tiles] uint8).  A
    pick that finds no row (every gain NaN) has index -1, gain -inf and leaves b alone.

    f is formed tile by tile, by the same call every time, so a tile evaluated again returns the same bits.  On integer
    data (every f and every sum an exact integer) the device returns the same BITS for every field; on continuous data its
    sums run in another order and agree to rounding."""
    X = np.asarray(X, dtype=np.float64)
    BT = np.ascontiguousarray(np.asarray(betas, dtype=np.float64).T)
    S, E = X.shape[0], BT.shape[1]
    b = np.array(b0, dtype=np.float64).reshape(-1).copy()
    tiles = -(-S // TILE)
    mask = np.zeros(S, dtype=bool)
    g = np.full(S, np.nan)
    index = np.full(picks, -1, dtype=np.int64)
    gain = np.full(picks, -np.inf)
    count = np.zeros(picks, dtype=np.int64)
    trace_g = trace_eval = None

    def f_of(t):
        return X[t * TILE:(t + 1) * TILE] @ BT

    def evaluate(t):
        g[t * TILE:(t + 1) * TILE] = gain_rows(f_of(t), b, criterion)

    def best_open(values):
        crit = np.where(mask | np.isnan(values), -np.inf, values)
        i = int(np.argmax(crit))                                 # the first of the largest: the lowest index
        return (i, crit[i]) if crit[i] > -np.inf else (-1, -np.inf)

    for k in range(picks):
        evaluated = np.zeros(tiles, dtype=np.uint8)
        if lazy and k > 0:
            c, _ = best_open(g)
            tau = -np.inf
            if c >= 0:
                tc = c // TILE
                evaluate(tc)
                evaluated[tc] = 1
                rows = slice(tc * TILE, (tc + 1) * TILE)
                fresh = g[rows][~mask[rows] & ~np.isnan(g[rows])]
                tau = fresh.max() if fresh.size else -np.inf
            for t in range(tiles):
                rows = slice(t * TILE, (t + 1) * TILE)
                with np.errstate(invalid='ignore'):
                    if not evaluated[t] and np.any(~mask[rows] & ~(g[rows] < tau)):
                        evaluate(t)
                        evaluated[t] = 1
        else:
            for t in range(tiles):
                evaluate(t)
            evaluated[:] = 1
        count[k] = int(evaluated.sum())
        if k == trace_pick:
            trace_g, trace_eval = g.copy(), evaluated
        i, value = best_open(g)
        if i < 0:
            continue
        index[k], gain[k] = i, value
        mask[i] = True
        f = f_of(i // TILE)[i % TILE]
        if criterion == 'ei':
            b = np.where(f > b, f, b)
        else:
            b = np.where(f > b, np.inf, b)
    return dict(index=index, gain=gain, incumbent_after=b, tiles_evaluated=count, trace_g=trace_g, trace_eval=trace_eval)


def _prepare(betas, mtx, phis, kernel, inputs, pool, picks, criterion, sense, incumbent, draws, lazy, keep):
    """Every check of ``acquire`` / ``acquire_host`` (ValueError) and the arguments in the form both use.  Touches no
    device."""
    kid = _kernel_id(kernel)
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}")
    if sense not in SENSES:
        raise ValueError(f"sense must be one of {SENSES}")
    if keep not in (None, 'first'):
        raise ValueError("keep must be None or 'first'")
    if mtx is None:
        raise ValueError("acquire needs a fitted model: call fit first (there is no interaction matrix mtx)")
    if betas is None:
        raise ValueError("acquire needs betas [draws, terms + 1]: the fit's, or what resample returned")
    if inputs is None:
        raise ValueError("acquire needs the fitted model's training inputs [n, M]")
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
        raise ValueError(f"the model has {nc} columns (terms + 1), acquire takes at most {MAX_COLUMNS} (a 16-row tile of basis "
                         f"values in LDS: 160 KiB)")
    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim == 1:
        betas = betas[np.newaxis, :]
    if betas.ndim != 2 or betas.shape[0] < 1:
        raise ValueError("betas must be [draws, terms + 1]")
    if betas.shape[1] != nc:
        raise ValueError(f"betas have {betas.shape[1]} columns, the interaction matrix wants {nc} (terms + 1)")
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
    if picks > S:
        raise ValueError(f"{picks} picks from a pool of {S} rows: at most {S} (a row is taken once: the function is noiseless "
                         f"and a second visit gains nothing)")
    bad = ~np.isfinite(pool).all(axis=1)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} of the {S} pool rows are NaN or infinite (the first is row {int(np.flatnonzero(bad)[0])})")
    if not np.isfinite(inputs).all():
        raise ValueError("the training inputs must be finite")
    if kid == getKernels.KERNEL_SPLINES:
        for name, arr in (('pool', pool), ('training inputs', inputs)):
            if arr.min() < 0.0 or arr.max() > 1.0:
                raise ValueError(f"the {name} are not normalized correctly: they must lie in [0, 1] (clean=True normalises them)")
    all_draws = betas.shape[0]
    index = None
    if draws is not None:
        if np.ndim(draws) == 0:
            if int(draws) != draws or not 1 <= int(draws) <= all_draws:
                raise ValueError(f"draws must be None (all), an integer in 1..{all_draws} (the last rows of betas) or an "
                                 f"index array")
            index = np.arange(all_draws - int(draws), all_draws)
        else:
            index = np.asarray(draws)
            if index.ndim != 1 or index.shape[0] < 1 or not np.issubdtype(index.dtype, np.integer) or \
                    index.min() < -all_draws or index.max() >= all_draws:
                raise ValueError(f"draws as an array must hold at least one integer index into the {all_draws} rows of betas")
        betas = betas[index]
    bad = ~np.isfinite(betas).all(axis=1)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} of the {betas.shape[0]} draws are NaN or infinite (the rows of a resample's flagged "
                         f"chains, res.flagged): drop them, e.g. with draws=np.flatnonzero(np.isfinite(res.sigsqd))")
    E = betas.shape[0]
    b0 = None
    if isinstance(incumbent, str):
        if incumbent not in ('training', 'none'):
            raise ValueError("incumbent must be 'training', 'none', a number or an array with one value per draw")
        if incumbent == 'none':
            b0 = np.full(E, -np.inf if sense == 'max' else np.inf)
    else:
        try:
            b0 = np.asarray(incumbent, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("incumbent must be 'training', 'none', a number or an array with one value per draw") from None
        if b0.ndim == 0:
            b0 = np.full(E, float(b0))
        elif b0.ndim == 1 and index is not None and b0.shape[0] == all_draws:
            b0 = b0[index]
        if b0.ndim != 1 or b0.shape[0] != E:
            raise ValueError(f"incumbent as an array must hold one value per draw ({E}), it has the shape {b0.shape}")
        none = -np.inf if sense == 'max' else np.inf
        if np.any(np.isnan(b0)) or np.any(np.isinf(b0) & (b0 != none)):
            raise ValueError(f"every incumbent must be finite, or {none} for a draw with none (sense='{sense}')")
    if b0 is not None and criterion == 'ei' and np.any(np.isinf(b0)):
        raise ValueError("criterion='ei' needs a finite incumbent for every draw: without one the expected improvement is "
                         "infinite (incumbent='none' goes with criterion='pi')")
    cap = os.environ.get('FOKL_ACQUIRE_FREE_BYTES')
    need = 8 * S * (M + nc + 3) + 8 * (nc + 4) * (E + 16)
    if cap is not None and need + SPARE_BYTES > int(cap):
        raise ValueError(f"a pool of {S} rows and {E} draws want {need} bytes on the device (inputs, {nc} columns, gains and the "
                         f"mask per row, {nc} coefficients per draw) and 64 MiB to spare, FOKL_ACQUIRE_FREE_BYTES counts "
                         f"{int(cap)} as free: select from the pool in parts, or thin the draws")
    return dict(kid=kid, mtx=mtx.astype(np.int32), phis=phis, kernel=kernel, inputs=np.ascontiguousarray(inputs),
                pool=np.ascontiguousarray(pool), betas=np.ascontiguousarray(betas), S=S, M=M, nc=nc, E=E, picks=picks,
                criterion=criterion, sense=sense, sign=1.0 if sense == 'max' else -1.0, incumbent=b0, lazy=bool(lazy),
                keep=keep)


class _HostSide:
    """Columns, training extremes and the selection in numpy: what ``acquire_host`` puts in the place of the device."""

    def __init__(self, p):
        self.p = p

    def columns(self, x):
        p = self.p
        return basis_matrix(x, p['mtx'], p['phis'], p['kernel']) if p['mtx'].shape[0] else np.ones((x.shape[0], 1))

    def training_extremes(self):
        """(min, max) [E] of every draw over the training inputs: ``propagate_host``'s."""
        betas = self.p['betas']
        mom, _, _ = population_stats_host(self.columns(self.p['inputs']), betas, betas[:, 0].copy())
        return mom[:, 2].copy(), mom[:, 3].copy()

    def select(self, betas, b0, trace_pick):
        p = self.p
        return select_host(self.columns(p['pool']), betas, b0, p['picks'], p['criterion'], p['lazy'], trace_pick)


class _DeviceSide:
    """Each population uploaded as a dataset, its columns built by K1; the pool last, for the selection."""

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

    def training_extremes(self):
        """(min, max) [E] of every draw over the training inputs: one ``fokl_population_stats`` launch, ``propagate``'s."""
        betas = self.p['betas']
        slots = self._stage(self.p['inputs'])
        mom, _ = self.backend.population_stats(slots, betas, betas[:, 0].copy(), None, False)
        return mom[:, 2].copy(), mom[:, 3].copy()

    def select(self, betas, b0, trace_pick):
        p = self.p
        slots = self._stage(p['pool'])
        return self.backend.acquire_select(slots, betas, b0, p['picks'], p['criterion'], p['lazy'], self.grid_cap, trace_pick)


def _run(p, side):
    sign = p['sign']
    b0 = p['incumbent']
    if b0 is None:                                               # 'training'
        lo, hi = side.training_extremes()
        b0 = hi if sign > 0 else lo
    raw = side.select(sign * p['betas'], sign * b0, 0 if p['keep'] == 'first' else -1)
    if np.any(raw['index'] < 0):
        raise RuntimeError(f"acquire: pick {int(np.flatnonzero(raw['index'] < 0)[0])} found no row to take (every gain was NaN: "
                           f"the fitted function overflows over the pool)")
    return AcquireResult(criterion=p['criterion'], sense=p['sense'], picks=p['picks'], rows=p['S'], draws=p['E'],
                         lazy=p['lazy'], index=raw['index'], x=p['pool'][raw['index']], gain=raw['gain'],
                         joint=np.cumsum(raw['gain']), incumbent=b0, incumbent_after=sign * raw['incumbent_after'],
                         first=raw['trace_g'] if p['keep'] == 'first' else None, tiles_evaluated=raw['tiles_evaluated'],
                         row_tiles=-(-p['S'] // TILE))


_SIGNATURE = """
    betas       : [E_all, terms + 1], rows are draws: the fit's, or what ``resample`` / ``resample_robust`` returned
    mtx, phis, kernel : the fitted model's (``FoKL.acquire`` passes its own)
    inputs      : [n, M] the model's training inputs, NORMALISED as the model's inputs are (incumbent='training' reads them)
    pool        : [S, M] the candidates, normalised likewise (``FoKL.acquire(clean=True)`` normalises the pool)
    picks       : how many rows to choose, at most S
    criterion   : 'ei' (expected improvement) or 'pi' (probability of improvement)
    sense       : 'max' or 'min'
    incumbent   : 'training', a number, an [E] array (or [E_all], thinned with ``draws``), or 'none' ('pi' only)
    draws       : None uses ALL rows of betas, an integer the last ``draws`` rows, an integer array those rows
    lazy        : True skips the tiles whose stale gains cannot win (module docstring); False evaluates everything.  The
                  result is the same bits
    keep        : 'first' also returns ``first`` [S], every row's criterion before the first pick: the classical EI / PI map

    Returns an ``AcquireResult`` (a dict with attribute access): index [picks] rows of the pool in pick order, x [picks, M]
    those rows of ``pool``, gain [picks] each pick's gain when it was taken, joint [picks] = cumsum(gain): the batch's joint
    q-EI / joint probability of improvement, incumbent [E] as used and incumbent_after [E] (under 'pi' a draw the batch
    improves on holds +inf, -inf for sense='min'), first (keep), tiles_evaluated [picks] of row_tiles 16-row tiles."""


def acquire(betas, mtx, phis, kernel, inputs, pool, picks=8, criterion='ei', sense='max', incumbent='training', draws=None,
            lazy=True, keep=None, device=None, grid_cap=0):
    """Which rows of ``pool`` to measure next to find a better optimum, on the device.

    device      : device index (default: the process's device, as for ``fit``) or a backend.  The pool replaces the
                  dataset uploaded to that device's context, as ``evaluate`` and ``propagate`` do.
    grid_cap    : 0 the device's grids; a test hook (the result does not depend on it)"""
    p = _prepare(betas, mtx, phis, kernel, inputs, pool, picks, criterion, sense, incumbent, draws, lazy, keep)
    backend = device if hasattr(device, 'acquire_select') and hasattr(device, 'build_terms') else None
    if backend is None:
        from . import FoKLRoutines
        backend = FoKLRoutines.device_backend(device)
    return _run(p, _DeviceSide(p, backend, grid_cap))


def acquire_host(betas, mtx, phis, kernel, inputs, pool, picks=8, criterion='ei', sense='max', incumbent='training',
                 draws=None, lazy=True, keep=None):
    """``acquire`` with columns, extremes and selection in numpy on this host: the statement of the computation (module
    docstring), for tests and for reading.  Same arguments, same result fields."""
    p = _prepare(betas, mtx, phis, kernel, inputs, pool, picks, criterion, sense, incumbent, draws, lazy, keep)
    return _run(p, _HostSide(p))


acquire.__doc__ += _SIGNATURE
acquire_host.__doc__ += _SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# acquire_system: the same selection under limits on other models' outputs (module docstring)
# ---------------------------------------------------------------------------------------------------------

MAX_MODELS = _capi.ACQUIRE_SYSTEM_MAX_MODELS


def feasible_rows(Gs, lo, hi):
    """ok [rows, E]: every constraint product Gs[k] [rows, E] lies in [lo[k], hi[k]]; a NaN lies in no interval."""
    ok = np.ones(Gs[0].shape, dtype=bool)
    with np.errstate(invalid='ignore'):
        for G, low, high in zip(Gs, lo, hi):
            ok &= (G >= low) & (G <= high)
    return ok


def gain_rows_system(F, ok, b, criterion):
    """``gain_rows`` with the terms of the infeasible draws replaced by exactly 0.0."""
    with np.errstate(invalid='ignore'):
        if criterion == 'ei':
            t = F - b
            terms = np.where(t <= 0.0, 0.0, t)
        else:
            terms = np.where(F > b, 1.0, F - F)
        return np.where(ok, terms, 0.0).sum(axis=1) / F.shape[1]


def joint_value_system(F, ok, b0, batch, criterion):
    """``joint_value`` over the feasible (row, draw) pairs only: mean_d max(max_{s in batch, ok_sd} f_sd - b0_d, 0) for 'ei',
    the share of the draws on which some feasible row of the batch is above b0 for 'pi'."""
    top = np.where(ok, F, -np.inf)[np.asarray(batch, dtype=int)].max(axis=0)
    if criterion == 'pi':
        return float(np.mean(top > b0))
    return float(np.mean(np.maximum(top - b0, 0.0)))             # b0 is finite under 'ei': -inf - b0 is -inf


def incumbent_system_host(Xs, betas, lo, hi):
    """The statement of ``fokl_acquire_system_incumbent``: Xs[k] [n, nc_k] the measured rows' columns of model k, betas[k]
    [E, nc_k] -> (best [E], count [E] int64): per draw the largest f over the rows feasible in that draw (-inf with none;
    NaN if a feasible row's f is not finite) and how many rows are feasible."""
    F = np.asarray(Xs[0], dtype=np.float64) @ np.asarray(betas[0], dtype=np.float64).T
    ok = feasible_rows([np.asarray(X, dtype=np.float64) @ np.asarray(B, dtype=np.float64).T for X, B in zip(Xs[1:], betas[1:])],
                       lo, hi)
    with np.errstate(invalid='ignore'):
        values = np.where(ok, np.where(np.isfinite(F), F, np.nan), -np.inf)
        return values.max(axis=0), ok.sum(axis=0).astype(np.int64)


def select_system_host(Xs, betas, b0, lo, hi, picks=1, criterion='ei', lazy=True, trace_pick=-1):
    """The statement of ``fokl_acquire_system_select``: ``select_host`` with Xs = [X0, X1, ..] (X0 [S, nc_0] the objective's
    columns, Xk those of constraint model k), betas = [B0, B1, ..] (Bk [E, nc_k]), lo / hi [K] the limits of the constraint
    models -> ``select_host``'s dict and feasible [picks] int64, the draws in which each pick is feasible (0 with index -1).
    With infinite limits every field is ``select_host``'s, bit for bit."""
    Xs = [np.asarray(X, dtype=np.float64) for X in Xs]
    BTs = [np.ascontiguousarray(np.asarray(B, dtype=np.float64).T) for B in betas]
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    if len(Xs) != len(BTs) or len(Xs) != lo.shape[0] + 1 or lo.shape != hi.shape:
        raise ValueError("select_system_host: one X and one betas per model, one (lo, hi) per constraint model")
    S, E = Xs[0].shape[0], BTs[0].shape[1]
    b = np.array(b0, dtype=np.float64).reshape(-1).copy()
    tiles = -(-S // TILE)
    mask = np.zeros(S, dtype=bool)
    g = np.full(S, np.nan)
    index = np.full(picks, -1, dtype=np.int64)
    gain = np.full(picks, -np.inf)
    count = np.zeros(picks, dtype=np.int64)
    feasible = np.zeros(picks, dtype=np.int64)
    trace_g = trace_eval = None

    def products(t):
        rows = slice(t * TILE, (t + 1) * TILE)
        return Xs[0][rows] @ BTs[0], feasible_rows([X[rows] @ BT for X, BT in zip(Xs[1:], BTs[1:])], lo, hi)

    def evaluate(t):
        F, ok = products(t)
        g[t * TILE:(t + 1) * TILE] = gain_rows_system(F, ok, b, criterion)

    def best_open(values):
        crit = np.where(mask | np.isnan(values), -np.inf, values)
        i = int(np.argmax(crit))
        return (i, crit[i]) if crit[i] > -np.inf else (-1, -np.inf)

    for k in range(picks):
        evaluated = np.zeros(tiles, dtype=np.uint8)
        if lazy and k > 0:
            c, _ = best_open(g)
            tau = -np.inf
            if c >= 0:
                tc = c // TILE
                evaluate(tc)
                evaluated[tc] = 1
                rows = slice(tc * TILE, (tc + 1) * TILE)
                fresh = g[rows][~mask[rows] & ~np.isnan(g[rows])]
                tau = fresh.max() if fresh.size else -np.inf
            for t in range(tiles):
                rows = slice(t * TILE, (t + 1) * TILE)
                with np.errstate(invalid='ignore'):
                    if not evaluated[t] and np.any(~mask[rows] & ~(g[rows] < tau)):
                        evaluate(t)
                        evaluated[t] = 1
        else:
            for t in range(tiles):
                evaluate(t)
            evaluated[:] = 1
        count[k] = int(evaluated.sum())
        if k == trace_pick:
            trace_g, trace_eval = g.copy(), evaluated
        i, value = best_open(g)
        if i < 0:
            continue
        index[k], gain[k] = i, value
        mask[i] = True
        F, ok = products(i // TILE)
        f, ok = F[i % TILE], ok[i % TILE]
        feasible[k] = int(ok.sum())
        with np.errstate(invalid='ignore'):
            b = np.where(ok & (f > b), f if criterion == 'ei' else np.inf, b)
    return dict(index=index, gain=gain, incumbent_after=b, tiles_evaluated=count, feasible=feasible, trace_g=trace_g,
                trace_eval=trace_eval)


_INCUMBENT_TEXT = "incumbent must be 'measured', 'none', a number or an array with one value per draw"


def _prepare_system(models, xvars, yvars, objective, pool, variables, constraints, picks, criterion, sense, incumbent,
                    measured, no_feasible, draws, lazy, keep):
    """Every check of ``acquire_system`` / ``acquire_system_host`` (ValueError) and the arguments in the form both use: the
    models in the order objective, constraint models (as in ``yvars``), each with its own normalised block of the pool.
    Touches no device."""
    from .optimize import _model_fields
    given = list(models)
    fields = [_model_fields(model, k) for k, model in enumerate(given)]
    count = len(fields)
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}")
    if sense not in SENSES:
        raise ValueError(f"sense must be one of {SENSES}")
    if keep not in (None, 'first'):
        raise ValueError("keep must be None or 'first'")
    if count == 0:
        raise ValueError("acquire_system needs the objective's model and at least one constraint model")
    if count > MAX_MODELS:
        raise ValueError(f"acquire_system handles at most {MAX_MODELS} models (the objective and {MAX_MODELS - 1} constraint "
                         f"models), not {count}")
    if len(xvars) != count or len(yvars) != count:
        raise ValueError("xvars and yvars need one entry per model")
    yvars = [str(name) for name in yvars]
    if len(set(yvars)) != count:
        raise ValueError("yvars: every model needs an output name of its own")
    xvars = [[str(name) for name in ([names] if isinstance(names, str) else names)] for names in xvars]
    union = []
    for names in xvars:
        if len(set(names)) != len(names):
            raise ValueError(f"xvars: a model reads a name twice: {names}")
        union += [name for name in names if name not in union]
    chained = [name for name in yvars if name in union]
    if chained:
        raise ValueError(f"output '{chained[0]}' is also a model's input: chained models make the columns depend on the draw, "
                         f"and rows x draws is then no matrix product; acquire_system does not take them (optimize_system "
                         f"does)")
    objective = str(objective)
    if objective not in yvars:
        raise ValueError(f"objective '{objective}' is not a model output ({yvars})")
    constraints = dict(constraints or {})
    if not constraints:
        raise ValueError("acquire_system needs at least one constraint: without one use acquire")
    limits = {}
    for name, pair in constraints.items():
        if name == objective:
            raise ValueError(f"constraints: '{name}' is the objective: a limit on the objective is not a constraint from "
                             f"another model")
        if name not in yvars:
            raise ValueError(f"constraints: '{name}' is not a model output ({yvars})")
        try:
            lo_c, hi_c = pair
            lo_c = -np.inf if lo_c is None else float(lo_c)
            hi_c = np.inf if hi_c is None else float(hi_c)
        except (TypeError, ValueError):
            raise ValueError(f"constraints['{name}'] must be (lower, upper), numbers or None") from None
        if np.isnan(lo_c) or np.isnan(hi_c):
            raise ValueError(f"constraints['{name}'] must be numbers or None, not NaN")
        if lo_c > hi_c:
            raise ValueError(f"constraints['{name}']: the lower limit {lo_c} is above the upper limit {hi_c}")
        limits[name] = (lo_c, hi_c)
    idle = [name for name in yvars if name != objective and name not in limits]
    if idle:
        raise ValueError(f"model '{idle[0]}' is neither the objective nor constrained: leave it out")
    order = [yvars.index(objective)] + [k for k in range(count) if yvars[k] in limits]
    lo = np.array([limits[yvars[k]][0] for k in order[1:]])
    hi = np.array([limits[yvars[k]][1] for k in order[1:]])

    if variables is None:
        variables = union
    else:
        variables = [str(name) for name in variables]
        if sorted(variables) != sorted(union):
            raise ValueError(f"variables must name every input the models read, once each: {union}")
    V = len(variables)
    if pool is None:
        raise ValueError(f"pool [S, {V}] is needed: the candidate inputs to choose from, in true scale, columns {variables}")
    pool = np.asarray(pool, dtype=np.float64)
    if pool.ndim == 1:
        pool = pool[:, np.newaxis]
    if pool.ndim != 2 or pool.shape[0] < 1 or pool.shape[1] != V:
        raise ValueError(f"pool must be [S, {V}] with at least one row (true scale, columns {variables})")
    S = pool.shape[0]
    if int(picks) != picks or int(picks) < 1:
        raise ValueError("picks must be an integer >= 1")
    picks = int(picks)
    if picks > S:
        raise ValueError(f"{picks} picks from a pool of {S} rows: at most {S} (a row is taken once: the function is noiseless "
                         f"and a second visit gains nothing)")
    bad = ~np.isfinite(pool).all(axis=1)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} of the {S} pool rows are NaN or infinite (the first is row {int(np.flatnonzero(bad)[0])})")

    # ---- the models, objective first ----
    kid = _kernel_id(fields[order[0]]['kernel'])
    packed = getKernels.pack_phis(fields[order[0]]['phis'], kid)
    parts = []
    for k in order:
        model = fields[k]
        same = _kernel_id(model['kernel']) == kid
        if same and model['phis'] is not fields[order[0]]['phis']:
            other = getKernels.pack_phis(model['phis'], kid)
            same = other[1:] == packed[1:] and np.array_equal(other[0], packed[0])
        if not same:
            raise ValueError(f"models[{k}]: its coefficient table (phis) differs from the other models'")
        M = len(xvars[k])
        mtx = np.asarray(model['mtx'])
        mtx = mtx.reshape(0, M) if mtx.size == 0 else np.atleast_2d(mtx)
        if mtx.ndim != 2 or mtx.shape[1] != M:
            raise ValueError(f"models[{k}] has {mtx.shape[-1]} inputs, xvars[{k}] names {M}")
        if np.any(mtx < 0) or np.any(mtx > len(model['phis'])):
            raise ValueError(f"models[{k}]: the interaction matrix holds orders outside the table of {len(model['phis'])} basis "
                             f"functions")
        b = np.asarray(model['betas'], dtype=np.float64)
        if b.ndim == 1:
            b = b[np.newaxis, :]
        if b.ndim != 2 or b.shape[0] < 1:
            raise ValueError(f"models[{k}]: betas must be [draws, terms + 1] or [terms + 1]")
        if b.shape[1] != mtx.shape[0] + 1:
            raise ValueError(f"models[{k}]: betas have {b.shape[1]} columns, the interaction matrix wants {mtx.shape[0] + 1} "
                             f"(terms + 1)")
        minmax = model['minmax']
        if len(minmax) != M:
            raise ValueError(f"models[{k}]: minmax describes {len(minmax)} inputs, mtx {M}")
        low = np.array([float(minmax[j][0]) for j in range(M)])
        span = np.array([float(minmax[j][1]) for j in range(M)]) - low
        if not np.all(span > 0):
            raise ValueError(f"models[{k}]: minmax must have max > min for every input")
        parts.append(dict(k=k, name=yvars[k], mtx=mtx.astype(np.int32), betas=b, low=low, span=span, nc=mtx.shape[0] + 1,
                          cols=np.array([variables.index(name) for name in xvars[k]], dtype=int), xvars=xvars[k]))
    padded = [-(-part['nc'] // 4) * 4 for part in parts]
    if sum(padded) > MAX_COLUMNS:
        raise ValueError(f"the models' columns (terms + 1), each padded to a multiple of 4, add up to {sum(padded)} ({padded}); "
                         f"acquire_system takes at most {MAX_COLUMNS} (a 16-row tile of every model's basis values in LDS: "
                         f"160 KiB)")
    rows = sorted({part['betas'].shape[0] for part in parts} - {1})
    if len(rows) > 1:
        raise ValueError(f"the draws are paired: every model needs the same number of draws (or one row, which is shared): the "
                         f"models have {[part['betas'].shape[0] for part in parts]}")
    all_draws = rows[0] if rows else 1
    index = None
    if draws is not None:
        if np.ndim(draws) == 0:
            if int(draws) != draws or not 1 <= int(draws) <= all_draws:
                raise ValueError(f"draws must be None (all), an integer in 1..{all_draws} (the last rows of betas) or an "
                                 f"index array")
            index = np.arange(all_draws - int(draws), all_draws)
        else:
            index = np.asarray(draws)
            if index.ndim != 1 or index.shape[0] < 1 or not np.issubdtype(index.dtype, np.integer) or \
                    index.min() < -all_draws or index.max() >= all_draws:
                raise ValueError(f"draws as an array must hold at least one integer index into the {all_draws} rows of betas")
    E = all_draws if index is None else index.shape[0]
    for part in parts:
        b = part['betas']
        if b.shape[0] == 1:
            b = np.broadcast_to(b, (E, b.shape[1]))
        elif index is not None:
            b = b[index]
        bad = ~np.isfinite(b).all(axis=1)
        if bad.any():
            raise ValueError(f"models[{part['k']}]: {int(bad.sum())} of the {E} draws are NaN or infinite (the rows of a "
                             f"resample's flagged chains, res.flagged): drop them with draws=")
        part['betas'] = np.ascontiguousarray(b)

    def blocks_of(x):
        return [np.ascontiguousarray((x[:, part['cols']] - part['low']) / part['span']) for part in parts]

    blocks = blocks_of(pool)
    if kid == getKernels.KERNEL_SPLINES:
        for part, block in zip(parts, blocks):
            if block.min() < 0.0 or block.max() > 1.0:
                raise ValueError(f"models[{part['k']}]: the pool reaches outside its minmax: a 'Cubic Splines' model is not "
                                 f"evaluated outside [0, 1]")

    # ---- the incumbent ----
    sign = 1.0 if sense == 'max' else -1.0
    none = -np.inf if sense == 'max' else np.inf
    b0 = measured_blocks = None
    if no_feasible is not None:
        try:
            no_feasible = float(no_feasible)
        except (TypeError, ValueError):
            raise ValueError("no_feasible must be None or a finite number") from None
        if not np.isfinite(no_feasible):
            raise ValueError("no_feasible must be None or a finite number")
    if isinstance(incumbent, str):
        if incumbent not in ('measured', 'none'):
            raise ValueError(_INCUMBENT_TEXT)
        if incumbent == 'none':
            b0 = np.full(E, none)
        else:
            if measured is None:
                head = parts[0]
                for part in parts[1:]:
                    extra = [name for name in part['xvars'] if name not in head['xvars']]
                    if extra:
                        raise ValueError(f"incumbent='measured' without measured= reads the objective model's training inputs, "
                                         f"and the constraint model '{part['name']}' reads {extra}, which the objective does not: "
                                         f"pass measured= [n, {V}] in true scale (columns {variables})")
                source = given[head['k']]
                inputs = source.get('inputs') if isinstance(source, dict) else getattr(source, 'inputs', None)
                if inputs is None:
                    raise ValueError("incumbent='measured' without measured= reads the objective model's training inputs and it "
                                     "has none: pass measured= in true scale")
                inputs = np.asarray(inputs, dtype=np.float64)
                if inputs.ndim == 1:
                    inputs = inputs[:, np.newaxis]
                if inputs.ndim != 2 or inputs.shape[0] < 1 or inputs.shape[1] != len(head['xvars']):
                    raise ValueError(f"the objective model's training inputs must be [n, {len(head['xvars'])}] with at least one "
                                     f"row; or pass measured=")
                measured = np.empty((inputs.shape[0], V))
                measured[:, head['cols']] = head['low'] + inputs * head['span']
            measured = np.asarray(measured, dtype=np.float64)
            if measured.ndim == 1:
                measured = measured[:, np.newaxis]
            if measured.ndim != 2 or measured.shape[0] < 1 or measured.shape[1] != V:
                raise ValueError(f"measured= must be [n, {V}] with at least one row (true scale, columns {variables})")
            if not np.isfinite(measured).all():
                raise ValueError("measured= must be finite")
            measured_blocks = blocks_of(measured)
    else:
        try:
            b0 = np.asarray(incumbent, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(_INCUMBENT_TEXT) from None
        if b0.ndim == 0:
            b0 = np.full(E, float(b0))
        elif b0.ndim == 1 and index is not None and b0.shape[0] == all_draws:
            b0 = b0[index]
        if b0.ndim != 1 or b0.shape[0] != E:
            raise ValueError(f"incumbent as an array must hold one value per draw ({E}), it has the shape {b0.shape}")
        if np.any(np.isnan(b0)) or np.any(np.isinf(b0) & (b0 != none)):
            raise ValueError(f"every incumbent must be finite, or {none} for a draw with none (sense='{sense}')")
    if b0 is not None and criterion == 'ei' and np.any(np.isinf(b0)):
        raise ValueError("criterion='ei' needs a finite incumbent for every draw: without one the expected improvement is "
                         "infinite (incumbent='none' goes with criterion='pi')")
    cap = os.environ.get('FOKL_ACQUIRE_FREE_BYTES')
    total_nc, total_m = sum(part['nc'] for part in parts), sum(len(part['xvars']) for part in parts)
    need = 8 * S * (total_m + total_nc + 3) + 8 * (total_nc + 4) * (E + 16)
    if cap is not None and need + SPARE_BYTES > int(cap):
        raise ValueError(f"a pool of {S} rows and {E} draws want {need} bytes on the device (inputs, {total_nc} columns over "
                         f"{len(parts)} models, gains and the mask per row, {total_nc} coefficients per draw) and 64 MiB to "
                         f"spare, FOKL_ACQUIRE_FREE_BYTES counts {int(cap)} as free: select from the pool in parts, or thin the "
                         f"draws")
    return dict(kid=kid, packed=packed, phis=fields[order[0]]['phis'], kernel=fields[order[0]]['kernel'], parts=parts, lo=lo,
                hi=hi, variables=variables, pool=pool, blocks=blocks, measured_blocks=measured_blocks, S=S, E=E, picks=picks,
                criterion=criterion, sense=sense, sign=sign, incumbent=b0, no_feasible=no_feasible, lazy=bool(lazy), keep=keep,
                constraints={part['name']: (float(lo[j]), float(hi[j])) for j, part in enumerate(parts[1:])})


class _SystemHostSide:
    """Columns, the feasible incumbent and the selection in numpy: what ``acquire_system_host`` puts in the place of the
    device."""

    def __init__(self, p):
        self.p = p

    def columns(self, blocks):
        p = self.p
        return [basis_matrix(x, part['mtx'], p['phis'], p['kernel']) if part['mtx'].shape[0] else np.ones((x.shape[0], 1))
                for part, x in zip(p['parts'], blocks)]

    def incumbent(self, betas):
        return incumbent_system_host(self.columns(self.p['measured_blocks']), betas, self.p['lo'], self.p['hi'])

    def select(self, betas, b0, trace_pick):
        p = self.p
        return select_system_host(self.columns(p['blocks']), betas, b0, p['lo'], p['hi'], p['picks'], p['criterion'], p['lazy'],
                                  trace_pick)


class _SystemDeviceSide:
    """The models' normalised blocks side by side as ONE dataset [rows, sum M_k]; each model's interaction matrix zero
    padded to that width at its block's offset, so that one K1 call per model builds its columns."""

    def __init__(self, p, backend, grid_cap=0):
        self.p, self.backend, self.grid_cap = p, backend, grid_cap

    def _stage(self, blocks):
        from . import engine
        p = self.p
        packed, nb, width = p['packed']
        x = np.ascontiguousarray(np.concatenate(blocks, axis=1))
        self.backend.upload(x, np.zeros(x.shape[0]), p['kid'], packed, nb, width)
        pool = engine.SlotPool(self.backend, initial=max(64, sum(part['nc'] for part in p['parts']) + 3))
        slots, offset = [], 0
        for part, block in zip(p['parts'], blocks):
            mine = [_capi.SLOT_ONES]
            terms = part['mtx'].shape[0]
            if terms:
                wide = np.zeros((terms, x.shape[1]), dtype=np.int32)
                wide[:, offset:offset + block.shape[1]] = part['mtx']
                term_slots = pool.take(terms)
                self.backend.build_terms(wide, term_slots)
                mine = mine + term_slots
            slots.append(mine)
            offset += block.shape[1]
        return slots

    def incumbent(self, betas):
        slots = self._stage(self.p['measured_blocks'])
        return self.backend.acquire_system_incumbent(slots, betas, self.p['lo'], self.p['hi'], self.grid_cap)

    def select(self, betas, b0, trace_pick):
        p = self.p
        slots = self._stage(p['blocks'])
        return self.backend.acquire_system_select(slots, betas, b0, p['lo'], p['hi'], p['picks'], p['criterion'], p['lazy'],
                                                  self.grid_cap, trace_pick)


def _run_system(p, side):
    sign, E = p['sign'], p['E']
    betas = [part['betas'] for part in p['parts']]
    betas[0] = sign * betas[0]
    b = p['incumbent']                                           # in the caller's sense, or None: 'measured'
    measured_feasible = None
    if b is None:
        best, measured_feasible = side.incumbent(betas)
        if np.any(np.isnan(best)):
            raise RuntimeError(f"acquire_system: the objective is not finite at a feasible measured row in "
                               f"{int(np.isnan(best).sum())} of the {E} draws (the fitted function overflows there)")
        b = sign * best                                          # no feasible row: -inf (+inf for sense='min')
        empty = measured_feasible == 0
        if empty.any() and p['no_feasible'] is not None:
            b = np.where(empty, p['no_feasible'], b)
        elif empty.any() and p['criterion'] == 'ei':
            raise ValueError(f"{int(empty.sum())} of the {E} draws have no feasible measured row, so no incumbent, and "
                             f"criterion='ei' needs a finite one for every draw: pass no_feasible=<number> as their incumbent, "
                             f"or use criterion='pi'")
    raw = side.select(betas, sign * b, 0 if p['keep'] == 'first' else -1)
    if np.any(raw['index'] < 0):
        raise RuntimeError(f"acquire_system: pick {int(np.flatnonzero(raw['index'] < 0)[0])} found no row to take (every gain "
                           f"was NaN: the fitted function overflows over the pool)")
    return AcquireResult(criterion=p['criterion'], sense=p['sense'], picks=p['picks'], rows=p['S'], draws=E, lazy=p['lazy'],
                         variables=p['variables'], constraints=p['constraints'], index=raw['index'],
                         x=p['pool'][raw['index']], gain=raw['gain'], joint=np.cumsum(raw['gain']), incumbent=b,
                         incumbent_after=sign * raw['incumbent_after'], feasible_draws=raw['feasible'],
                         p_feasible=raw['feasible'] / E, measured_feasible=measured_feasible,
                         first=raw['trace_g'] if p['keep'] == 'first' else None, tiles_evaluated=raw['tiles_evaluated'],
                         row_tiles=-(-p['S'] // TILE))


_SYSTEM_SIGNATURE = """
    models      : 2 to 8 fitted models (or dicts with betas, mtx, phis, minmax, kernel; the objective's also ``inputs`` for
                  incumbent='measured' without ``measured=``), all of one kernel and one ``phis``
    xvars, yvars: per model the names of its inputs, and the name of its output (as for ``optimize_system``)
    objective   : the output to improve; every other model needs an entry in ``constraints``
    pool        : [S, V] the candidates in TRUE scale, columns in the order of ``variables`` (default: the union of
                  ``xvars`` in the order of first appearance); every model normalises its own inputs with its own minmax
    constraints : {output name: (lower, upper)}, None for no limit on that side
    picks, criterion, sense, draws, lazy, keep : as for ``acquire``; draw d is row d of EVERY model's betas (one row is shared)
    incumbent   : 'measured' (default): per draw the best objective over the rows of ``measured`` [n, V] (true scale) that are
                  feasible in that draw; ``measured=None`` takes the objective model's training inputs back through its
                  minmax (only if no constraint model reads a variable the objective does not).  A draw without a feasible
                  measured row has -inf: 'pi' takes that, 'ei' wants ``no_feasible=<number>`` for those draws.  A number, an
                  [E] array and 'none' as for ``acquire``

    Returns an ``AcquireResult``: index, x (rows of ``pool`` as passed), gain, joint = cumsum(gain), incumbent,
    incumbent_after, feasible_draws [picks] int64 (the draws in which each pick is feasible), p_feasible = feasible_draws / E,
    measured_feasible [E] int64 (feasible measured rows per draw; None unless incumbent='measured'), first (keep),
    tiles_evaluated [picks] of row_tiles 16-row tiles."""


def acquire_system(models, xvars, yvars, objective, pool, variables=None, constraints=None, picks=8, criterion='ei',
                   sense='max', incumbent='measured', measured=None, no_feasible=None, draws=None, lazy=True, keep=None,
                   device=None, grid_cap=0):
    """Which rows of ``pool`` to measure next to improve ``objective`` while the other models' outputs stay within their
    limits, over every posterior draw, on the device (module docstring: "Under output limits").

    device      : device index (default: the process's device) or a backend; the pool replaces the dataset uploaded there
    grid_cap    : 0 the device's grids; a test hook (the result does not depend on it)"""
    p = _prepare_system(models, xvars, yvars, objective, pool, variables, constraints, picks, criterion, sense, incumbent,
                        measured, no_feasible, draws, lazy, keep)
    backend = device if hasattr(device, 'acquire_system_select') and hasattr(device, 'build_terms') else None
    if backend is None:
        from . import FoKLRoutines
        backend = FoKLRoutines.device_backend(device)
    return _run_system(p, _SystemDeviceSide(p, backend, grid_cap))


def acquire_system_host(models, xvars, yvars, objective, pool, variables=None, constraints=None, picks=8, criterion='ei',
                        sense='max', incumbent='measured', measured=None, no_feasible=None, draws=None, lazy=True, keep=None):
    """``acquire_system`` with columns, incumbent and selection in numpy on this host: the statement of the computation, for
    tests and for reading.  Same arguments, same result fields."""
    p = _prepare_system(models, xvars, yvars, objective, pool, variables, constraints, picks, criterion, sense, incumbent,
                        measured, no_feasible, draws, lazy, keep)
    return _run_system(p, _SystemHostSide(p))


acquire_system.__doc__ += _SYSTEM_SIGNATURE
acquire_system_host.__doc__ += _SYSTEM_SIGNATURE

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

"""
Optimise every posterior draw over a pool of runnable experiments: each draw's best rows, the posterior of the optimiser's
location, and Thompson batches.

``optimize`` returns one continuous optimum per draw; ``acquire`` reduces the rows x draws product over the DRAWS for every
pool row (EI, PI).  ``optimize_pool`` reduces it the other way, with the row attached:

  f_sd = x_s . beta_d          the fitted function of draw d at pool row s (x_s: the row's basis values, ones first).  There
                               is no noise term: the optimum is that of the latent function.
  candidates of draw d         the rows that are not excluded and whose f_sd is not NaN (+inf and -inf compare as numbers)
  order                        value descending, on equal values the lower pool index: strict, because indices differ
  ranked[r, d]                 the r-th candidate of draw d in that order, r = 0 .. top - 1; -1 (value -inf) from the rank on
                               at which draw d runs out of candidates
  sense='max' works on f; sense='min' is the same computation on -betas (negation is exact) with the values flipped back.

From ``best = ranked[0]`` follow
  share                        of row s: the part of the draws whose best row it is, the "probability of being optimal";
                               ``rows`` lists the rows with a share, by share descending, then index ascending
  entropy                      -sum share log share, in nats: 0 when every draw agrees, log(len(rows)) when they split evenly
  share_top                    of row s: the part of the draws in which it is among the best ``top``

Thompson batch (``picks=q``).  perm = np.random.default_rng(seed).permutation(E); pick j belongs to draw perm[j % E] and is
that draw's highest-ranked row not already in the batch (``thompson_host``: pure bookkeeping over the ranks).  If the q
draws' best rows are distinct they are the batch.  Otherwise ONE more call ranks only the batch's distinct draws to the
depth min(q, open rows): a pick skips at most the q - 1 rows taken before it, so that depth always suffices.  The rule reads
the ranks alone, so the host twin follows the same path.  It needs no incumbent and has no degenerate case where the draws
agree: they then take ranks 0, 1, 2, ...

``optimize_pool`` runs the columns (K1) and the ranks (``fokl_drawbest_rows``, csrc/fokl_drawbest_device.inc: the rows x
draws product on the fp64 matrix pipe, one pass over the pool per rank, f never stored) on the device; without the library
or a gfx950 device it raises, there is no host fallback.  ``optimize_pool_host`` is the same function in numpy with no
device: the STATEMENT the kernels are tested against (``ranks_host``).  They share ``_prepare`` (every check; touches no
device) and ``_run`` and differ only in who forms the columns and who ranks.

Out of scope: feasibility limits from other models (a later ``optimize_pool_system``), continuous refinement of a row
(``optimize``), and noise in the function values.
"""
import os

import numpy as np

from . import _capi
from . import getKernels
from .acquire import AcquireResult, SENSES, SPARE_BYTES, TILE
from .embedded import basis_matrix, _kernel_id

MAX_COLUMNS = _capi.DRAWBEST_MAX_COLUMNS
MAX_RANKS = _capi.DRAWBEST_MAX_RANKS
MAX_PICKS = 64
_NO_ROW = np.iinfo(np.int64).max


def ranks_host(X, betas, ranks=1, mask=None):
    """The statement of ``fokl_drawbest_rows``: X [S, nc] the pool's columns, betas [E, nc], sense 'max', mask [S] (non-zero:
    no candidate) -> dict(index [ranks, E] int64, value [ranks, E]).  The candidates of draw d are the unmasked rows whose
    f_sd is not NaN; the order is value descending, on equal values index ascending; a draw with fewer than r + 1
    candidates has index -1 and value -inf from rank r on.

    f is formed tile by tile (16 rows), by the same call every time, so a tile evaluated again returns the same bits; only
    the best ``ranks`` of the tiles so far are kept.  On integer data (every f an exact integer) the device returns the
    same BITS; on continuous data its sums run in another order and agree to rounding."""
    X = np.asarray(X, dtype=np.float64)
    BT = np.ascontiguousarray(np.asarray(betas, dtype=np.float64).T)
    S, E = X.shape[0], BT.shape[1]
    ranks = int(ranks)
    closed = np.zeros(S, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    value = np.full((ranks, E), -np.inf)
    index = np.full((ranks, E), _NO_ROW, dtype=np.int64)
    for t in range(-(-S // TILE)):
        rows = np.arange(t * TILE, min((t + 1) * TILE, S), dtype=np.int64)
        with np.errstate(invalid='ignore', over='ignore'):
            f = X[rows] @ BT
        out = closed[rows][:, np.newaxis] | np.isnan(f)
        v = np.concatenate([value, np.where(out, -np.inf, f)])
        i = np.concatenate([index, np.where(out, _NO_ROW, rows[:, np.newaxis])])
        order = np.lexsort((i, -v), axis=0)[:ranks]              # value descending, then index ascending; no row: last
        value, index = np.take_along_axis(v, order, axis=0), np.take_along_axis(i, order, axis=0)
    return dict(index=np.where(index == _NO_ROW, -1, index), value=value)


def thompson_draws(E, picks, seed):
    """The draw every pick of a Thompson batch belongs to: perm[j % E], perm = default_rng(seed).permutation(E).  A
    generator of its own: numpy's global stream is not touched."""
    perm = np.random.default_rng(seed).permutation(int(E))
    return perm[np.arange(int(picks)) % int(E)].astype(np.int64)


def thompson_host(index_of, E, picks, seed):
    """The batch rule: pick j belongs to draw ``thompson_draws(E, picks, seed)[j]`` and is that draw's highest-ranked row
    not already in the batch.  ``index_of(d, r)`` is the row of draw d at rank r, -1 where the draw has none; a [ranks, E]
    array of ranked rows serves too (beyond its depth: none).  -> dict(index [picks] int64, draw [picks] int64, rank [picks]
    int64); a pick whose draw runs out of rows has index -1 and rank -1.  Pure bookkeeping, the same on both sides."""
    if not callable(index_of):
        ranked = np.asarray(index_of)
        index_of = lambda d, r: int(ranked[r, d]) if r < ranked.shape[0] else -1
    draw = thompson_draws(E, picks, seed)
    index = np.full(int(picks), -1, dtype=np.int64)
    rank = np.full(int(picks), -1, dtype=np.int64)
    taken = set()
    for j, d in enumerate(draw):
        r = 0
        while True:
            s = int(index_of(int(d), r))
            if s < 0:
                break
            if s not in taken:
                index[j], rank[j] = s, r
                taken.add(s)
                break
            r += 1
    return dict(index=index, draw=draw, rank=rank)


def shares(rows_per_draw, E):
    """Of the rows in ``rows_per_draw`` [..., E] (-1: none; a row at most once per draw): (rows, share) -- the distinct rows
    and the part of the E draws each appears in, by share descending, then index ascending -- and the entropy
    -sum share log share in nats."""
    flat = np.asarray(rows_per_draw, dtype=np.int64).reshape(-1)
    rows, counts = np.unique(flat[flat >= 0], return_counts=True)
    order = np.lexsort((rows, -counts))
    rows, share = rows[order], counts[order] / float(E)
    return rows, share, float(-np.sum(share * np.log(share)) + 0.0)     # + 0.0: one row's -0.0 reads as 0.0


def rows_of(pool, index):
    """pool[index] with NaN rows where index is -1."""
    index = np.asarray(index, dtype=np.int64)
    x = np.asarray(pool, dtype=np.float64)[np.maximum(index, 0)]
    x[index < 0] = np.nan
    return x


def _prepare(betas, mtx, phis, kernel, pool, sense, top, picks, seed, exclude, draws):
    """Every check of ``optimize_pool`` / ``optimize_pool_host`` (ValueError) and the arguments in the form both use.
    Touches no device."""
    kid = _kernel_id(kernel)
    if sense not in SENSES:
        raise ValueError(f"sense must be one of {SENSES}")
    if mtx is None:
        raise ValueError("optimize_pool needs a fitted model: call fit first (there is no interaction matrix mtx)")
    if betas is None:
        raise ValueError("optimize_pool needs betas [draws, terms + 1]: the fit's, or what resample returned")
    if pool is None:
        raise ValueError("pool [S, M] is needed: the candidate inputs to choose from")
    pool = np.asarray(pool, dtype=np.float64)
    if pool.ndim == 1:
        pool = pool[:, np.newaxis]
    if pool.ndim != 2 or pool.shape[0] < 1 or pool.shape[1] < 1:
        raise ValueError("pool must be [S, M] with at least one row")
    S, M = pool.shape
    mtx = np.asarray(mtx)
    mtx = mtx.reshape(0, M) if mtx.size == 0 else np.atleast_2d(mtx)
    if mtx.ndim != 2 or mtx.shape[1] != M:
        raise ValueError(f"the pool has {M} columns, the interaction matrix has {mtx.shape[-1]}")
    if np.any(mtx < 0) or np.any(mtx > len(phis)):
        raise ValueError(f"the interaction matrix holds orders outside the table of {len(phis)} basis functions")
    nc = mtx.shape[0] + 1
    if nc > MAX_COLUMNS:
        raise ValueError(f"the model has {nc} columns (terms + 1), optimize_pool takes at most {MAX_COLUMNS} (a 16-row tile of "
                         f"basis values in LDS: 160 KiB)")
    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim == 1:
        betas = betas[np.newaxis, :]
    if betas.ndim != 2 or betas.shape[0] < 1:
        raise ValueError("betas must be [draws, terms + 1]")
    if betas.shape[1] != nc:
        raise ValueError(f"betas have {betas.shape[1]} columns, the interaction matrix wants {nc} (terms + 1)")
    bad = ~np.isfinite(pool).all(axis=1)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} of the {S} pool rows are NaN or infinite (the first is row {int(np.flatnonzero(bad)[0])})")
    if kid == getKernels.KERNEL_SPLINES and (pool.min() < 0.0 or pool.max() > 1.0):
        raise ValueError("the pool are not normalized correctly: they must lie in [0, 1] (clean=True normalises them)")
    if int(top) != top or not 1 <= int(top) <= MAX_RANKS:
        raise ValueError(f"top must be an integer in 1..{MAX_RANKS} (one pass over the pool per rank)")
    top = int(top)
    if int(picks) != picks or not 0 <= int(picks) <= MAX_PICKS:
        raise ValueError(f"picks must be an integer in 0..{MAX_PICKS} (0: no batch; a pick may need a rank of its own, and "
                         f"there are at most {MAX_RANKS})")
    picks = int(picks)
    mask = np.zeros(S, dtype=np.uint8)
    if exclude is not None:
        exclude = np.asarray(exclude).reshape(-1)
        if exclude.size and (not np.issubdtype(exclude.dtype, np.integer) or exclude.min() < 0 or exclude.max() >= S):
            raise ValueError(f"exclude must hold integer rows of the pool, 0..{S - 1}")
        mask[exclude.astype(np.int64)] = 1
    open_rows = int(S - mask.sum())
    if open_rows == 0:
        raise ValueError(f"exclude names every one of the {S} pool rows: no row is left to choose from")
    if picks > open_rows:
        raise ValueError(f"{picks} picks from {open_rows} open rows (a pool of {S}, {S - open_rows} excluded): at most "
                         f"{open_rows} (a row is taken once: the function is noiseless and a second visit gains nothing)")
    all_draws = betas.shape[0]
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
    cap = os.environ.get('FOKL_ACQUIRE_FREE_BYTES')
    depth = max(top, picks)
    need = S * (8 * (M + nc) + 1) + 8 * (nc + 2 * depth + 64) * (E + 128)
    if cap is not None and need + SPARE_BYTES > int(cap):
        raise ValueError(f"a pool of {S} rows and {E} draws want {need} bytes on the device (inputs, {nc} columns and the mask "
                         f"per row, {nc} coefficients, {depth} ranks and the row chunks' records per draw) and 64 MiB to spare, "
                         f"FOKL_ACQUIRE_FREE_BYTES counts {int(cap)} as free: rank the pool in parts, or thin the draws")
    return dict(kid=kid, mtx=mtx.astype(np.int32), phis=phis, kernel=kernel, pool=np.ascontiguousarray(pool),
                betas=np.ascontiguousarray(betas), S=S, M=M, nc=nc, E=E, top=top, picks=picks, seed=seed, mask=mask,
                open_rows=open_rows, sense=sense, sign=1.0 if sense == 'max' else -1.0)


class _HostSide:
    """Columns and ranks in numpy: what ``optimize_pool_host`` puts in the place of the device."""

    def __init__(self, p):
        self.p = p
        self.X = None

    def ranks(self, betas, ranks):
        p = self.p
        if self.X is None:
            self.X = basis_matrix(p['pool'], p['mtx'], p['phis'], p['kernel']) if p['mtx'].shape[0] else np.ones((p['S'], 1))
        return ranks_host(self.X, betas, ranks, p['mask'])


class _DeviceSide:
    """The pool uploaded as a dataset, its columns built by K1, once for both calls."""

    def __init__(self, p, backend, grid_cap=0):
        self.p, self.backend, self.grid_cap = p, backend, grid_cap
        self.packed = getKernels.pack_phis(p['phis'], p['kid'])
        self.slots = None

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

    def ranks(self, betas, ranks):
        if self.slots is None:
            self.slots = self._stage(self.p['pool'])
        mask = self.p['mask'] if self.p['mask'].any() else None
        return self.backend.drawbest_rows(self.slots, betas, mask, ranks, self.grid_cap)


def _run(p, side):
    sign, E, top, q = p['sign'], p['E'], p['top'], p['picks']
    betas = sign * p['betas']
    raw = side.ranks(betas, top)
    ranked, best = raw['index'], raw['index'][0]
    rows, share, entropy = shares(best, E)
    rows_top, share_top, _ = shares(ranked, E)
    res = AcquireResult(sense=p['sense'], rows_in_pool=p['S'], open_rows=p['open_rows'], draws=E, top=top, picks=q,
                        best=best, value=sign * raw['value'][0], x_best=rows_of(p['pool'], best), ranked=ranked,
                        ranked_value=sign * raw['value'], rows=rows, share=share, entropy=entropy, rows_top=rows_top,
                        share_top=share_top, no_candidate=int(np.sum(best < 0)))
    if q > 0:
        draw = thompson_draws(E, q, p['seed'])
        first = best[draw]
        second_call = bool(np.any(first < 0)) or np.unique(first).shape[0] < q
        if not second_call:
            batch = dict(index=first.copy(), draw=draw, rank=np.zeros(q, dtype=np.int64))
        else:
            distinct = np.unique(draw)
            depth = min(q, p['open_rows'])
            deep = side.ranks(betas[distinct], depth)['index']
            column = {int(d): k for k, d in enumerate(distinct)}
            batch = thompson_host(lambda d, r: deep[r, column[d]] if r < depth else -1, E, q, p['seed'])
        if np.any(batch['index'] < 0):
            j = int(np.flatnonzero(batch['index'] < 0)[0])
            raise RuntimeError(f"optimize_pool: pick {j} found no row to take (draw {int(batch['draw'][j])} has too few rows "
                               f"whose value is not NaN: the fitted function overflows over the pool)")
        res.update(index=batch['index'], x=p['pool'][batch['index']], draw=batch['draw'], rank=batch['rank'],
                   second_call=second_call)
    return res


_SIGNATURE = """
    betas       : [E_all, terms + 1], rows are draws: the fit's, or what ``resample`` / ``resample_robust`` returned
    mtx, phis, kernel : the fitted model's (``FoKL.optimize_pool`` passes its own)
    pool        : [S, M] the candidates, NORMALISED as the model's inputs are (``FoKL.optimize_pool(clean=True)`` normalises)
    sense       : 'max' or 'min'
    top         : ranks per draw, 1..64 (one pass over the pool each)
    picks       : 0, or the size q <= 64 of a Thompson batch, at most the number of open rows
    seed        : of the batch's permutation of the draws (a generator of its own)
    exclude     : integer array of pool rows that are no candidates, e.g. rows already measured
    draws       : None uses ALL rows of betas, an integer the last ``draws`` rows, an integer array those rows

    Returns an ``AcquireResult`` (a dict with attribute access): best [E] int64 and value [E], every draw's best row and its
    f (-1 / -inf, +inf for 'min': the draw has no candidate; ``no_candidate`` counts them); x_best [E, M] = pool[best];
    ranked [top, E] and ranked_value [top, E]; rows and share, the distinct best rows and their share of the draws (by
    share descending, then index ascending; the shares sum to 1 when every draw has a candidate); entropy in nats; rows_top
    and share_top, the same for "among the best ``top``".  With ``picks=q``: index [q] the batch in pick order, x [q, M] those
    rows of ``pool``, draw [q] and rank [q] -- pick j is the row of rank[j] of draw[j] -- and second_call, whether the draws'
    best rows collided so that a second call ranked the batch's draws deeper.  Also sense, top, picks, draws (E),
    rows_in_pool (S) and open_rows (S less the excluded)."""


def optimize_pool(betas, mtx, phis, kernel, pool, sense='max', top=1, picks=0, seed=0, exclude=None, draws=None, device=None,
                  grid_cap=0):
    """For every posterior draw its best rows of ``pool``, the share of the draws each row wins, and a Thompson batch, on the
    device.

    device      : device index (default: the process's device, as for ``fit``) or a backend.  The pool replaces the
                  dataset uploaded to that device's context, as ``evaluate`` and ``propagate`` do.
    grid_cap    : 0 the device's grids; a test hook (the result does not depend on it)"""
    p = _prepare(betas, mtx, phis, kernel, pool, sense, top, picks, seed, exclude, draws)
    backend = device if hasattr(device, 'drawbest_rows') and hasattr(device, 'build_terms') else None
    if backend is None:
        from . import FoKLRoutines
        backend = FoKLRoutines.device_backend(device)
    return _run(p, _DeviceSide(p, backend, grid_cap))


def optimize_pool_host(betas, mtx, phis, kernel, pool, sense='max', top=1, picks=0, seed=0, exclude=None, draws=None):
    """``optimize_pool`` with columns and ranks in numpy on this host: the statement of the computation (module docstring),
    for tests and for reading.  Same arguments, same result fields."""
    p = _prepare(betas, mtx, phis, kernel, pool, sense, top, picks, seed, exclude, draws)
    return _run(p, _HostSide(p))


optimize_pool.__doc__ += _SIGNATURE
optimize_pool_host.__doc__ += _SIGNATURE

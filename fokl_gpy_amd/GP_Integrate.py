"""
GP_Integrate -- Runge-Kutta integration of a dynamical system whose right-hand sides are fitted BSS-ANOVA models.

``GP_Integrate`` is the same call as the reference's ``FoKL.GP_Integrate.GP_Integrate``
(/root/reference/src/FoKL/GP_Integrate.py:5-282, "GI" below); the loop itself runs in libfokl_hip.so
(``fokl_gp_integrate``, csrc/fokl_integrate.cpp).  ONE trajectory is host work by nature: thousands of dependent steps
with a few hundred flops each.  What the method is for is not one trajectory: a fit returns a thousand posterior draws
per model, and the trajectory with its uncertainty is one integration per draw.  Those are independent of each other, so
``GP_Integrate_ensemble`` integrates them all at once on the device (``fokl_gp_integrate_ensemble``,
csrc/fokl_integrate_device.inc: one lane per member) and returns the mean and the 95 % band over the members.

Behaviour kept from the reference (both functions):
  * cubic-spline models only, evaluated on 498 intervals (GI:103-131) although the table has 499 pieces;
  * ``Y[:, 0]`` is the initial state; ``GP_Integrate`` advances ``y0`` in place (GI:271 ``y += ...``), the ensemble
    does not (there is no single end state);
  * how a model's input vector is assembled (GI:174-199): its used states in order, normalised with ``norms`` and
    clamped to [0, 1]; then the forcing values -- the FIRST used forcing input contributes the whole row ``b[t]``,
    every further one appends its own column; a model reads only its first ``mtx.shape[1]`` inputs;
  * re-ordering through ``used_inputs`` entries > 1 does not work in the reference (GI:62-67 builds a one-element
    array and indexes past it): an ``IndexError`` is raised here as well.
Not kept: the hard-wired ``np.reshape(y, [2, 1])`` of GI:272 -- any number of states works on the host, up to
``_capi.INTEGRATE_MAX_STATES`` in the ensemble.
"""
import ctypes

import numpy as np

from . import _capi
from . import getKernels


def _route(betas, matrix, b, norms, phis, start, stop, n_states, h, used_inputs, per_member=False):
    """Argument checks and input routing shared by ``GP_Integrate`` and ``GP_Integrate_ensemble``.  With ``per_member`` a
    2-D ``betas[k]`` is kept as [members, rows + 1] (its last axis is checked against the matrix); otherwise it is
    flattened, as the reference's callers pass it.  -> dict of what the native entry points take."""
    if len(betas) != n_states or len(matrix) != n_states or len(used_inputs) != n_states:
        raise ValueError("betas, matrix and used_inputs need one entry per integrated state")
    T = np.arange(start, stop + h, h)
    n_steps = len(T) - 1
    b = np.asarray(b, dtype=np.float64)
    n_other = int(b.size / b.shape[0]) if b.size > 0 else 0           # GI:179
    forcing = np.ascontiguousarray(b.reshape(b.shape[0], n_other)) if n_other else np.zeros((0, 0))
    if n_other and forcing.shape[0] < n_steps:
        raise IndexError(f"b has {forcing.shape[0]} rows but {n_steps} steps are integrated")   # GI:187 b[ind - 1]
    norms = np.ascontiguousarray(norms, dtype=np.float64)
    if norms.shape != (2, n_states):
        raise ValueError("norms must be [2, n_states]: minima on top of maxima")

    packed, n_basis, width = getKernels.pack_phis(phis, 0)
    sources, coeffs, orders = [], [], []
    for k in range(n_states):
        used = np.asarray(used_inputs[k])
        if used.shape[0] < n_states + n_other:
            raise IndexError("used_inputs entries need one flag per state and per forcing input")
        if np.amax(used) > 1:
            raise IndexError("re-ordering inputs through used_inputs > 1 fails in the reference (GP_Integrate.py:62-67)")
        src = [j for j in range(n_states) if used[j] != 0]            # GI:174-178
        first = True
        for jj in range(n_states, n_states + n_other):                # GI:181-196
            if used[jj] != 0:
                src.extend(-(c + 1) for c in range(n_other)) if first else src.append(-(jj - n_states + 1))
                first = False
        mtx = np.ascontiguousarray(np.atleast_2d(matrix[k]), dtype=np.int32)
        if per_member and np.ndim(betas[k]) == 2:
            beta = np.ascontiguousarray(betas[k], dtype=np.float64)
        else:
            beta = np.ascontiguousarray(np.reshape(betas[k], -1), dtype=np.float64)
        if beta.shape[-1] != mtx.shape[0] + 1:
            raise ValueError("every coefficient vector needs one entry per row of its matrix plus the constant")
        if len(src) < mtx.shape[1]:
            raise IndexError("a model has more input columns than used_inputs routes to it")   # GI:125 x[j]
        sources.append(np.array(src, dtype=np.int32))
        coeffs.append(beta)
        orders.append(mtx)
    return dict(T=T, n_steps=n_steps, n_other=n_other, forcing=forcing, norms=norms, packed=packed, n_basis=int(n_basis),
                width=int(width), sources=sources, coeffs=coeffs, orders=orders,
                rows=np.array([m.shape[0] for m in orders], dtype=np.int32),
                cols=np.array([m.shape[1] for m in orders], dtype=np.int32),
                n_src=np.array([s.shape[0] for s in sources], dtype=np.int32))


def _pointer_array(arrays):
    return (ctypes.c_void_p * len(arrays))(*[_capi._ptr(a) for a in arrays])


def GP_Integrate(betas, matrix, b, norms, phis, start, stop, y0, h, used_inputs):
    """
    betas       : list of 1-D coefficient vectors (constant first), one per integrated state -- a draw or the mean
    matrix      : list of interaction matrices, one per state
    b           : forcing inputs over the integration period, already normalised: [steps] or [steps, n_other]
    norms       : [2, n_states] minima (row 0) and maxima (row 1) of the integrated states in the training data
    phis        : cubic-spline coefficients (``model.phis``)
    start, stop, h : T = np.arange(start, stop + h, h)
    y0          : initial state [n_states]; advanced in place
    used_inputs : per state, one flag per (state..., forcing...) input of its model
    returns (T, Y) with Y [n_states, len(T)]
    """
    n_states = len(y0)
    r = _route(betas, matrix, b, norms, phis, start, stop, n_states, h, used_inputs)
    y = np.asarray(y0)
    state = np.ascontiguousarray(y, dtype=np.float64).copy()
    Y = np.empty((n_states, r['n_steps'] + 1), dtype=np.float64)
    lib = _capi.load()
    _capi._check(lib.fokl_gp_integrate(n_states, r['n_other'], r['n_steps'], _pointer_array(r['coeffs']),
                                       _pointer_array(r['orders']), _capi._ptr(r['rows']), _capi._ptr(r['cols']),
                                       _pointer_array(r['sources']), _capi._ptr(r['n_src']),
                                       _capi._ptr(r['forcing']) if r['n_other'] else None, _capi._ptr(r['norms']),
                                       _capi._ptr(r['packed']), r['n_basis'], r['width'], float(h), _capi._ptr(state),
                                       _capi._ptr(Y)))
    try:
        y[...] = state                                                # the reference advances y0 in place (GI:271)
    except (TypeError, ValueError):
        pass
    return r['T'], Y


def bounds_cut(n_members):
    """``evaluate``'s order-statistic convention (FR:973-977): bounds = (sorted[cut], sorted[n_members - cut])."""
    return int(np.floor(0.025 * n_members)) + 1


def _device_context(device):
    """None / device index -> the process-wide context of that device (created on first use: raises without a gfx950
    device, there is no host fallback); a backend or a ``_capi.DeviceContext`` is used as it is."""
    if isinstance(device, _capi.DeviceContext):
        return device
    if hasattr(device, 'ctx') and isinstance(device.ctx, _capi.DeviceContext):
        return device.ctx
    from . import FoKLRoutines
    return FoKLRoutines.device_backend(device).ctx


def GP_Integrate_ensemble(betas, matrix, b, norms, phis, start, stop, y0, h, used_inputs, ReturnBounds=True,
                          ReturnMembers=False, device=None):
    """
    ``GP_Integrate`` for a whole posterior at once, on the device: the trajectory with its uncertainty.

    Arguments as for ``GP_Integrate``, two of them widened:
    betas[k]    : [E, rows_k + 1] -- rows are draws exactly as ``fit`` returns them, e.g. ``betas_k[1000:]`` -- or 1-D
                  (shared by every member)
    y0          : [n_states] (shared) or [E, n_states] (an initial-condition sweep); NOT advanced in place (there is no
                  single end state)
    Member e integrates draw e of every state's model from initial state e.  All 2-D arguments must agree on E; with
    everything 1-D, E = 1.  b, norms, phis, used_inputs, start / stop / h are shared by all members.
    ReturnBounds  : also the 95 % band, ``evaluate``'s convention: cut = floor(0.025 E) + 1, lower = sorted[cut],
                    upper = sorted[E - cut] of the members' values at every point (needs E >= 2, at most 16 384)
    ReturnMembers : also every member's trajectory
    device        : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``

    returns (T, mean[, bounds][, members]): mean [n_states, len(T)] over the members, bounds [n_states, len(T), 2],
    members [E, n_states, len(T)].
    """
    if len(phis) > 0 and np.ndim(phis[0][0]) == 0:
        raise ValueError("GP_Integrate_ensemble integrates cubic-spline models only (phis holds Bernoulli polynomials)")
    y0 = np.ascontiguousarray(y0, dtype=np.float64)
    if y0.ndim not in (1, 2) or y0.shape[-1] == 0:
        raise ValueError("y0 must be [n_states] or [members, n_states]")
    n_states = y0.shape[-1]
    r = _route(betas, matrix, b, norms, phis, start, stop, n_states, h, used_inputs, per_member=True)
    sizes = {f"betas[{k}]": c.shape[0] for k, c in enumerate(r['coeffs']) if c.ndim == 2}
    if y0.ndim == 2:
        sizes['y0'] = y0.shape[0]
    if len(set(sizes.values())) > 1:
        raise ValueError(f"the per-member arguments disagree on the number of members: {sizes}")
    n_members = next(iter(sizes.values())) if sizes else 1
    if n_members < 1:
        raise ValueError("an ensemble needs at least one member")
    cut = bounds_cut(n_members)
    if ReturnBounds and not 1 <= cut < n_members:
        raise ValueError(f"bounds (sorted[{cut}], sorted[{n_members} - {cut}]) need at least 2 members, there "
                         f"{'is' if n_members == 1 else 'are'} {n_members}: pass ReturnBounds=False")
    per_member = np.array([c.ndim == 2 for c in r['coeffs']], dtype=np.int32)
    ctx = _device_context(device)
    mean, bounds, members = ctx.gp_integrate_ensemble(
        n_members, n_states, r['n_other'], r['n_steps'], _pointer_array(r['coeffs']), per_member,
        _pointer_array(r['orders']), r['rows'], r['cols'], _pointer_array(r['sources']), r['n_src'],
        r['forcing'] if r['n_other'] else None, r['norms'], r['packed'], r['n_basis'], r['width'], float(h), y0,
        cut if ReturnBounds else None, bool(ReturnMembers))
    return (r['T'], mean) + ((bounds,) if ReturnBounds else ()) + ((members,) if ReturnMembers else ())

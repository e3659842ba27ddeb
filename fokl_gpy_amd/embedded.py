"""
Embedded GPs: K BSS-ANOVA GPs inside a user equation, sampled by Hamiltonian Monte Carlo, every chain at once on the
device.  (The reference's ``Experimental_Embedded_GPs``; its notebook ports by changing the import and ``jnp`` -> ``np``.)

    data_i = equation(GP_0(x_i), ..., GP_{K-1}(x_i); known columns c_i) + noise

THE EQUATION IS TRACED.  ``model.Processed_GPs[k]`` is a symbolic value; ``+ - * /``, unary minus, ``** constant`` and the
ufuncs ``np.exp / log / sqrt / square / reciprocal / negative`` applied to it record a tape.  A length-N array met in the
arithmetic becomes a *column* leaf (one per array object), a scalar a constant.  The result is a flat program in
single-assignment form with common subexpressions merged: leaves (GP k, column j, constant) and at most ``MAX_OPS``
operations.  Anything else raises a ``ValueError`` naming the operation at ``set_equation``, before any launch.

THE ALGORITHM.  Parameters q = (beta_0 .. beta_{K-1}, s), beta_k of length P = T + 1 (intercept first) for the T rows of
the shared interaction matrix, s = ln sigma^2, D = K P + 1.  With X the N x P basis matrix (all GPs read the same
inputs), g_k = X beta_k, r = equation(g; c), e = data - r:

    U(q)       = N/2 (ln 2 pi + s) + exp(-s)/2 sum_i e_i^2 + |beta|^2 / 2000 + (D - 1)/2 ln(2000 pi)
    dU/dbeta_k = -exp(-s) X^T (e * dr/dg_k) + beta_k / 1000             dU/ds = N/2 - exp(-s)/2 sum_i e_i^2

-- the reference's N(0, 1000 I) prior written as its logarithm (the reference takes log(pdf), which underflows for
large D); dr/dg_k per row comes from one reverse sweep over the tape.

  1. Transition (the reference's ``HMC``): momentum p_j = z_j / sqrt(w_j) with z standard normal and w the diagonal
     inverse mass; p -= eps/2 dU(q); ``leapfrog`` times { q += eps w p; p -= eps dU(q), the last one eps/2 }; accept if
     u < exp(U - U' + K - K') with K = sum_j p_j^2 w_j / 2.  U and dU of the current state are kept, so a transition is
     ``leapfrog`` passes over the rows.
  2. Step search (``find_reasonable_epsilon``) at a state: momentum r0; a trial is one leapfrog step of size eps.  eps = 1
     is halved until the trial's U and gradient are finite, AT MOST 60 TIMES (none: the chain ends with status
     'no step', its remaining draws are NaN; it never spins); log a = U - U' - (K' - K) of that trial, eps /= 2; then eps
     is doubled (a > 1/2) or halved until a crosses 1/2, at most 60 times.
  3. Adaptation (``full_sample``): after every 50 draws the window's acceptance count n scales eps by 0.5 (n < 15),
     0.8 (n < 30), 1.2 (30 < n <= 45) or 1.5 (n > 45).  Once, after draw 500, if at least 5 of the draws 401 .. 500 were
     accepted and every parameter's variance over those 100 states is finite and positive, the inverse mass becomes that
     variance and the step search runs again from the current state.
  4. Random numbers: Philox 4x32-10 keyed by (seed, chain) with counter (draw, purpose, index), one Box-Muller normal per
     counter (``csrc/fokl_philox.h``, compiled into the kernel and into the host entry ``fokl_embedded_rng``): the host
     statement and the kernel draw the same numbers.  numpy's global stream and the fit's MT19937 are not touched.

Deliberate deviations from the reference: the mass stays diagonal with M = 1 / variance (the reference mixes diag(cov)
with the diagonal of inv(cov)) and the kinetic energy of the step search uses it (the reference uses r . r); momentum and
the accept uniform use different random numbers (the reference reuses one subkey); the adaptation window is the 50 draws
just made and the variance is over the last 100 states, repeats included (the reference's slices are off by one and
de-duplicated); the step search tests for non-finite, not only infinite, values; JAX's threefry stream is not matched;
a spline piece is evaluated at the fit's local coordinate in [0, 1) (the reference's embedded module subtracts the
one-based piece index and so evaluates every piece one piece-width to the left of where ``fit`` does).
The start is all ones, as in the reference.

``full_sample`` / ``full_routine`` run on the device (``fokl_embedded_hmc``: one workgroup per chain, the whole chain in
one launch; without the library or a gfx950 device they raise, there is no host fallback).  ``full_sample_host`` /
``full_routine_host`` are the same algorithm in numpy with no device: the STATEMENT the kernel is tested against.  Sums
are ordered differently on the two sides, so values agree to rounding, and an accept decision within rounding of its
threshold may differ: compare chains whose accept flags agree.

``full_routine`` is the reference's forward selection: sub-stages enumerated as in ``fit`` (``engine.deal_indvec /
distinct_arrangements / advance_indvec``), the sub-stage's rows appended to the shared matrix, one sampling run per model,
ev = D ln N + 2 min U over all chains and draws, and the reference's stop rule on ``tolerance``.  (The reference counts
2 T + 1 parameters for its K = 2 case; D = K (T + 1) + 1 differs from that by a constant for K = 2, so the same models are
selected.)

Limits, checked before anything is launched and again by the native entry point: K <= 8 GPs, <= 16 columns, <= 32
operations, D <= 257, N (T + 1) <= 4 194 304 (all chains stream the same X from the last-level cache; a row-parallel
chain is not built), chains <= 4096.
"""
import numpy as np

from . import _capi, engine, getKernels
from .GP_Integrate import _device_context

MAX_GPS, MAX_COLUMNS, MAX_OPS, MAX_CONSTS, MAX_PARAMS = 8, 16, 32, 64, 257
MAX_VALUES = 4194304
MAX_CHAINS = 4096
SEARCH_CAP, WINDOW, MASS_DRAW, MASS_STATES, MASS_MOVED = 60, 50, 500, 100, 5
PRIOR_VARIANCE = 1000.0

ADD, SUB, MUL, DIV, NEG, EXP, LOG, SQRT, SQUARE, RECIP, POWC = range(11)
OP_NAMES = ('add', 'subtract', 'multiply', 'divide', 'negative', 'exp', 'log', 'sqrt', 'square', 'reciprocal', 'power')
KIND_SLOT, KIND_COLUMN, KIND_CONST = 0, 1, 2
PURPOSE_MOMENTUM, PURPOSE_ACCEPT, PURPOSE_SEARCH = 0, 1, 2
OK, NO_STEP = 0, 1
STATUS_TEXT = {OK: 'ok', NO_STEP: 'no step'}
KERNELS = ('Cubic Splines', 'Bernoulli Polynomials')

_UNARY_UFUNCS = {np.negative: NEG, np.exp: EXP, np.log: LOG, np.sqrt: SQRT, np.square: SQUARE, np.reciprocal: RECIP}
_BINARY_UFUNCS = {np.add: ADD, np.subtract: SUB, np.multiply: MUL, np.true_divide: DIV}


# ---------------------------------------------------------------------------------------------------------
# tracing
# ---------------------------------------------------------------------------------------------------------

class Tape:
    """A traced equation: ``ops`` int32 [n_ops, 3] rows (opcode, a, b) with operands (kind << 8) | index -- kind 0 a value
    (index < n_gps: that GP; n_gps + o: operation o), 1 a column, 2 a constant --, ``columns`` [n_cols, N], ``consts``
    and ``result`` (an operand of kind 0)."""

    def __init__(self, n_gps, rows):
        self.n_gps, self.rows = int(n_gps), int(rows)
        self.ops, self.columns, self.consts, self.result = [], [], [], None
        self._column_ids, self._seen = {}, {}

    def _refuse(self, what):
        raise ValueError(f"embedded equation: {what}")

    def operand(self, value, op):
        if isinstance(value, _Symbol):
            if value.tape is not self:
                self._refuse(f"'{op}' mixes values of two traces")
            return value.code
        if isinstance(value, (bool, np.bool_)):
            self._refuse(f"'{op}' with a boolean")
        arr = np.asarray(value)
        if arr.dtype == object or not (np.issubdtype(arr.dtype, np.number)) or np.iscomplexobj(arr):
            self._refuse(f"'{op}' with a value of type {type(value).__name__}")
        if arr.ndim == 0:
            c = float(arr)
            for i, have in enumerate(self.consts):
                if have == c and np.signbit(have) == np.signbit(c):
                    return (KIND_CONST << 8) | i
            if len(self.consts) >= MAX_CONSTS:
                self._refuse(f"'{op}' needs more than {MAX_CONSTS} constants")
            self.consts.append(c)
            return (KIND_CONST << 8) | (len(self.consts) - 1)
        if arr.shape != (self.rows,):
            self._refuse(f"'{op}' with an array of shape {arr.shape}: a column has one value per row, ({self.rows},)")
        key = id(value)
        if key not in self._column_ids:
            if len(self.columns) >= MAX_COLUMNS:
                self._refuse(f"'{op}' needs more than {MAX_COLUMNS} columns")
            self._column_ids[key] = (len(self.columns), value)          # (the array is kept alive with its id)
            self.columns.append(np.asarray(arr, dtype=np.float64))
        return (KIND_COLUMN << 8) | self._column_ids[key][0]

    def record(self, code, a, b=0):
        key = (code, a, b)
        if code in (ADD, MUL) and b < a:
            key = (code, b, a)
        if key not in self._seen:
            if len(self.ops) >= MAX_OPS:
                self._refuse(f"'{OP_NAMES[code]}' is operation {MAX_OPS + 1}: at most {MAX_OPS} (MAX_OPS)")
            self.ops.append(key)
            self._seen[key] = (KIND_SLOT << 8) | (self.n_gps + len(self.ops) - 1)
        return _Symbol(self, self._seen[key])

    def arrays(self):
        """(ops int32 [n_ops, 3], columns float64 [n_cols, N], consts float64) as the native entry point takes them."""
        return (np.array(self.ops, dtype=np.int32).reshape(-1, 3), np.array(self.columns, dtype=np.float64).reshape(-1, self.rows),
                np.array(self.consts, dtype=np.float64))

    def _fetch(self, code, values):
        kind, idx = code >> 8, code & 255
        return values[idx] if kind == KIND_SLOT else self.columns[idx] if kind == KIND_COLUMN else self.consts[idx]

    def forward(self, g):
        """Values of every slot for GP values g [n_gps, N]: a list, the GPs first."""
        values = [np.asarray(g[k], dtype=np.float64) for k in range(self.n_gps)]
        with np.errstate(all='ignore'):
            for code, ca, cb in self.ops:
                a = self._fetch(ca, values)
                if code <= DIV:
                    b = self._fetch(cb, values)
                    r = a + b if code == ADD else a - b if code == SUB else a * b if code == MUL else a / b
                elif code == NEG:
                    r = -a
                elif code == EXP:
                    r = np.exp(a)
                elif code == LOG:
                    r = np.log(a)
                elif code == SQRT:
                    r = np.sqrt(a)
                elif code == SQUARE:
                    r = a * a
                elif code == RECIP:
                    r = 1.0 / a
                else:
                    r = np.power(a, self.consts[cb & 255])
                values.append(r * np.ones(self.rows))
        return values

    def evaluate(self, g):
        """The equation's value [N] at GP values g [n_gps, N]."""
        return self.forward(g)[self.result & 255]

    def backward(self, values):
        """dr/dg_k [n_gps, N] from the values of ``forward``: one reverse sweep."""
        adj = [np.zeros(self.rows) for _ in values]
        adj[self.result & 255] = np.ones(self.rows)
        with np.errstate(all='ignore'):
            for o in range(len(self.ops) - 1, -1, -1):
                code, ca, cb = self.ops[o]
                slot_a, slot_b = (ca >> 8) == KIND_SLOT, code <= DIV and (cb >> 8) == KIND_SLOT
                if not (slot_a or slot_b):
                    continue
                bar, r = adj[self.n_gps + o], values[self.n_gps + o]
                da = db = 1.0
                if code == SUB:
                    db = -1.0
                elif code == MUL:
                    da, db = self._fetch(cb, values), self._fetch(ca, values)
                elif code == DIV:
                    b = self._fetch(cb, values)
                    da, db = 1.0 / b, -r / b
                elif code > DIV:
                    a = self._fetch(ca, values)
                    if code == NEG:
                        da = -1.0
                    elif code == EXP:
                        da = r
                    elif code == LOG:
                        da = 1.0 / a
                    elif code == SQRT:
                        da = 0.5 / r
                    elif code == SQUARE:
                        da = 2.0 * a
                    elif code == RECIP:
                        da = -(r * r)
                    else:
                        c = self.consts[cb & 255]
                        da = c * np.power(a, c - 1.0)
                if slot_a:
                    adj[ca & 255] = adj[ca & 255] + bar * da
                if slot_b:
                    adj[cb & 255] = adj[cb & 255] + bar * db
        return np.array(adj[:self.n_gps])


class _Symbol:
    """A value of the equation while it is traced."""
    __array_priority__ = 1000.0
    __hash__ = None

    def __init__(self, tape, code):
        self.tape, self.code = tape, code

    def _binary(self, code, other, swap=False):
        b = self.tape.operand(other, OP_NAMES[code])
        return self.tape.record(code, b, self.code) if swap else self.tape.record(code, self.code, b)

    def __add__(self, o): return self._binary(ADD, o)
    def __radd__(self, o): return self._binary(ADD, o, True)
    def __sub__(self, o): return self._binary(SUB, o)
    def __rsub__(self, o): return self._binary(SUB, o, True)
    def __mul__(self, o): return self._binary(MUL, o)
    def __rmul__(self, o): return self._binary(MUL, o, True)
    def __truediv__(self, o): return self._binary(DIV, o)
    def __rtruediv__(self, o): return self._binary(DIV, o, True)
    def __neg__(self): return self.tape.record(NEG, self.code)
    def __pos__(self): return self

    def __pow__(self, o):
        if isinstance(o, _Symbol) or np.ndim(o) != 0:
            self.tape._refuse("'power' with an exponent that is not a constant")
        return self.tape.record(POWC, self.code, self.tape.operand(o, 'power'))

    def __rpow__(self, o):
        self.tape._refuse("'power' with a GP in the exponent (write np.exp(GP * np.log(base)))")

    def _no(name):
        def refuse(self, *args, **kwargs):
            self.tape._refuse(f"'{name}' is not an operation a tape can hold")
        return refuse

    __lt__ = _no('less'); __le__ = _no('less_equal'); __gt__ = _no('greater'); __ge__ = _no('greater_equal')
    __eq__ = _no('equal'); __ne__ = _no('not_equal'); __bool__ = _no('bool'); __abs__ = _no('absolute')
    __floordiv__ = __rfloordiv__ = _no('floor_divide'); __mod__ = __rmod__ = _no('remainder')
    __matmul__ = __rmatmul__ = _no('matmul'); __getitem__ = _no('indexing'); __len__ = _no('len'); __iter__ = _no('iteration')
    __float__ = _no('float'); __int__ = _no('int')
    del _no

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        name = ufunc.__name__
        if method != '__call__' or kwargs:
            self.tape._refuse(f"'{name}' ({method}{', with keywords' if kwargs else ''}) is not an operation a tape can hold")
        if ufunc in _UNARY_UFUNCS:
            return self.tape.record(_UNARY_UFUNCS[ufunc], inputs[0].code)
        if ufunc in _BINARY_UFUNCS:
            code = _BINARY_UFUNCS[ufunc]
            a, b = (self.tape.operand(v, name) for v in inputs)
            return self.tape.record(code, a, b)
        if ufunc is np.power:
            if isinstance(inputs[0], _Symbol):
                return inputs[0].__pow__(inputs[1])
            return inputs[1].__rpow__(inputs[0])
        self.tape._refuse(f"'{name}' is not an operation a tape can hold (supported: + - * /, ** constant, negative, exp, "
                          f"log, sqrt, square, reciprocal)")


# ---------------------------------------------------------------------------------------------------------
# the statement: basis, potential, chain
# ---------------------------------------------------------------------------------------------------------

def _kernel_id(kernel):
    if kernel in (0, KERNELS[0]):
        return getKernels.KERNEL_SPLINES
    if kernel in (1, KERNELS[1]):
        return getKernels.KERNEL_BERNOULLI
    raise ValueError(f"The kernel {kernel} is not currently supported. Please select from the following: {list(KERNELS)}.")


def basis_matrix(inputs, mtx, phis, kernel='Cubic Splines'):
    """X [N, T + 1] of the interaction matrix ``mtx`` [T, M] at normalised inputs [N, M] (ones first), in numpy."""
    inputs = np.asarray(inputs, dtype=np.float64)
    mtx = np.atleast_2d(np.asarray(mtx)).astype(int)
    n, m = inputs.shape
    X = np.ones((n, mtx.shape[0] + 1))
    splines = _kernel_id(kernel) == getKernels.KERNEL_SPLINES
    if splines:
        pieces = len(phis[0][0])
        phind = np.ceil(inputs * pieces).astype(int)
        phind = phind + (phind == 0)
        phind = phind - 1
        xsm = pieces * inputs - phind                      # in [0, 1): the fit's local coordinate
        if phind.min() < 0 or phind.max() >= pieces:
            raise ValueError("Inputs are not normalized correctly: they must lie in [0, 1]")
    for t in range(mtx.shape[0]):
        for j in range(m):
            order = mtx[t, j]
            if order <= 0:
                continue
            if order > len(phis):
                raise ValueError(f"basis order {order} is outside the table of {len(phis)} basis functions")
            if splines:
                c = [np.asarray(phis[order - 1][k], dtype=np.float64)[phind[:, j]] for k in range(4)]
                X[:, t + 1] *= c[0] + c[1] * xsm[:, j] + c[2] * xsm[:, j] ** 2 + c[3] * xsm[:, j] ** 3
            else:
                c = phis[order - 1]
                X[:, t + 1] *= c[0] + sum(c[k] * inputs[:, j] ** k for k in range(1, len(c)))
    return X


def potential(q, X, tape, data):
    """(U, dU/dq) of the module docstring at q [D]."""
    n, P = X.shape
    K = tape.n_gps
    q = np.asarray(q, dtype=np.float64)
    B, s = q[:-1].reshape(K, P), q[-1]
    with np.errstate(all='ignore'):
        values = tape.forward(B @ X.T)
        e = data - values[tape.result & 255]
        sse, prec = float(e @ e), np.exp(-s)
        U = 0.5 * n * (np.log(2 * np.pi) + s) + 0.5 * prec * sse + float(q[:-1] @ q[:-1]) / (2 * PRIOR_VARIANCE) + \
            0.5 * (q.shape[0] - 1) * np.log(2 * PRIOR_VARIANCE * np.pi)
        W = tape.backward(values) * e
        grad = np.empty_like(q)
        grad[:-1] = (-prec * (W @ X) + B / PRIOR_VARIANCE).reshape(-1)
        grad[-1] = 0.5 * n - 0.5 * prec * sse
    return float(U), grad


def adapt_step(eps, accepted_in_window):
    """The step size after a 50-draw window with that many accepted draws."""
    n = int(accepted_in_window)
    return eps * (0.5 if n < 15 else 0.8 if n < 30 else 1.5 if n > 45 else 1.2 if n > 30 else 1.0)


def step_search(pot, q, U, grad, inv_mass, r0):
    """``find_reasonable_epsilon`` (docstring 2) -> the step, or 0.0 when no finite step exists.  pot(q) -> (U, grad)."""
    K0 = 0.5 * float(np.sum(r0 * r0 * inv_mass))
    eps, a, phase, halvings, moves = 1.0, 1.0, 0, 0, 0
    with np.errstate(all='ignore'):
        for _ in range(2 * SEARCH_CAP + 2):
            half = r0 - 0.5 * eps * grad
            Un, gn = pot(q + eps * inv_mass * half)
            rp = half - 0.5 * eps * gn
            finite = np.isfinite(Un) and np.isfinite(np.sum(np.abs(gn)))
            log_accept = U - Un - (0.5 * float(np.sum(rp * rp * inv_mass)) - K0)
            if phase == 0:
                if not finite:
                    halvings += 1
                    if halvings > SEARCH_CAP:
                        return 0.0
                    eps *= 0.5
                    continue
                a = 1.0 if log_accept > -np.log(2.0) else -1.0
                eps *= 0.5
                phase = 1
            if not (a * log_accept > -a * np.log(2.0)) or moves == SEARCH_CAP:
                break
            moves += 1
            eps = eps * 2.0 if a > 0 else eps * 0.5
    return eps if np.isfinite(eps) and eps > 0 else 0.0


def chain_host(pot, D, chain, draws, leapfrog=20, seed=0, q0=None, eps0=0.0, adapt=True, accept_script=None):
    """One chain of the statement; pot(q) -> (U, grad).  ``accept_script`` (a sequence of booleans) replaces the accept
    decisions, for tests of the bookkeeping.  Returns the dict ``DeviceContext.embedded_hmc`` returns, per chain."""
    rng = lambda draw, purpose, count: _capi.embedded_rng(seed, chain, draw, purpose, count)
    q = np.ones(D) if q0 is None else np.array(q0, dtype=np.float64)
    inv_mass = np.ones(D)
    states, Us = np.full((draws + 1, D), np.nan), np.full(draws + 1, np.nan)
    accepted, eps_hist = np.zeros(draws + 1, dtype=np.int32), np.full(draws // WINDOW, np.nan)
    U, grad = pot(q)
    states[0], Us[0] = q, U
    out = dict(states=states, potential=Us, accepted=accepted, eps_hist=eps_hist, inv_mass=inv_mass, grad0=grad.copy(),
               proposal=np.full(D + 1, np.nan), status=OK, mass_updated=False, eps_final=np.nan)
    eps = float(eps0) if eps0 > 0 else step_search(pot, q, U, grad, inv_mass, rng(0, PURPOSE_SEARCH, D) / np.sqrt(inv_mass))
    if not eps > 0:
        out['status'] = NO_STEP
        return out
    window = moved = 0
    with np.errstate(all='ignore'):
        for d in range(1, draws + 1):
            p0 = rng(d, PURPOSE_MOMENTUM, D) / np.sqrt(inv_mass)
            K0 = 0.5 * float(np.sum(p0 * p0 * inv_mass))
            qn, pn = q.copy(), p0 - 0.5 * eps * grad
            for l in range(leapfrog):
                qn = qn + eps * inv_mass * pn
                Un, gn = pot(qn)
                pn = pn - (0.5 * eps if l == leapfrog - 1 else eps) * gn
            K1 = 0.5 * float(np.sum(pn * pn * inv_mass))
            u = rng(d, PURPOSE_ACCEPT, 1)[0]
            accept = bool(u < np.exp(U - Un + K0 - K1)) if accept_script is None else bool(accept_script[d - 1])
            if d == draws:
                out['proposal'] = np.append(qn, Un)
            if accept:
                q, U, grad = qn, Un, gn
            states[d], Us[d], accepted[d] = q, U, accept
            window += accept
            if MASS_DRAW - MASS_STATES < d <= MASS_DRAW:
                moved += accept
            if d % WINDOW == 0:
                if adapt:
                    eps = adapt_step(eps, window)
                window = 0
                if adapt and d == MASS_DRAW and moved >= MASS_MOVED:
                    var = np.var(states[d - MASS_STATES + 1:d + 1], axis=0, ddof=1)
                    if np.all(np.isfinite(var) & (var > 0)):
                        inv_mass = var
                        out['inv_mass'], out['mass_updated'] = inv_mass, True
                        eps = step_search(pot, q, U, grad, inv_mass, rng(d, PURPOSE_SEARCH, D) / np.sqrt(inv_mass))
                eps_hist[d // WINDOW - 1] = eps if eps > 0 else np.nan
                if not eps > 0:
                    out['status'] = NO_STEP
                    return out
    out['eps_final'] = eps
    return out


def split_rhat(samples):
    """Split R-hat per parameter of samples [chains, n, D]: every chain is cut in two halves (Gelman et al., BDA3)."""
    samples = np.asarray(samples, dtype=np.float64)
    half = samples.shape[1] // 2
    if half < 2:
        return np.full(samples.shape[2], np.nan)
    parts = np.concatenate([samples[:, :half], samples[:, half:2 * half]], axis=0)
    with np.errstate(all='ignore'):
        within = parts.var(axis=1, ddof=1).mean(axis=0)
        between = half * parts.mean(axis=1).var(axis=0, ddof=1)
        return np.sqrt(((half - 1) / half * within + between / half) / within)


# ---------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------

class GP:
    """One unknown function of the equation (the reference's placeholder class; the model holds everything)."""


class _DeviceSession:
    """The dataset, the equation's columns and the column slots of one ``full_sample`` / ``full_routine`` on a context."""

    def __init__(self, model, tape, device):
        self.ctx = _device_context(device)
        kid = _kernel_id(model.kernel)
        packed, nb, width = getKernels.pack_phis(model.phis, kid)
        self.ctx.upload(model._inputs(), model._data(), kid, packed, nb, width)
        self.pool = engine.SlotPool(self.ctx, initial=64)
        self.tape = tape
        self.ops, columns, self.consts = tape.arrays()
        self.col_slots = self.pool.take(columns.shape[0])
        for slot, column in zip(self.col_slots, columns):
            self.ctx.write_slot(slot, column)
        self.term_slots = []

    def sample(self, mtx, chains, draws, leapfrog, seed, **extra):
        mtx = np.ascontiguousarray(np.atleast_2d(mtx), dtype=np.int32)
        if len(self.term_slots) < mtx.shape[0]:
            self.term_slots += self.pool.take(mtx.shape[0] - len(self.term_slots))
        slots = self.term_slots[:mtx.shape[0]]
        self.ctx.build_terms(mtx, slots)
        return self.ctx.embedded_hmc(self.tape.n_gps, [_capi.SLOT_ONES] + slots, self.col_slots, self.ops, self.consts,
                                     self.tape.result, chains, draws, leapfrog, seed, **extra)


class Embedded_GP_Model:
    """K GPs inside one equation (module docstring).  Set ``inputs`` [N, M] (already in [0, 1]), ``phis`` and ``data`` [N],
    then ``set_equation``; ``full_routine`` selects the shared interaction matrix, ``full_sample`` samples ``discmtx``."""

    def __init__(self, *GP, kernel='Cubic Splines'):
        if not 1 <= len(GP) <= MAX_GPS:
            raise ValueError(f"embedded model: {len(GP)} GPs, 1 to {MAX_GPS} are supported")
        _kernel_id(kernel)
        self.GP, self.kernel = GP, kernel
        self.discmtx = np.array([[1]])
        self.betas = np.ones(len(GP) * 2 + 1)
        self.inputs = self.phis = self.data = self.equation = self.tape = None
        self.mtx = self.evs = self.diagnostics = None
        self.Processed_GPs = None

    def _inputs(self):
        if self.inputs is None or self.data is None or self.phis is None:
            raise ValueError("embedded model: set model.inputs, model.phis and model.data first")
        x = np.asarray(self.inputs, dtype=np.float64)
        x = x[:, None] if x.ndim == 1 else x
        if x.ndim != 2 or x.shape[0] != np.size(self.data):
            raise ValueError("embedded model: inputs must be [N, M] and data [N]")
        if not (np.isfinite(x).all() and x.min() >= 0.0 and x.max() <= 1.0):
            raise ValueError("embedded model: inputs must be normalised to [0, 1]")
        return np.ascontiguousarray(x)

    def _data(self):
        return np.ascontiguousarray(np.reshape(np.asarray(self.data, dtype=np.float64), -1))

    def set_equation(self, equation_func):
        """Trace ``equation_func`` (no arguments; it reads ``model.Processed_GPs[k]``) into ``model.tape``; raises a
        ValueError that names the operation for anything a tape cannot hold."""
        n = self._inputs().shape[0]
        tape = Tape(len(self.GP), n)
        self.Processed_GPs = [_Symbol(tape, (KIND_SLOT << 8) | k) for k in range(len(self.GP))]
        result = equation_func()
        if not isinstance(result, _Symbol) or result.tape is not tape:
            raise ValueError("embedded equation: the result does not depend on a GP (read model.Processed_GPs[k] inside it)")
        tape.result = result.code
        self.equation, self.tape = equation_func, tape
        return tape

    def _check(self, mtx, chains, draws, leapfrog):
        if self.equation is None:
            raise ValueError("embedded model: call set_equation first")
        tape = self.set_equation(self.equation)                 # again: inputs or data may have been replaced
        mtx = np.atleast_2d(np.asarray(mtx)).astype(int)
        x = self._inputs()
        if mtx.shape[1] != x.shape[1]:
            raise ValueError(f"embedded model: the interaction matrix has {mtx.shape[1]} columns, the inputs {x.shape[1]}")
        if mtx.min() < 0 or mtx.max() > len(self.phis):
            raise ValueError(f"embedded model: basis orders must lie in 0 .. {len(self.phis)}")
        D = len(self.GP) * (mtx.shape[0] + 1) + 1
        if D > MAX_PARAMS:
            raise ValueError(f"embedded model: {len(self.GP)} GPs x {mtx.shape[0] + 1} coefficients + 1 = {D} parameters, at "
                             f"most {MAX_PARAMS}")
        if x.shape[0] * (mtx.shape[0] + 1) > MAX_VALUES:
            raise ValueError(f"embedded model: {x.shape[0]} rows x {mtx.shape[0] + 1} basis columns exceed {MAX_VALUES} values "
                             f"(32 MB, what every chain can stream from the last-level cache); a row-parallel chain is not built")
        if not 1 <= int(chains) <= MAX_CHAINS or int(draws) < 0 or int(leapfrog) < 1:
            raise ValueError(f"embedded model: chains in 1 .. {MAX_CHAINS}, draws >= 0 and leapfrog >= 1 expected")
        return tape, mtx, x, D

    def _finish(self, runs, mtx):
        """runs: per-chain dicts stacked -> the reference's return values, ``betas`` / ``diagnostics`` set."""
        samples, accepted, U = runs['states'], runs['accepted'].astype(bool), runs['potential']
        chains, rows = samples.shape[0], samples.shape[1]
        kept = samples[:, rows // 2:]
        self.diagnostics = dict(
            acceptance_rate=accepted[:, 1:].mean(axis=1) if rows > 1 else np.zeros(chains), step_size=runs['eps_final'],
            mass_updated=np.asarray(runs['mass_updated'], dtype=bool), status=np.asarray(runs['status']),
            status_text=[STATUS_TEXT[int(s)] for s in runs['status']], eps_history=runs['eps_hist'],
            inv_mass=runs['inv_mass'], rhat=split_rhat(kept) if chains > 1 else None)
        self.samples, self.discmtx = samples, np.array(mtx)
        self.betas = samples[0] if chains == 1 else samples
        if chains == 1:
            return samples[0], accepted[0], U[0]
        return samples, accepted, U

    def full_sample(self, draws, *, chains=1, seed=0, leapfrog=20, kernel=None, device=None, _session=None):
        """HMC for ``model.discmtx`` on the device -> (samples [draws + 1, D], accepted [draws + 1], U [draws + 1]); with
        ``chains > 1`` every array gets a leading chain axis.  ``model.diagnostics`` describes the run."""
        self.kernel = self.kernel if kernel is None else kernel
        tape, mtx, _, _ = self._check(self.discmtx, chains, draws, leapfrog)
        session = _session if _session is not None else _DeviceSession(self, tape, device)
        return self._finish(session.sample(mtx, chains, draws, leapfrog, seed), mtx)

    def host_potential(self, mtx=None):
        """pot(q) -> (U, gradient) of the statement for the interaction matrix ``mtx`` (default ``model.discmtx``)."""
        tape, mtx, x, _ = self._check(self.discmtx if mtx is None else mtx, 1, 0, 1)
        X, data = basis_matrix(x, mtx, self.phis, self.kernel), self._data()
        return lambda q: potential(q, X, tape, data)

    def full_sample_host(self, draws, *, chains=1, seed=0, leapfrog=20, kernel=None, q0=None, eps0=0.0, adapt=True):
        """``full_sample`` in numpy with no device: the statement."""
        self.kernel = self.kernel if kernel is None else kernel
        tape, mtx, x, D = self._check(self.discmtx, chains, draws, leapfrog)
        pot = self.host_potential(mtx)
        per = [chain_host(pot, D, c, draws, leapfrog, seed, None if q0 is None else np.asarray(q0)[c], eps0, adapt)
               for c in range(chains)]
        runs = {k: np.array([r[k] for r in per]) for k in per[0]}
        return self._finish(runs, mtx)

    def _routine(self, sample, draws, tolerance, way3):
        x = self._inputs()
        n, m = x.shape
        sett = 1 if m == 1 else 3 if way3 else 2
        if way3 and m < 3:
            raise ValueError("embedded model: way3 needs at least three inputs")
        damtx, evs, best = np.zeros((0, m), dtype=int), [], None
        ind, greater, finished = 1, 0, False
        while not finished:
            indvec = engine.deal_indvec(ind, m, sett)
            while True:
                damtx = np.vstack([damtx, engine.distinct_arrangements(indvec).astype(int)])
                D = len(self.GP) * (damtx.shape[0] + 1) + 1
                if D > MAX_PARAMS:
                    finished = True                             # the next model is beyond the kernel: keep the best so far
                    break
                self.discmtx = damtx
                samples, accepted, U = sample(draws)
                ev = D * np.log(n) + 2.0 * np.nanmin(U) if np.isfinite(U).any() else np.inf
                evs.append(ev)
                if len(evs) == 1 or ev < min(evs[:-1]):
                    best, greater = (samples, damtx.copy(), self.diagnostics), 1
                elif greater < tolerance:
                    greater += 1
                else:
                    finished = True
                    break
                if not engine.advance_indvec(indvec, m, way3):
                    break
            ind += 1
            if ind > len(self.phis):
                break
        if best is None:
            raise ValueError("embedded model: no model fits the kernel's limits")
        self.betas, self.mtx, self.diagnostics = best
        self.discmtx, self.evs = self.mtx, np.array(evs)
        self.samples = self.betas if self.betas.ndim == 3 else self.betas[None]
        return self.betas, self.mtx, self.evs

    def full_routine(self, draws, tolerance=0, way3=0, *, chains=1, seed=0, leapfrog=20, kernel=None, device=None):
        """Forward selection of the shared interaction matrix on the device -> (samples of the best model, its matrix,
        the ``evs`` trace).  The dataset, the columns and the tape go up once; every sub-stage model is one launch."""
        self.kernel = self.kernel if kernel is None else kernel
        tape, _, _, _ = self._check(np.zeros((1, self._inputs().shape[1]), dtype=int) + 1, chains, draws, leapfrog)
        session = _DeviceSession(self, tape, device)
        return self._routine(lambda d: self.full_sample(d, chains=chains, seed=seed, leapfrog=leapfrog, _session=session),
                             draws, tolerance, way3)

    def full_routine_host(self, draws, tolerance=0, way3=0, *, chains=1, seed=0, leapfrog=20, kernel=None):
        """``full_routine`` in numpy with no device: the statement."""
        self.kernel = self.kernel if kernel is None else kernel
        return self._routine(lambda d: self.full_sample_host(d, chains=chains, seed=seed, leapfrog=leapfrog), draws,
                             tolerance, way3)

    def evaluate(self, inputs, GP_number=0, draws=100, ReturnBounds=0, *, device=None):
        """GP ``GP_number``'s posterior over new normalised inputs [n, M] from the last ``draws`` states of every chain
        pooled, through the device prediction path -> mean [n] (and bounds [n, 2] with ``ReturnBounds``)."""
        if getattr(self, 'samples', None) is None:
            raise ValueError("embedded model: sample first (full_sample or full_routine)")
        if not 0 <= int(GP_number) < len(self.GP):
            raise ValueError(f"embedded model: GP_number must lie in 0 .. {len(self.GP) - 1}")
        x = np.asarray(inputs, dtype=np.float64)
        x = np.ascontiguousarray(x[:, None] if x.ndim == 1 else x)
        mtx = np.ascontiguousarray(np.atleast_2d(self.discmtx), dtype=np.int32)
        P = mtx.shape[0] + 1
        draws = min(int(draws), self.samples.shape[1])
        pooled = self.samples[:, self.samples.shape[1] - draws:, GP_number * P:(GP_number + 1) * P].reshape(-1, P)
        pooled = np.ascontiguousarray(pooled[np.isfinite(pooled).all(axis=1)])
        if pooled.shape[0] == 0:
            raise ValueError("embedded model: no finite draws to evaluate")
        ctx = _device_context(device)
        kid = _kernel_id(self.kernel)
        packed, nb, width = getKernels.pack_phis(self.phis, kid)
        ctx.upload(x, np.zeros(x.shape[0]), kid, packed, nb, width)
        slots = engine.SlotPool(ctx, initial=max(64, P + 2)).take(P - 1)
        ctx.build_terms(mtx, slots)
        slots = [_capi.SLOT_ONES] + slots
        if ReturnBounds:
            return ctx.predict(slots, pooled, int(np.floor(pooled.shape[0] * 0.025) + 1))
        return ctx.predict(slots, pooled)

"""An extended-precision reference of the embedded-GP potential for RAW tapes, the tapes the edge tests of the device
kernel use, and the CPU-side margins those tests assert (tests/test_embedded_reference.py, test_embedded_edges_gpu.py).

``reference_potential`` evaluates (U, dU/dq) of ``embedded``'s docstring in ``np.longdouble`` and shares no derivative code
shape with ``Tape.backward`` or the kernel: every slot carries a TANGENT per GP (forward mode), no adjoint is accumulated.
Its own guard is a central difference of its own U (``reference_self_check``).
"""
import numpy as np

from fokl_gpy_amd import _capi, embedded, engine, getKernels
from fokl_gpy_amd.embedded import ADD, SUB, MUL, DIV, NEG, EXP, LOG, SQRT, SQUARE, RECIP, POWC

L = np.longdouble
WIDE = 256                     # threads of the plan for up to 34 slots
NARROW = 128                   # ... and of the plan above that
SWITCH_SLOTS = 34              # the last slot count of the 256-thread plan
LDS_BUDGET = 160 * 1024


def S(i):
    return (embedded.KIND_SLOT << 8) | i


def C(j):
    return (embedded.KIND_COLUMN << 8) | j


def lds_bytes(n_slots, n_ops, threads):
    """The kernel's LDS request, recomputed from its layout: seven parameter rows of 257, the per-wave partials, 64
    constants, values and adjoints [slot][thread], the tape."""
    waves = threads // 64
    return 8 * (7 * 257 + waves + 257 * waves + 64 + 2 * n_slots * threads) + 12 * max(n_ops, 1)


class RawTape:
    """A hand-written tape over ``n_gps`` GPs: ops rows (opcode, a, b), constants, the result's slot."""

    def __init__(self, name, n_gps):
        self.name, self.n_gps, self.ops, self.consts, self.result = name, n_gps, [], [], None

    def K(self, c):
        """the operand of the constant c (a new entry every time: the entry point does not ask for merged constants)"""
        self.consts.append(float(c))
        return (embedded.KIND_CONST << 8) | (len(self.consts) - 1)

    def op(self, code, a, b=0):
        self.ops.append((code, a, b))
        return S(self.n_gps + len(self.ops) - 1)

    def power(self, a, c):
        return self.op(POWC, a, self.K(c))

    def done(self, result=None):
        self.result = S(self.n_slots - 1) if result is None else result
        return self

    @property
    def n_slots(self):
        return self.n_gps + len(self.ops)

    def padded(self, n_slots=SWITCH_SLOTS + 1):
        """the same equation with dead operations behind it (they read live values, nothing reads them) up to n_slots"""
        out = RawTape(self.name + '+dead', self.n_gps)
        out.ops, out.consts, out.result = list(self.ops), list(self.consts), self.result
        last = S(0)
        while out.n_slots < n_slots:
            o = len(out.ops)
            last = (out.op(MUL, last, S(o % out.n_slots)) if o % 3 == 0 else out.op(ADD, C(o % 3), last) if o % 3 == 1
                    else out.op(SUB, last, out.K(0.25 * o)))
        assert len(out.ops) <= embedded.MAX_OPS and len(out.consts) <= embedded.MAX_CONSTS
        return out

    def arrays(self):
        return (np.array(self.ops, dtype=np.int32).reshape(-1, 3), np.array(self.consts, dtype=np.float64))

    def host_tape(self, columns):
        """the ``embedded.Tape`` of the same program (the statement's potential runs on it)"""
        tape = embedded.Tape(self.n_gps, columns.shape[1])
        tape.ops, tape.columns, tape.consts, tape.result = list(self.ops), list(columns), list(self.consts), self.result
        return tape


def chain_tape(n_gps, n_ops):
    """Exactly n_ops cheap operations that stay finite and O(1) over ALL the GPs, with fan-out: a running value takes a GP,
    a column, a constant or an earlier value in turn, and is damped (bounded maps, halvings) so that it does not grow."""
    t = RawTape(f'chain K={n_gps} ops={n_ops}', n_gps)
    run, k, turn, kept = S(0), 1, 0, [S(0)]
    while len(t.ops) < n_ops:
        if len(t.ops) % 2 == 0:                                     # the next GP joins
            gp = S(k % n_gps)
            run = t.op(ADD, run, gp) if k % 3 == 0 else t.op(SUB, gp, run) if k % 3 == 1 else t.op(MUL, run, gp)
            k += 1
            continue
        step, turn = turn % 7, turn + 1
        if step == 0:
            run = t.op(MUL, C(turn % 3), run)
        elif step == 1:
            kept.append(run)
            run = t.op(SQUARE, run)
        elif step == 2:
            run = t.op(MUL, run, t.K(0.5))
        elif step == 3:
            run = t.op(ADD, run, kept[-1])                          # an earlier value, read again
        elif step == 4:
            run = t.op(DIV, run, C(turn % 3))
        elif step == 5 and len(t.ops) + 3 <= n_ops:
            run = t.op(EXP, t.op(NEG, t.op(SQUARE, run)))           # in (0, 1]
        else:
            run = t.op(SUB, t.K(0.7), run)
    assert len(t.ops) == n_ops and {S(g) for g in range(n_gps)} <= {x for row in t.ops for x in row[1:]}    # every GP is read
    return t.done()


def semantic_tapes():
    """One small tape over 3 GPs per (opcode, operand kinds, position) the entry point accepts, and the structural cases.
    Operations with a restricted domain read G0 + 3 (positive) or G0 - 3 (negative): to the kernel a GP and an operation's
    value are the same kind of operand, and 0.3 N(0, 1) coefficients keep |G0| below 3."""
    tapes = []

    def new(name):
        t = RawTape(name, 3)
        tapes.append(t)
        return t

    names = {ADD: 'add', SUB: 'sub', MUL: 'mul', DIV: 'div'}
    for code in (ADD, SUB, MUL, DIV):
        t = new(f'{names[code]}(slot, slot)')
        t.op(code, S(0), t.op(ADD, S(1), t.K(3.0)))
        t.done()
        t = new(f'{names[code]}(slot, column)')
        t.op(code, S(0), C(1))
        t.done()
        t = new(f'{names[code]}(column, slot)')
        t.op(code, C(1), t.op(ADD, S(0), t.K(3.0)))
        t.done()
        t = new(f'{names[code]}(slot, const)')
        t.op(code, S(1), t.K(1.7))
        t.done()
        t = new(f'{names[code]}(const, slot)')
        t.op(code, t.K(2.0), t.op(ADD, S(0), t.K(3.0)))
        t.done()
        if code != DIV:                                             # c - G on the GP itself; no GP is a divisor: it may vanish
            t = new(f'{names[code]}(const, GP)')
            t.op(code, t.K(2.0), S(1))
            t.done()
        t = new(f'{names[code]}(column, column)')
        t.op(MUL, t.op(code, C(0), C(2)), S(1))
        t.done()
        t = new(f'{names[code]}(const, column)')
        t.op(MUL, S(2), t.op(code, t.K(2.5), C(0)))
        t.done()
    unary = {NEG: 'neg', EXP: 'exp', LOG: 'log', SQRT: 'sqrt', SQUARE: 'square', RECIP: 'recip'}
    for code, name in unary.items():
        t = new(f'{name}(slot)')
        t.op(code, t.op(ADD, S(0), t.K(3.0)))
        t.done()
        t = new(f'{name}(column)')
        t.op(ADD, t.op(MUL, t.op(code, C(2)), S(0)), S(1))
        t.done()
    for code, name in ((NEG, 'neg'), (RECIP, 'recip'), (SQUARE, 'square')):
        t = new(f'{name}(negative slot)')
        t.op(code, t.op(SUB, S(0), t.K(3.0)))
        t.done()
    for c in (2.0, 3.0, 0.5, -1.0, 1.0, 0.0):
        t = new(f'pow(slot, {c})')
        t.op(ADD, t.power(t.op(ADD, S(0), t.K(3.0)), c), S(1))
        t.done()
    t = new('pow(negative slot, 3)')
    t.power(t.op(SUB, S(0), t.K(3.0)), 3.0)
    t.done()
    t = new('pow(column, 0.5)')
    t.op(MUL, t.power(C(1), 0.5), S(2))
    t.done()
    # structure
    t = new('a value read by three later operations')
    v = t.op(MUL, S(0), S(1))
    a, b, c = t.op(EXP, t.op(NEG, t.op(SQUARE, v))), t.op(MUL, v, C(0)), t.op(SUB, t.K(1.0), v)
    t.op(ADD, t.op(ADD, a, b), t.op(MUL, c, v))
    t.done()
    t = new('the result in the middle, live-looking operations behind it')
    r = t.op(MUL, t.op(ADD, S(0), S(1)), C(1))
    t.op(ADD, t.op(EXP, r), t.op(MUL, r, S(2)))
    t.op(SQUARE, S(0))
    t.done(r)
    t = new('a GP that no operation reads')
    t.op(MUL, t.op(SUB, S(0), C(0)), S(2))
    t.done()
    t = new('a leading block of GP-free operations')
    free = t.op(SQRT, t.op(ADD, t.op(MUL, C(0), C(1)), t.K(0.5)))
    free = t.op(DIV, t.op(EXP, t.op(NEG, free)), t.power(C(2), 2.0))
    t.op(SUB, t.op(MUL, free, S(1)), t.op(SQUARE, S(0)))
    t.done()
    t = new('the result is a GP')
    t.done(S(1))
    return tapes


class Problem:
    """Rows, basis, columns and data of one launch; the columns lie in [0.5, 1.5] and q0 = 0.3 N(0, 1) as in
    test_potential_and_gradient, so the arguments of the transcendental functions stay O(1)."""

    def __init__(self, N, P, kernel='Bernoulli Polynomials', seed=0):
        rng = np.random.default_rng(1000 * P + N + seed)
        self.x = rng.random((N, 2))
        self.columns = np.array([0.5 + rng.random(N) for _ in range(3)])
        self.data = rng.standard_normal(N)
        self.kernel = kernel
        self.phis = getKernels.sp500() if kernel == 'Cubic Splines' else getKernels.bernoulli()
        self.mtx = np.array([(1 + t % 5, (t // 5) % 4) for t in range(P - 1)], dtype=int).reshape(P - 1, 2)
        self.X = embedded.basis_matrix(self.x, self.mtx, self.phis, kernel)

    def launch(self, ctx, tape, q0, draws=0, leapfrog=20, seed=0, **kw):
        """the raw tape straight to ``DeviceContext.embedded_hmc`` over this problem's rows"""
        kid = embedded._kernel_id(self.kernel)
        packed, nb, width = getKernels.pack_phis(self.phis, kid)
        ctx.upload(self.x, self.data, kid, packed, nb, width)
        pool = engine.SlotPool(ctx, initial=64)
        col_slots = pool.take(self.columns.shape[0])
        for slot, column in zip(col_slots, self.columns):
            ctx.write_slot(slot, column)
        slots = pool.take(self.mtx.shape[0])
        if slots:
            ctx.build_terms(np.ascontiguousarray(self.mtx, dtype=np.int32), slots)
        ops, consts = tape.arrays()
        return ctx.embedded_hmc(tape.n_gps, [_capi.SLOT_ONES] + slots, col_slots, ops, consts, tape.result, q0.shape[0], draws,
                                leapfrog, seed, q0=q0, **kw)


def reference_forward(tape, g, columns):
    """(value [N], tangents [K, N] = d value / d g_k) of the tape's result at GP values g [K, N], in longdouble."""
    K, N = g.shape
    zero = np.zeros((K, N), dtype=L)
    slots = [(g[k], np.eye(K, dtype=L)[k][:, None] * np.ones(N, dtype=L)) for k in range(K)]

    def fetch(code):
        kind, idx = code >> 8, code & 255
        if kind == embedded.KIND_SLOT:
            return slots[idx]
        return ((columns[idx].astype(L) if kind == embedded.KIND_COLUMN else np.full(N, L(tape.consts[idx]))), zero)

    with np.errstate(all='ignore'):
        for code, ca, cb in tape.ops:
            a, ta = fetch(ca)
            if code in (ADD, SUB, MUL, DIV):
                b, tb = fetch(cb)
                if code == ADD:
                    v, t = a + b, ta + tb
                elif code == SUB:
                    v, t = a - b, ta - tb
                elif code == MUL:
                    v, t = a * b, ta * b + a * tb
                else:
                    v = a / b
                    t = (ta * b - a * tb) / (b * b)
            elif code == NEG:
                v, t = -a, -ta
            elif code == EXP:
                v = np.exp(a)
                t = ta * v
            elif code == LOG:
                v, t = np.log(a), ta / a
            elif code == SQRT:
                v = np.sqrt(a)
                t = ta / (v + v)
            elif code == SQUARE:
                v, t = a * a, (a + a) * ta
            elif code == RECIP:
                v, t = L(1) / a, -ta / (a * a)
            else:
                c = L(tape.consts[cb & 255])
                v = np.power(a, c)
                t = zero if c == 0 else ta if c == 1 else ta * (c * v / a)
            slots.append((v, t))
    return slots[tape.result & 255]


def reference_potential(q, X, tape, columns, data):
    """(U, dU/dq, e, dr/dg) of ``embedded``'s docstring for a raw tape, in longdouble with forward-mode derivatives."""
    N, P = X.shape
    K = tape.n_gps
    q, XL = np.asarray(q).astype(L), X.astype(L)
    B, s = q[:-1].reshape(K, P), q[-1]
    g = (B[:, None, :] * XL[None, :, :]).sum(axis=2)
    r, drdg = reference_forward(tape, g, columns)
    pi = 4 * np.arctan(L(1))
    with np.errstate(all='ignore'):
        e = data.astype(L) - r
        sse, prec = np.sum(e * e), np.exp(-s)
        D = q.shape[0]
        U = L(N) / 2 * (np.log(2 * pi) + s) + prec * sse / 2 + np.sum(q[:-1] * q[:-1]) / 2000 + L(D - 1) / 2 * np.log(2000 * pi)
        grad = np.empty(D, dtype=L)
        for k in range(K):
            grad[k * P:(k + 1) * P] = -prec * ((e * drdg[k])[:, None] * XL).sum(axis=0) + B[k] / 1000
        grad[-1] = L(N) / 2 - prec * sse / 2
    return U, grad, e, drdg


def reference_self_check(q, X, tape, columns, data, h=1e-6):
    """max_j |central difference of the reference's U - its gradient| / max_j |gradient|, every component, in longdouble.
    The truncation error is h^2 U''' / 6 ~ 1e-12 U''', the rounding error eps_L U / h ~ 1e-19 1e4 / 1e-6 = 1e-9 absolute:
    that is why the error is measured against the gradient's largest component and not against every component's own size
    (a prior-only component is ~3e-4)."""
    U, grad, _, _ = reference_potential(q, X, tape, columns, data)
    q = np.asarray(q).astype(L)
    fd = np.empty_like(grad)
    for j in range(q.shape[0]):
        step = np.zeros(q.shape[0], dtype=L)
        step[j] = L(h)
        fd[j] = (reference_potential(q + step, X, tape, columns, data)[0] -
                 reference_potential(q - step, X, tape, columns, data)[0]) / (2 * L(h))
    return float(np.max(np.abs(fd - grad)) / np.max(np.abs(grad)))


def term_scales(q, X, e, drdg):
    """(scale_U, scale_g [D]): the size of the terms U and dU/dq are summed from at q, for residuals e [N] and dr/dg
    [K, N] -- what a rounding-error bound on the device's sums is a multiple of."""
    q, e = np.asarray(q, dtype=np.float64), np.asarray(e, dtype=np.float64)
    N, P = X.shape
    D = q.shape[0]
    B = q[:-1].reshape((D - 1) // P, P)
    prec = np.exp(-q[-1])
    scale_U = 0.5 * N * (np.log(2 * np.pi) + abs(q[-1])) + 0.5 * prec * (e @ e) + 0.5 * (D - 1) * np.log(2000 * np.pi)
    W = np.abs(np.asarray(drdg, dtype=np.float64) * e)
    scale_g = np.append((prec * (W @ np.abs(X)) + np.abs(B) / 1000).reshape(-1), 0.5 * N + 0.5 * prec * (e @ e))
    return scale_U, scale_g


def assert_device_matches_reference(dev, q0, problem, tape, where):
    """potential[c, 0] and grad0[c] of a launch against the reference at q0[c], at the project's 1e-11 x term scale."""
    for c in range(q0.shape[0]):
        U, grad, e, drdg = reference_potential(q0[c], problem.X, tape, problem.columns, problem.data)
        assert np.isfinite(float(U)) and np.all(np.isfinite(grad.astype(np.float64))), (where, c)
        scale_U, scale_g = term_scales(q0[c], problem.X, e, drdg)
        err_U = abs(float(L(dev['potential'][c, 0]) - U))
        err_g = np.abs((dev['grad0'][c].astype(L) - grad).astype(np.float64))
        assert err_U <= 1e-11 * scale_U, (where, c, err_U / scale_U)
        assert np.all(err_g <= 1e-11 * scale_g + 1e-300), (where, c, float(np.max(err_g / (scale_g + 1e-300))))
        assert np.array_equal(dev['states'][c, 0], q0[c]), (where, c)
        assert dev['status'][c] == embedded.OK


def traced_model(equation, K, T, N, kernel='Bernoulli Polynomials', seed=0, data=None):
    """A traced model of K GPs over two inputs with T terms and N rows.  'cstr': two rate terms (2 GPs); 'wide': a sum of
    rate terms over all K GPs long enough for 35 slots and more; 'log': log(G0), finite only where G0 > 0; 'steep':
    exp(40 G0), which overflows a step away from the start; 'identity': G0."""
    rng = np.random.default_rng(1000 * K + 10 * T + N + seed)
    x = rng.random((N, 2))
    cols = [0.5 + rng.random(N) for _ in range(3)]
    model = embedded.Embedded_GP_Model(*[embedded.GP() for _ in range(K)], kernel=kernel)
    model.inputs, model.data = x, rng.standard_normal(N) if data is None else data(x, rng)
    model.phis = getKernels.sp500() if kernel == 'Cubic Splines' else getKernels.bernoulli()
    G = lambda k: model.Processed_GPs[k % K]
    if equation == 'cstr':
        eq = lambda: -(np.exp(-G(0)) * cols[0] * cols[1] - np.exp(-G(1)) * cols[2])
    elif equation == 'wide':
        if K >= 6:                                                  # 4 K - 1 operations
            eq = lambda: sum((cols[j % 3] * np.exp(-G(j)) for j in range(1, K)), cols[0] * np.exp(-G(0)))
        else:                                                       # 3 + 5 * 5 + 4 = 32 operations
            eq = lambda: sum((cols[j % 3] * np.exp(-(G(j) * (1.0 + 0.125 * j))) for j in range(1, 6)),
                             cols[0] * np.exp(-G(0))) + (np.square(G(1)) + 1.0) / cols[1]
    elif equation == 'log':
        eq = lambda: np.log(G(0))
    elif equation == 'steep':
        eq = lambda: np.exp(40.0 * G(0))
    else:
        eq = lambda: G(0)
    model.set_equation(eq)
    model.discmtx = np.array([(1 + t % 5, (t // 5) % 4) for t in range(T)], dtype=int).reshape(T, 2)
    return model


def launch_model(ctx, model, chains, draws, **kw):
    session = embedded._DeviceSession(model, model.tape, ctx)
    return session.sample(model.discmtx, chains, draws, kw.pop('leapfrog', 20), kw.pop('seed', 0), **kw)


# ---------------------------------------------------------------------------------------------------------
# margins of the statement's decisions, from host runs
# ---------------------------------------------------------------------------------------------------------

def accept_margins(pot, host, chain, leapfrog, seed, eps):
    """|u - exp(U - U' + K - K')| of every transition of a ``chain_host`` run with unit mass and the step ``eps`` (one
    value, or one per draw), replayed from the run's own states; the replay's decisions must be the run's."""
    draws, D = host['states'].shape[0] - 1, host['states'].shape[1]
    margins, steps = np.empty(draws), np.broadcast_to(np.asarray(eps, dtype=np.float64), (draws,))
    for d in range(1, draws + 1):
        eps = steps[d - 1]
        q, (U, grad) = host['states'][d - 1], pot(host['states'][d - 1])
        p0 = _capi.embedded_rng(seed, chain, d, embedded.PURPOSE_MOMENTUM, D)
        qn, pn = q.copy(), p0 - 0.5 * eps * grad
        for l in range(leapfrog):
            qn = qn + eps * pn
            Un, gn = pot(qn)
            pn = pn - (0.5 * eps if l == leapfrog - 1 else eps) * gn
        u = _capi.embedded_rng(seed, chain, d, embedded.PURPOSE_ACCEPT, 1)[0]
        with np.errstate(all='ignore'):
            threshold = np.exp(U - Un + 0.5 * float(p0 @ p0) - 0.5 * float(pn @ pn))
        assert bool(u < threshold) == bool(host['accepted'][d]), (chain, d)
        margins[d - 1] = abs(u - threshold) if np.isfinite(threshold) else np.inf
    return margins


def step_search_trace(pot, q, seed, chain):
    """``embedded.step_search`` at q with unit mass and the momentum of (seed, chain, draw 0) -> (the step, the
    log-acceptances of the finite trials in order, the number of non-finite trials, the largest finite |U'|).  The trials
    are recorded from the statement's own calls of ``pot``; their steps are recovered from the halving / doubling rule and
    checked against the recorded trial points, bit for bit."""
    q = np.asarray(q, dtype=np.float64)
    D = q.shape[0]
    U, grad = pot(q)
    r0 = _capi.embedded_rng(seed, chain, 0, embedded.PURPOSE_SEARCH, D)
    calls = []

    def recording(at):
        out = pot(at)
        calls.append((np.array(at), out[0], np.array(out[1])))
        return out

    inv_mass = np.ones(D)
    eps = embedded.step_search(recording, q, U, grad, inv_mass, r0)
    K0 = 0.5 * float(r0 @ r0)
    logs, nonfinite, largest = [], 0, 0.0
    for at, Un, gn in calls:
        # the trial's step: the power of two that reproduces the trial point
        found = [e for e in (2.0 ** j for j in range(-130, 131)) if np.array_equal(q + e * inv_mass * (r0 - 0.5 * e * grad), at)]
        assert len(found) == 1, found
        half = r0 - 0.5 * found[0] * grad
        rp = half - 0.5 * found[0] * gn
        with np.errstate(all='ignore'):
            if np.isfinite(Un) and np.isfinite(np.sum(np.abs(gn))):
                logs.append(U - Un - (0.5 * float(rp @ rp) - K0))
                largest = max(largest, abs(Un))
            else:
                assert not logs, "a non-finite trial after a finite one"
                nonfinite += 1
    return eps, np.array(logs), nonfinite, largest

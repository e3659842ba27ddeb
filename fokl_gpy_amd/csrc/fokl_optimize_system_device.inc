// Constrained optimisation over a SYSTEM of Bernoulli-polynomial models, per posterior draw (textually included by
// fokl_hip.hip behind fokl_optimize_core.inc and fokl_optimize_device.inc): one bound-constrained augmented-Lagrangian
// solve per (draw, start), all solves at once.  The algorithm is stated in numpy by fokl_gpy_amd/optimize.py
// (solve_system_host; the module docstring lists the steps); this file is that statement, one lane per solve.  Compiled
// under the tree's -ffp-contract=off.
//
// system_optimize_kernel: 64 solves per wavefront, one wavefront per workgroup, solve n = draw n / S, start n % S, as
// in model_optimize_kernel.  The evaluation of a model and the Newton step are fokl_optimize_core.inc's; what is here is
// the merit function around them and the multiplier / penalty updates.  What the problem is -- every model's term
// entries, its factors' (variable, order, shift, slope), the polynomial coefficients, the box, the constraint list -- is
// wave-uniform: scalar loads.  A draw's coefficients (the models' rows side by side) are scalar loads when S is a
// multiple of 64 (UNIFORM), per-lane loads otherwise.  A solve's own values sit in LDS as
// [item][lane], touched by their own lane only (no barriers):
//     3 F            phi, phi', phi'' of the distinct (input, order) factors of ONE model: the models are evaluated one
//                    after the other through the same rows, F = the largest model's count
//     n (n + 1) / 2  the Hessian of the merit function, factored in place
//     3 n            iterate, gradient, direction (the direction's rows hold a model's plain gradient while the
//                    derivatives are formed: the rank-one terms of its constraints need it whole)
//     2 K            every model's value and the sum of its terms' magnitudes at the point last evaluated
//     2 C            two multipliers per constraint (lower side; upper side or equality)
// rows of 512 bytes, at most 288 (144 KB).  An iteration is: one VALUE pass over the models (the constraints' weights
// need the values), the merit function from those values, one DERIVATIVE pass (each model's Hessian terms weighted by
// d merit / d output, its plain gradient, then the rank-one terms), the tests, and then per solve EITHER a multiplier /
// penalty update (a select; the iterate stays) OR the projected Newton step with the arc search (value passes only).
// Control flow is wave-uniform throughout.  No scratch.

namespace fokl {

constexpr int SYS_MAX_MODELS = 8;
constexpr int SYS_MAX_CONSTRAINTS = 2 * SYS_MAX_MODELS;               // a range and a tie per model
constexpr int SYS_INFEASIBLE = 4;
constexpr int64_t SYS_ITERATION_CAP = (int64_t)1 << 22;               // solves x max_iter asked of one launch
constexpr double SYS_RHO_START = 10.0, SYS_RHO_GROWTH = 10.0, SYS_RHO_MAX = 1e10;
constexpr double SYS_INNER_START = 1e-2, SYS_INNER_SHRINK = 1e-2, SYS_FEASIBLE_START = 1e-1, SYS_FEASIBLE_SHRINK = 1e-1;
// per model: entries, first entry, first slot, slots, first coefficient, its constraints [begin, end)
constexpr int SYS_MODEL_WORDS = 8;
constexpr int SYS_CON_WORDS = 5;      // per constraint: lo, hi, scale, tie offset, tie span

struct SysProblem {
    int n, n_models, n_con, n_hess, max_slots, width, max_iter, n_starts, n_coef, obj_model, obj_var;
    int64_t first, end;                                               // this launch solves [first, end)
    double sign, tol, ctol, obj_offset, obj_span;
};

struct SysData {                                                      // device pointers, the same for every solve
    const int *models, *slot_var, *slot_ord, *long_slots, *con_model, *con_var;
    const int4 *entries;
    const double *slot_map, *table, *box, *con_par;
};

struct SysCon {
    double psi, slope, curve, viol, measure, new_lo, new_hi;
};

// What the system kernel appends to a row of the trace (fokl_optimize_core.inc: OpTrace) behind OpTraceAt::of(n).end:
// ev [K], nz [K] and lam [2 C] at the entry, then rho, inner, target, viol, measure, update, good at the entry, then
// lam [2 C], rho, inner, target at the exit (after the update, if the iteration was one)
constexpr int SYS_TR_RHO = 0, SYS_TR_INNER = 1, SYS_TR_TARGET = 2, SYS_TR_VIOL = 3, SYS_TR_MEASURE = 4, SYS_TR_UPDATE = 5,
              SYS_TR_GOOD = 6, SYS_TR_HEAD = 7;

struct SysTraceAt {
    int ev, nz, lam_in, head, lam_out, tail, end;
    __host__ __device__ static SysTraceAt of(int n, int K, int C)
    {
        SysTraceAt a;
        a.ev = OpTraceAt::of(n).end;
        a.nz = a.ev + K;
        a.lam_in = a.nz + K;
        a.head = a.lam_in + 2 * C;
        a.lam_out = a.head + SYS_TR_HEAD;
        a.tail = a.lam_out + 2 * C;
        a.end = a.tail + 3;
        return a;
    }
};

// max(a, b) that keeps a NaN in either (numpy.maximum)
__device__ __forceinline__ double sys_max(double a, double b) { return a != a ? a : !(b <= a) ? b : a; }

// One constraint at residual r (optimize.py: _constraint).  par: lo, hi, scale (lo == hi: an equality, whose multiplier
// is the upper side's; -inf / +inf: no such side).  Which branch runs is wave-uniform.
__device__ __forceinline__ SysCon sys_constraint(const double *__restrict__ par, double r, double lam_lo, double lam_hi,
                                                 double rho)
{
    const double lo = par[0], hi = par[1], s = par[2];
    SysCon c;
    if (lo == hi) {
        const double cc = (r - lo) / s, w = lam_hi + rho * cc;
        c.psi = lam_hi * cc + 0.5 * rho * cc * cc;
        c.slope = w / s;
        c.curve = rho / (s * s);
        c.viol = c.measure = fabs(cc);
        c.new_lo = lam_lo;
        c.new_hi = w;
        return c;
    }
    c.psi = c.slope = c.curve = c.viol = c.measure = 0.0;
    c.new_lo = lam_lo;
    c.new_hi = lam_hi;
    if (hi < (double)INFINITY) {
        const double g = (r - hi) / s;
        c.new_hi = sys_max(0.0, lam_hi + rho * g);
        c.psi = c.psi + (c.new_hi * c.new_hi - lam_hi * lam_hi) / (2.0 * rho);
        c.slope = c.slope + c.new_hi / s;
        c.curve = c.curve + (c.new_hi > 0.0 ? rho / (s * s) : 0.0);
        c.viol = sys_max(c.viol, g);
        c.measure = sys_max(c.measure, fabs(sys_max(g, -lam_hi / rho)));
    }
    if (lo > -(double)INFINITY) {
        const double g = (lo - r) / s;
        c.new_lo = sys_max(0.0, lam_lo + rho * g);
        c.psi = c.psi + (c.new_lo * c.new_lo - lam_lo * lam_lo) / (2.0 * rho);
        c.slope = c.slope - c.new_lo / s;
        c.curve = c.curve + (c.new_lo > 0.0 ? rho / (s * s) : 0.0);
        c.viol = sys_max(c.viol, g);
        c.measure = sys_max(c.measure, fabs(sys_max(g, -lam_lo / rho)));
    }
    return c;
}

// Every model's value and sum of |terms| at the iterate (or the trial point) into ev, nz [K][64]
template <bool TRIAL>
__device__ __forceinline__ void sys_values(const SysProblem &p, const SysData &s, const double *__restrict__ coef,
                                           const double *xs, const double *dv, double alpha, double *fac, double *ev,
                                           double *nz)
{
    for (int k = 0; k < p.n_models; ++k) {
        const int *md = s.models + k * SYS_MODEL_WORDS;
        double e, noise;
        op_factors<0, TRIAL, true>(md[3], s.slot_var + md[2], s.slot_ord + md[2], s.slot_map + 2 * md[2], s.table, p.width,
                                   p.n, s.box, xs, dv, alpha, fac);
        op_terms<0>(md[0], s.slot_var + md[2], s.entries + md[1], s.long_slots, coef + md[4], 1.0, 0.0, fac, nullptr, nullptr,
                    e, noise);
        ev[k * OP_LANES] = e;
        nz[k * OP_LANES] = noise;
    }
}

// constraint i at the point ev was formed at
template <bool TRIAL>
__device__ __forceinline__ SysCon sys_constraint_at(const SysProblem &p, const SysData &s, int i, const double *xs,
                                                    const double *dv, double alpha, const double *ev, const double *nz,
                                                    const double *lam, double rho, double &reach)
{
    const int k = s.con_model[i], u = s.con_var[i];
    const double *par = s.con_par + i * SYS_CON_WORDS;
    double r = ev[k * OP_LANES];
    reach = nz[k * OP_LANES];
    if (u >= 0) {
        const double tied = par[3] + par[4] * op_point<TRIAL>(p.n, s.box, xs, dv, alpha, u);
        r = r - tied;
        reach = reach + fabs(tied);
    }
    return sys_constraint(par, r, lam[(2 * i) * OP_LANES], lam[(2 * i + 1) * OP_LANES], rho);
}

// The merit function L from the values, the sum of magnitudes its rounding allowance is taken from, the largest scaled
// violation and the largest convergence measure
template <bool TRIAL>
__device__ __forceinline__ void sys_merit(const SysProblem &p, const SysData &s, const double *xs, const double *dv,
                                          double alpha, const double *ev, const double *nz, const double *lam, double rho,
                                          double &L, double &size, double &viol, double &measure)
{
    if (p.obj_model >= 0) {
        L = p.sign * ev[p.obj_model * OP_LANES];
        size = nz[p.obj_model * OP_LANES];
    } else {
        const double value = p.obj_offset + p.obj_span * op_point<TRIAL>(p.n, s.box, xs, dv, alpha, p.obj_var);
        L = p.sign * value;
        size = fabs(value);
    }
    viol = measure = 0.0;
    for (int i = 0; i < p.n_con; ++i) {
        double reach;
        const SysCon c = sys_constraint_at<TRIAL>(p, s, i, xs, dv, alpha, ev, nz, lam, rho, reach);
        L = L + c.psi;
        size = size + fabs(c.slope) * reach;
        viol = sys_max(viol, c.viol);
        measure = sys_max(measure, c.measure);
    }
}

// Gradient g [n][64] and Hessian triangle H of L at the iterate; gm [n][64] is overwritten (a model's plain gradient)
__device__ __forceinline__ void sys_derivatives(const SysProblem &p, const SysData &s, const double *__restrict__ coef,
                                                const double *xs, const double *ev, const double *nz, const double *lam,
                                                double rho, double *fac, double *g, double *H, double *gm)
{
    const int n = p.n;
    for (int j = 0; j < n; ++j) g[j * OP_LANES] = 0.0;
    for (int h = 0; h < p.n_hess; ++h) H[h * OP_LANES] = 0.0;
    if (p.obj_var >= 0) g[p.obj_var * OP_LANES] += p.sign * p.obj_span;
    for (int k = 0; k < p.n_models; ++k) {
        const int *md = s.models + k * SYS_MODEL_WORDS;
        double weight = k == p.obj_model ? p.sign : 0.0, plain = 0.0, tie_slope = 0.0, tie_curve = 0.0;
        int tie = -1;
        for (int i = md[5]; i < md[6]; ++i) {
            double reach;
            const SysCon c = sys_constraint_at<false>(p, s, i, xs, gm, 0.0, ev, nz, lam, rho, reach);
            weight = weight + c.slope;
            if (s.con_var[i] < 0) {
                plain = plain + c.curve;
            } else {
                tie = i;
                tie_slope = c.slope;
                tie_curve = c.curve;
            }
        }
        for (int j = 0; j < n; ++j) gm[j * OP_LANES] = 0.0;
        double e, noise;
        op_factors<2, false, true>(md[3], s.slot_var + md[2], s.slot_ord + md[2], s.slot_map + 2 * md[2], s.table, p.width, n,
                                   s.box, xs, gm, 0.0, fac);
        op_terms<2>(md[0], s.slot_var + md[2], s.entries + md[1], s.long_slots, coef + md[4], 1.0, weight, fac, gm, H, e, noise);
        for (int j = 0; j < n; ++j) g[j * OP_LANES] += weight * gm[j * OP_LANES];
        if (md[6] > md[5] && (tie < 0 || md[6] - md[5] > 1))          // the rank-one terms of the range constraints
            for (int i = 0; i < n; ++i)
                for (int j = 0; j <= i; ++j)
                    H[(i * (i + 1) / 2 + j) * OP_LANES] += plain * gm[i * OP_LANES] * gm[j * OP_LANES];
        if (tie >= 0) {                                                // the tie's residual has -span at its variable
            const int u = s.con_var[tie];
            const double span = s.con_par[tie * SYS_CON_WORDS + 4];
            g[u * OP_LANES] += tie_slope * (-span);
            gm[u * OP_LANES] = gm[u * OP_LANES] - span;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j <= i; ++j)
                    H[(i * (i + 1) / 2 + j) * OP_LANES] += tie_curve * gm[i * OP_LANES] * gm[j * OP_LANES];
        }
    }
}

// box [2][n], starts [n_starts][n], betas [draws][n_coef]; x_out [solves][n], y_out [solves][K], mu_out [solves][C], the
// others [solves].  Lanes beyond p.end (the launch's last wavefront) solve nothing and write nothing.  TRACE: iteration
// trace_it of every solve also goes into its row of trace [solves][SysTraceAt::of(n, K, C).end]; the product
// instantiations never read those two arguments.
template <bool UNIFORM, bool TRACE>
__global__ __launch_bounds__(OP_LANES) void system_optimize_kernel(SysProblem p, SysData s,
                                                                   const double *__restrict__ starts,
                                                                   const double *__restrict__ betas,
                                                                   double *__restrict__ x_out, double *__restrict__ f_out,
                                                                   double *__restrict__ viol_out,
                                                                   double *__restrict__ y_out, double *__restrict__ mu_out,
                                                                   int *__restrict__ it_out, int *__restrict__ st_out,
                                                                   double *__restrict__ trace, int trace_it)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t solve = p.first + (int64_t)blockIdx.x * OP_LANES + lane;
    const bool real = solve < p.end;
    const int draw = real ? (int)(solve / p.n_starts) : 0, start = real ? (int)(solve % p.n_starts) : 0;
    const double *coef = betas + (size_t)(UNIFORM ? __builtin_amdgcn_readfirstlane(draw) : draw) * p.n_coef;
    const int n = p.n;
    const double *box = s.box;
    double *fac = lds + lane;                                          // [3 max_slots][64]
    double *H = fac + (size_t)3 * p.max_slots * OP_LANES;              // [n_hess][64]
    double *xs = H + (size_t)p.n_hess * OP_LANES;                      // [n][64] each: iterate, gradient, direction
    double *g = xs + n * OP_LANES;
    double *dv = g + n * OP_LANES;
    double *ev = dv + n * OP_LANES;                                    // [K][64] each: model values, sums of magnitudes
    double *nz = ev + p.n_models * OP_LANES;
    double *lam = nz + p.n_models * OP_LANES;                          // [2 C][64]
    unsigned fixed = 0;
    for (int j = 0; j < n; ++j) {
        xs[j * OP_LANES] = fmin(fmax(starts[(size_t)start * n + j], box[j]), box[n + j]);
        if (box[j] == box[n + j]) fixed |= 1u << j;
    }
    for (int i = 0; i < 2 * p.n_con; ++i) lam[i * OP_LANES] = 0.0;
    int status = real ? -1 : OP_CONVERGED, iterations = 0;             // -1: running
    bool steepest = false;
    double rho = SYS_RHO_START, inner = p.n_con ? fmax(p.tol, SYS_INNER_START) : p.tol;
    double target = fmax(p.ctol, SYS_FEASIBLE_START);
    OpTrace tr;
    SysTraceAt ts = {};
    if constexpr (TRACE) {
        tr.at = OpTraceAt::of(n);
        ts = SysTraceAt::of(n, p.n_models, p.n_con);
    }
    (void)ts;
    for (int it = 0; __any(status < 0); ++it) {
        double F, noise, viol, measure;
        const bool running = status < 0;
        if constexpr (TRACE) tr.row = real && it == trace_it ? trace + (size_t)solve * ts.end : nullptr;
        sys_values<false>(p, s, coef, xs, dv, 0.0, fac, ev, nz);
        sys_merit<false>(p, s, xs, dv, 0.0, ev, nz, lam, rho, F, noise, viol, measure);
        sys_derivatives(p, s, coef, xs, ev, nz, lam, rho, fac, g, H, dv);
        double pg;
        unsigned active;
        bool finite;
        op_survey(n, box, xs, g, F, fixed, finite, pg, active);
        const bool settled = pg <= p.tol && measure <= p.ctol;
        if (status < 0 && (!finite || settled || it == p.max_iter)) {
            status = !finite ? OP_NON_FINITE : settled ? OP_CONVERGED : OP_ITERATION_LIMIT;
            iterations = it;
        }
        if constexpr (TRACE) {
            op_trace_entry(tr, n, running, F, noise, pg, active, status, xs, g, H);
            if (tr.row && running) {
                for (int k = 0; k < p.n_models; ++k) {
                    tr.row[ts.ev + k] = ev[k * OP_LANES];
                    tr.row[ts.nz + k] = nz[k * OP_LANES];
                }
                for (int i = 0; i < 2 * p.n_con; ++i) tr.row[ts.lam_in + i] = tr.row[ts.lam_out + i] = lam[i * OP_LANES];
                tr.row[ts.head + SYS_TR_RHO] = tr.row[ts.tail] = rho;
                tr.row[ts.head + SYS_TR_INNER] = tr.row[ts.tail + 1] = inner;
                tr.row[ts.head + SYS_TR_TARGET] = tr.row[ts.tail + 2] = target;
                tr.row[ts.head + SYS_TR_VIOL] = viol;
                tr.row[ts.head + SYS_TR_MEASURE] = measure;
            }
        }
        if (!__any(status < 0)) break;
        // the inner problem is solved to its tolerance: multipliers or penalty move, the iterate does not
        bool update = status < 0 && pg <= inner;
        const bool capped = rho >= SYS_RHO_MAX;
        if (update && !(measure <= target) && capped && viol > p.ctol) {
            status = SYS_INFEASIBLE;
            iterations = it;
            update = false;
        }
        const bool good = measure <= target || capped;
        for (int i = 0; i < p.n_con; ++i) {
            double reach;
            const SysCon c = sys_constraint_at<false>(p, s, i, xs, dv, 0.0, ev, nz, lam, rho, reach);
            if (update && good) {
                lam[(2 * i) * OP_LANES] = c.new_lo;
                lam[(2 * i + 1) * OP_LANES] = c.new_hi;
            }
        }
        if (update && good) {
            inner = fmax(p.tol, SYS_INNER_SHRINK * inner);
            target = fmax(p.ctol, SYS_FEASIBLE_SHRINK * target);
        }
        if (update && !good) rho = fmin(SYS_RHO_GROWTH * rho, SYS_RHO_MAX);
        if constexpr (TRACE)
            if (tr.row && running) {
                tr.row[ts.head + SYS_TR_UPDATE] = update;
                tr.row[ts.head + SYS_TR_GOOD] = good;
                for (int i = 0; i < 2 * p.n_con; ++i) tr.row[ts.lam_out + i] = lam[i * OP_LANES];
                tr.row[ts.tail] = rho;
                tr.row[ts.tail + 1] = inner;
                tr.row[ts.tail + 2] = target;
            }
        const bool stalled = op_step<TRACE>(n, box, active, status < 0 && !update, F, noise, H, g, dv, xs, steepest, [&](double alpha) {
            double Ft, noise_t, viol_t, measure_t;
            sys_values<true>(p, s, coef, xs, dv, alpha, fac, ev, nz);
            sys_merit<true>(p, s, xs, dv, alpha, ev, nz, lam, rho, Ft, noise_t, viol_t, measure_t);
            return Ft;
        }, tr);
        if (stalled) {
            status = OP_STALLED;
            iterations = it;
        }
        if constexpr (TRACE) op_trace_exit(tr, n, xs, steepest, status);
    }
    // the results at the end point: objective, violation, every model's value, first-order multipliers
    double F, noise, viol, measure;
    sys_values<false>(p, s, coef, xs, dv, 0.0, fac, ev, nz);
    sys_merit<false>(p, s, xs, dv, 0.0, ev, nz, lam, rho, F, noise, viol, measure);
    if ((status == OP_ITERATION_LIMIT || status == OP_STALLED) && !(viol <= p.ctol)) status = SYS_INFEASIBLE;
    if (real) {
        for (int j = 0; j < n; ++j) x_out[(size_t)solve * n + j] = xs[j * OP_LANES];
        for (int k = 0; k < p.n_models; ++k) y_out[(size_t)solve * p.n_models + k] = ev[k * OP_LANES];
        f_out[solve] = p.obj_model >= 0 ? ev[p.obj_model * OP_LANES] : p.obj_offset + p.obj_span * xs[p.obj_var * OP_LANES];
        viol_out[solve] = viol;
        it_out[solve] = iterations;
        st_out[solve] = status;
    }
    for (int i = 0; i < p.n_con; ++i) {
        double reach;
        const SysCon c = sys_constraint_at<false>(p, s, i, xs, dv, 0.0, ev, nz, lam, rho, reach);
        if (real) mu_out[(size_t)solve * p.n_con + i] = c.slope;
    }
}

}  // namespace fokl

// fokl_system_optimize and fokl_system_optimize_trace (trace != nullptr: iteration trace_it into trace [N][stride])
static int system_optimize_run(const std::string &who, fokl_ctx *ctx, int n_vars, int n_models, const int32_t *n_inputs,
                               const int32_t *n_terms, const int32_t *mtx, const int32_t *var_of, const double *shift,
                               const double *slope, int n_draws, const double *betas, const double *table, int n_basis,
                               int width, const double *lo, const double *hi, int n_starts, const double *starts,
                               int obj_model, int obj_var, double obj_offset, double obj_span, double sign, int n_con,
                               const int32_t *con_model, const int32_t *con_var, const double *con_par, int max_iter,
                               double tol, double ctol, double *x, double *f, double *violation, double *y,
                               double *multipliers, int32_t *iterations, int32_t *status, int trace_it, double *trace)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->system_optimize_report, 0, sizeof ctx->system_optimize_report);
    if (n_vars <= 0 || n_models <= 0 || n_draws <= 0 || n_starts <= 0 || n_basis <= 0 || width <= 0 || n_con < 0 ||
        !n_inputs || !n_terms || !mtx || !var_of || !shift || !slope || !betas || !table || !lo || !hi || !starts ||
        (n_con > 0 && (!con_model || !con_var || !con_par || !multipliers)) || !x || !f || !violation || !y || !iterations ||
        !status)
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer or empty problem");
    if (n_vars > OP_MAX_INPUTS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_vars) +
                                           " decision variables, the kernel is built for at most " +
                                           std::to_string(OP_MAX_INPUTS));
    if (n_models > SYS_MAX_MODELS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_models) + " models, the kernel is built for at most " +
                                           std::to_string(SYS_MAX_MODELS));
    if (n_con > SYS_MAX_CONSTRAINTS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_con) + " constraints, at most a range and a tie per model");
    if ((obj_model >= 0) == (obj_var >= 0) || obj_model >= n_models || obj_var >= n_vars ||
        (obj_var >= 0 && !(std::fabs(obj_offset) <= DBL_MAX && std::fabs(obj_span) <= DBL_MAX)))
        return fail(ctx, FOKL_ERR_ARG, who + "the objective is one model's output or one decision variable");
    const std::string refusal = op_refusal(sign, max_iter >= 0 && tol >= 0.0 && ctol >= 0.0, "max_iter, tol and ctol", n_vars,
                                           lo, hi, "variable", n_draws, n_starts);
    if (!refusal.empty()) return fail(ctx, FOKL_ERR_ARG, who + refusal);

    // ---- the models as the kernel reads them: per model its distinct (variable, order) factors with the map they read,
    //      and the 16-byte term entries over the model's own slots ----
    std::vector<int32_t> models((size_t)n_models * SYS_MODEL_WORDS, 0);
    OpTables tables;
    int max_slots = 0, n_coef = 0, total_terms = 0;
    size_t in0 = 0, mtx0 = 0;
    for (int k = 0; k < n_models; ++k) {
        const int m = n_inputs[k], terms = n_terms[k];
        if (m <= 0 || m > n_vars || terms < 0)
            return fail(ctx, FOKL_ERR_ARG,
                        who + "model " + std::to_string(k) + " has no inputs, or more than there are variables");
        unsigned seen = 0;
        for (int j = 0; j < m; ++j) {
            const int v = var_of[in0 + j];
            if (v < 0 || v >= n_vars || ((seen >> v) & 1u))
                return fail(ctx, FOKL_ERR_ARG,
                            who + "model " + std::to_string(k) + " reads a variable outside the system, or twice");
            seen |= 1u << v;
            if (!(std::fabs(shift[in0 + j]) <= DBL_MAX) || !(std::fabs(slope[in0 + j]) <= DBL_MAX))
                return fail(ctx, FOKL_ERR_ARG, who + "model " + std::to_string(k) + " has a non-finite input map");
        }
        const int slot0 = (int)tables.slot_var.size(), entry0 = (int)tables.entries.size() / 4;
        if (!op_pack_model(mtx + mtx0, m, terms, var_of + in0, shift + in0, slope + in0, n_basis, width, tables))
            return fail(ctx, FOKL_ERR_ARG, who + "basis order outside the coefficient table");
        int32_t *md = models.data() + (size_t)k * SYS_MODEL_WORDS;
        md[0] = terms;
        md[1] = entry0;
        md[2] = slot0;
        md[3] = (int)tables.slot_var.size() - slot0;
        md[4] = n_coef;
        md[5] = md[6] = 0;
        max_slots = std::max(max_slots, md[3]);
        n_coef += terms + 1;
        total_terms += terms;
        in0 += (size_t)m;
        mtx0 += (size_t)terms * m;
    }
    // constraints: ordered by model, at most one range and then one tie per model
    for (int i = 0; i < n_con; ++i) {
        const int k = con_model[i], u = con_var[i];
        const double *par = con_par + (size_t)i * SYS_CON_WORDS;
        if (k < 0 || k >= n_models || u >= n_vars || (i > 0 && k < con_model[i - 1]) ||
            (i > 0 && k == con_model[i - 1] && (con_var[i - 1] >= 0 || u < 0)))
            return fail(ctx, FOKL_ERR_ARG, who + "constraints must be ordered by model, a model's range before its tie");
        if (!(par[0] <= par[1]) || !(par[2] > 0.0) || !(par[2] <= DBL_MAX) || par[0] == (double)INFINITY ||
            par[1] == -(double)INFINITY || (par[0] == -(double)INFINITY && par[1] == (double)INFINITY))
            return fail(ctx, FOKL_ERR_ARG, who + "constraint " + std::to_string(i) +
                                               " needs lo <= hi, one finite side and a positive scale");
        if (u >= 0 && !(par[0] == 0.0 && par[1] == 0.0 && std::fabs(par[3]) <= DBL_MAX && std::fabs(par[4]) <= DBL_MAX))
            return fail(ctx, FOKL_ERR_ARG,
                        who + "a tie is the equality output - (offset + span z) = 0 with finite offset and span");
        int32_t *md = models.data() + (size_t)k * SYS_MODEL_WORDS;
        if (md[6] == md[5]) md[5] = i;
        md[6] = i + 1;
    }
    SysProblem p{};
    p.n = n_vars;
    p.n_models = n_models;
    p.n_con = n_con;
    p.n_hess = n_vars * (n_vars + 1) / 2;
    p.max_slots = max_slots;
    p.width = width;
    p.max_iter = max_iter;
    p.n_starts = n_starts;
    p.n_coef = n_coef;
    p.obj_model = obj_model >= 0 ? obj_model : -1;
    p.obj_var = obj_var >= 0 ? obj_var : -1;
    p.sign = sign;
    p.tol = tol;
    p.ctol = ctol;
    p.obj_offset = obj_offset;
    p.obj_span = obj_span;
    const size_t lds_rows = (size_t)3 * max_slots + p.n_hess + (size_t)3 * n_vars + (size_t)2 * n_models + (size_t)2 * n_con;
    const size_t lds_bytes = lds_rows * OP_LANES * sizeof(double);
    if (lds_bytes > OP_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(max_slots) +
                                           " distinct (input, order) factors in the largest model, " +
                                           std::to_string(p.n_hess) + " Hessian entries, " + std::to_string(n_models) +
                                           " models and " + std::to_string(n_con) + " constraints need " +
                                           std::to_string(lds_rows) + " values per solve, a wavefront's LDS holds " +
                                           std::to_string(OP_LDS_BUDGET / (OP_LANES * sizeof(double))));

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    const size_t N = (size_t)n_draws * n_starts, n = (size_t)n_vars, K = (size_t)n_models, C = (size_t)n_con;
    std::vector<double> box(lo, lo + n);
    box.insert(box.end(), hi, hi + n);
    int *d_models = nullptr, *d_var = nullptr, *d_ord = nullptr, *d_long = nullptr, *d_cm = nullptr, *d_cv = nullptr;
    int *d_it = nullptr, *d_st = nullptr;
    int4 *d_entries = nullptr;
    double *d_map = nullptr, *d_table = nullptr, *d_box = nullptr, *d_par = nullptr, *d_starts = nullptr, *d_betas = nullptr;
    double *d_x = nullptr, *d_f = nullptr, *d_viol = nullptr, *d_y = nullptr, *d_mu = nullptr;
    HIP_TRY(ctx, buf.upload(&d_models, models.data(), models.size()));
    HIP_TRY(ctx, buf.upload(&d_var, tables.slot_var.data(), tables.slot_var.size()));
    HIP_TRY(ctx, buf.upload(&d_ord, tables.slot_ord.data(), tables.slot_ord.size()));
    HIP_TRY(ctx, buf.upload(&d_map, tables.slot_map.data(), tables.slot_map.size()));
    HIP_TRY(ctx, buf.upload(&d_long, tables.long_slots.data(), tables.long_slots.size()));
    HIP_TRY(ctx, buf.upload(&d_entries, tables.entries.data(), tables.entries.size() / 4));
    HIP_TRY(ctx, buf.upload(&d_table, table, (size_t)n_basis * width));
    HIP_TRY(ctx, buf.upload(&d_box, box.data(), box.size()));
    HIP_TRY(ctx, buf.upload(&d_cm, con_model, C));
    HIP_TRY(ctx, buf.upload(&d_cv, con_var, C));
    HIP_TRY(ctx, buf.upload(&d_par, con_par, C * SYS_CON_WORDS));
    HIP_TRY(ctx, buf.upload(&d_starts, starts, (size_t)n_starts * n));
    HIP_TRY(ctx, buf.upload(&d_betas, betas, (size_t)n_draws * n_coef));
    HIP_TRY(ctx, buf.get(&d_x, N * n));
    HIP_TRY(ctx, buf.get(&d_f, N));
    HIP_TRY(ctx, buf.get(&d_viol, N));
    HIP_TRY(ctx, buf.get(&d_y, N * K));
    HIP_TRY(ctx, buf.get(&d_mu, N * C));
    HIP_TRY(ctx, buf.get(&d_it, N));
    HIP_TRY(ctx, buf.get(&d_st, N));
    double *d_trace = nullptr;
    const size_t stride = (size_t)SysTraceAt::of(n_vars, n_models, n_con).end;
    if (trace) {                                                       // NaN everywhere, running = 0
        std::fill(trace, trace + N * stride, std::nan(""));
        for (size_t i = 0; i < N; ++i) trace[i * stride + OP_TR_RUNNING] = 0.0;
        HIP_TRY(ctx, buf.upload(&d_trace, trace, N * stride));
    }
    SysData s{};
    s.models = d_models;
    s.slot_var = d_var;
    s.slot_ord = d_ord;
    s.long_slots = d_long;
    s.con_model = d_cm;
    s.con_var = d_cv;
    s.entries = d_entries;
    s.slot_map = d_map;
    s.table = d_table;
    s.box = d_box;
    s.con_par = d_par;

    decltype(&system_optimize_kernel<true, false>) kernel = nullptr;
    bool raised = false;
    if (trace)
        HIP_TRY(ctx, op_pick(system_optimize_kernel<true, true>, system_optimize_kernel<false, true>, n_starts, lds_bytes,
                             &kernel, &raised));
    else
        HIP_TRY(ctx, op_pick(system_optimize_kernel<true, false>, system_optimize_kernel<false, false>, n_starts, lds_bytes,
                             &kernel, &raised));
    int launches = 0, first_grid = 0;
    // a launch is asked for at most SYS_ITERATION_CAP solve-iterations (solves x max_iter), in whole wavefronts
    const int64_t per_launch = std::max<int64_t>(OP_LANES, SYS_ITERATION_CAP / std::max(1, max_iter) / OP_LANES * OP_LANES);
    for (int64_t first = 0; first < (int64_t)N; first += per_launch) {
        p.first = first;
        p.end = std::min<int64_t>((int64_t)N, first + per_launch);
        const double count = (double)(p.end - p.first);
        const int grid = (int)((p.end - p.first + OP_LANES - 1) / OP_LANES);
        // per iterate and solve roughly: 50 flops and 9 + 18 LDS accesses per term over the value and derivative passes
        TimedRegion timed(ctx, FOKL_K_OPTIMIZE_SYSTEM, 8.0 * count * (n + K + C + 4.0) + 8.0 * (double)n_draws * n_coef,
                          count * 50.0 * std::max(1, total_terms));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(OP_LANES), lds_bytes, ctx->stream, p, s, d_starts, d_betas, d_x, d_f,
                           d_viol, d_y, d_mu, d_it, d_st, d_trace, trace_it);
        HIP_TRY(ctx, hipGetLastError());
        if (!launches++) first_grid = grid;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(x, d_x, N * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(f, d_f, N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(violation, d_viol, N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(y, d_y, N * K * sizeof(double), hipMemcpyDeviceToHost));
    if (C) HIP_TRY(ctx, hipMemcpy(multipliers, d_mu, N * C * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(iterations, d_it, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(status, d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (trace) HIP_TRY(ctx, hipMemcpy(trace, d_trace, N * stride * sizeof(double), hipMemcpyDeviceToHost));
    int64_t *rep = ctx->system_optimize_report;
    rep[0] = n_starts % OP_LANES == 0 ? FOKL_OPTIMIZE_UNIFORM : FOKL_OPTIMIZE_PER_LANE;
    rep[1] = first_grid;
    rep[2] = (int64_t)lds_bytes;
    rep[3] = raised;
    rep[4] = max_slots;
    rep[5] = (int64_t)tables.long_slots.size();
    rep[6] = (int64_t)N;
    rep[7] = launches;
    rep[8] = trace != nullptr;
    return FOKL_OK;
}

extern "C" int fokl_system_optimize(fokl_ctx *ctx, int n_vars, int n_models, const int32_t *n_inputs, const int32_t *n_terms,
                                    const int32_t *mtx, const int32_t *var_of, const double *shift, const double *slope,
                                    int n_draws, const double *betas, const double *table, int n_basis, int width,
                                    const double *lo, const double *hi, int n_starts, const double *starts, int obj_model,
                                    int obj_var, double obj_offset, double obj_span, double sign, int n_con,
                                    const int32_t *con_model, const int32_t *con_var, const double *con_par, int max_iter,
                                    double tol, double ctol, double *x, double *f, double *violation, double *y,
                                    double *multipliers, int32_t *iterations, int32_t *status)
{
    return system_optimize_run("fokl_system_optimize: ", ctx, n_vars, n_models, n_inputs, n_terms, mtx, var_of, shift, slope,
                               n_draws, betas, table, n_basis, width, lo, hi, n_starts, starts, obj_model, obj_var, obj_offset,
                               obj_span, sign, n_con, con_model, con_var, con_par, max_iter, tol, ctol, x, f, violation, y,
                               multipliers, iterations, status, 0, nullptr);
}

extern "C" int fokl_system_optimize_trace(fokl_ctx *ctx, int n_vars, int n_models, const int32_t *n_inputs,
                                          const int32_t *n_terms, const int32_t *mtx, const int32_t *var_of,
                                          const double *shift, const double *slope, int n_draws, const double *betas,
                                          const double *table, int n_basis, int width, const double *lo, const double *hi,
                                          int n_starts, const double *starts, int obj_model, int obj_var, double obj_offset,
                                          double obj_span, double sign, int n_con, const int32_t *con_model,
                                          const int32_t *con_var, const double *con_par, int max_iter, double tol,
                                          double ctol, double *x, double *f, double *violation, double *y,
                                          double *multipliers, int32_t *iterations, int32_t *status, int trace_iteration,
                                          double *trace)
{
    const std::string who = "fokl_system_optimize_trace: ";
    if (ctx) std::memset(ctx->system_optimize_report, 0, sizeof ctx->system_optimize_report);
    if (!trace || trace_iteration < 0) return fail(ctx, FOKL_ERR_ARG, who + "null trace or negative iteration");
    return system_optimize_run(who, ctx, n_vars, n_models, n_inputs, n_terms, mtx, var_of, shift, slope, n_draws, betas, table,
                               n_basis, width, lo, hi, n_starts, starts, obj_model, obj_var, obj_offset, obj_span, sign, n_con,
                               con_model, con_var, con_par, max_iter, tol, ctol, x, f, violation, y, multipliers, iterations,
                               status, trace_iteration, trace);
}

extern "C" int fokl_system_optimize_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_system_optimize_report: null argument");
    std::memcpy(out, ctx->system_optimize_report, sizeof ctx->system_optimize_report);
    return FOKL_OK;
}

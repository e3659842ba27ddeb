// Multistart box-constrained optimisation of a Bernoulli-polynomial model over its posterior (textually included by
// fokl_hip.hip behind fokl_optimize_core.inc): one projected Newton solve per (draw, start), all solves at once.  The
// algorithm is stated in numpy by fokl_gpy_amd/optimize.py (solve_host: the module docstring lists the steps); this file
// is that statement, one lane per solve, on the evaluation and the Newton step of fokl_optimize_core.inc.
//
// model_optimize_kernel: 64 solves per wavefront, one wavefront per workgroup -- what binds is the latency of a solve's
// dependent chain (a few dozen value / gradient / Hessian evaluations one after the other), so the wavefronts are spread
// over the CUs.  Solve n = draw n / S, start n % S: starts are the fast axis.  A draw's coefficients are read where they
// were uploaded, [draw][coefficient]: with S a multiple of 64 a wavefront belongs to one draw and they are scalar loads
// (the UNIFORM instantiation), otherwise each lane reads its draw's row (two rows per wavefront at S = 32, consecutive
// terms on one cache line).  An iterate costs ONE pass: value, gradient and Hessian of F = sign * model come out of the
// same term loop.  LDS per solve: 3 n_slots + m (m + 1) / 2 + 3 m rows of 512 bytes, 140 KB for 16 inputs with two orders
// each.  A solve that has stopped keeps its results in registers and idles until its wavefront is done.  No scratch.

namespace fokl {

struct OpProblem {
    int m, n_slots, n_entries, n_coef, n_hess, width, max_iter, n_starts;
    int64_t n_solves;
    double sign, tol;
};

// box [2][m] (lower bounds, upper bounds), starts [n_starts][m], betas [draws][n_coef]; x_out [n_solves][m], the others
// [n_solves].  Lanes beyond n_solves (the last wavefront) solve nothing and write nothing.  TRACE: iteration trace_it of
// every solve also goes into its row of trace [n_solves][OpTraceAt::of(m).end] (fokl_optimize_core.inc: OpTrace); the
// product instantiations never read those two arguments.
template <bool UNIFORM, bool TRACE>
__global__ __launch_bounds__(OP_LANES) void model_optimize_kernel(OpProblem p, const int *__restrict__ slot_src,
                                                                  const int *__restrict__ slot_ord,
                                                                  const int4 *__restrict__ entries,
                                                                  const int *__restrict__ long_slots,
                                                                  const double *__restrict__ table,
                                                                  const double *__restrict__ box,
                                                                  const double *__restrict__ starts,
                                                                  const double *__restrict__ betas,
                                                                  double *__restrict__ x_out, double *__restrict__ f_out,
                                                                  int *__restrict__ it_out, int *__restrict__ st_out,
                                                                  double *__restrict__ trace, int trace_it)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * OP_LANES + lane;
    const bool real = n < p.n_solves;
    const int draw = real ? (int)(n / p.n_starts) : 0, start = real ? (int)(n % p.n_starts) : 0;
    const double *coef = betas + (size_t)(UNIFORM ? __builtin_amdgcn_readfirstlane(draw) : draw) * p.n_coef;
    const int m = p.m;
    double *fac = lds + lane;                                          // [3 n_slots][64]
    double *H = fac + (size_t)3 * p.n_slots * OP_LANES;                // [n_hess][64]
    double *xs = H + (size_t)p.n_hess * OP_LANES;                      // [m][64] each: iterate, gradient, direction
    double *g = xs + m * OP_LANES;
    double *dv = g + m * OP_LANES;
    unsigned fixed = 0;
    for (int j = 0; j < m; ++j) {
        xs[j * OP_LANES] = fmin(fmax(starts[(size_t)start * m + j], box[j]), box[m + j]);
        if (box[j] == box[m + j]) fixed |= 1u << j;
    }
    int status = real ? -1 : OP_CONVERGED, iterations = 0;             // -1: running
    double f_end = NAN;
    bool steepest = false;
    OpTrace tr;
    if constexpr (TRACE) tr.at = OpTraceAt::of(m);
    for (int it = 0; __any(status < 0); ++it) {
        double F, noise, pg;
        unsigned active;
        bool finite;
        const bool running = status < 0;
        if constexpr (TRACE) tr.row = real && it == trace_it ? trace + (size_t)n * tr.at.end : nullptr;
        op_factors<2, false, false>(p.n_slots, slot_src, slot_ord, nullptr, table, p.width, m, box, xs, dv, 0.0, fac);
        for (int j = 0; j < m; ++j) g[j * OP_LANES] = 0.0;
        for (int h = 0; h < p.n_hess; ++h) H[h * OP_LANES] = 0.0;
        op_terms<2>(p.n_entries, slot_src, entries, long_slots, coef, p.sign, p.sign, fac, g, H, F, noise);
        op_survey(m, box, xs, g, F, fixed, finite, pg, active);
        if (status < 0 && (!finite || pg <= p.tol || it == p.max_iter)) {
            status = !finite ? OP_NON_FINITE : pg <= p.tol ? OP_CONVERGED : OP_ITERATION_LIMIT;
            iterations = it;
            f_end = F;
        }
        if constexpr (TRACE) op_trace_entry(tr, m, running, F, noise, pg, active, status, xs, g, H);
        if (!__any(status < 0)) break;
        const bool stalled = op_step<TRACE>(m, box, active, status < 0, F, noise, H, g, dv, xs, steepest, [&](double alpha) {
            double Ft, noise_t;
            op_factors<0, true, false>(p.n_slots, slot_src, slot_ord, nullptr, table, p.width, m, box, xs, dv, alpha, fac);
            op_terms<0>(p.n_entries, slot_src, entries, long_slots, coef, p.sign, p.sign, fac, g, H, Ft, noise_t);
            return Ft;
        }, tr);
        if (stalled) {
            status = OP_STALLED;
            iterations = it;
            f_end = F;
        }
        if constexpr (TRACE) op_trace_exit(tr, m, xs, steepest, status);
    }
    if (real) {
        for (int j = 0; j < m; ++j) x_out[(size_t)n * m + j] = xs[j * OP_LANES];
        f_out[n] = p.sign * f_end;
        it_out[n] = iterations;
        st_out[n] = status;
    }
}

}  // namespace fokl

// fokl_model_optimize and fokl_model_optimize_trace (trace != nullptr: iteration trace_it into trace [N][stride])
static int model_optimize_run(const std::string &who, fokl_ctx *ctx, int n_inputs, int n_terms, const int32_t *mtx,
                              int n_draws, const double *betas, const double *table, int n_basis, int width,
                              const double *lo, const double *hi, int n_starts, const double *starts, double sign,
                              int max_iter, double tol, double *x, double *f, int32_t *iterations, int32_t *status,
                              int trace_it, double *trace)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->optimize_report, 0, sizeof ctx->optimize_report);
    if (n_inputs <= 0 || n_terms < 0 || n_draws <= 0 || n_starts <= 0 || n_basis <= 0 || width <= 0 ||
        (n_terms > 0 && !mtx) || !betas || !table || !lo || !hi || !starts || !x || !f || !iterations || !status)
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer or empty problem");
    if (n_inputs > OP_MAX_INPUTS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_inputs) + " inputs, the kernel is built for at most " +
                                           std::to_string(OP_MAX_INPUTS));
    const std::string refusal = op_refusal(sign, max_iter >= 0 && tol >= 0.0, "max_iter and tol", n_inputs, lo, hi, "input",
                                           n_draws, n_starts);
    if (!refusal.empty()) return fail(ctx, FOKL_ERR_ARG, who + refusal);
    OpTables tables;
    if (!op_pack_model(mtx, n_inputs, n_terms, nullptr, nullptr, nullptr, n_basis, width, tables))
        return fail(ctx, FOKL_ERR_ARG, who + "basis order outside the coefficient table");
    OpProblem p{};
    p.m = n_inputs;
    p.n_slots = (int)tables.slot_var.size();
    p.n_entries = n_terms;
    p.n_coef = n_terms + 1;
    p.n_hess = n_inputs * (n_inputs + 1) / 2;
    p.width = width;
    p.max_iter = max_iter;
    p.n_starts = n_starts;
    p.n_solves = (int64_t)n_draws * n_starts;
    p.sign = sign;
    p.tol = tol;
    const size_t lds_rows = (size_t)3 * p.n_slots + p.n_hess + (size_t)3 * n_inputs;
    const size_t lds_bytes = lds_rows * OP_LANES * sizeof(double);
    if (lds_bytes > OP_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(p.n_slots) + " distinct (input, order) factors and " +
                                           std::to_string(p.n_hess) + " Hessian entries need " + std::to_string(lds_rows) +
                                           " values per solve, a wavefront's LDS holds " +
                                           std::to_string(OP_LDS_BUDGET / (OP_LANES * sizeof(double))));

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    const size_t N = (size_t)p.n_solves, m = (size_t)n_inputs;
    std::vector<double> box(lo, lo + m);
    box.insert(box.end(), hi, hi + m);
    int *d_src = nullptr, *d_ord = nullptr, *d_long = nullptr, *d_it = nullptr, *d_st = nullptr;
    int4 *d_entries = nullptr;
    double *d_table = nullptr, *d_box = nullptr, *d_starts = nullptr, *d_betas = nullptr, *d_x = nullptr, *d_f = nullptr;
    HIP_TRY(ctx, buf.upload(&d_src, tables.slot_var.data(), tables.slot_var.size()));
    HIP_TRY(ctx, buf.upload(&d_ord, tables.slot_ord.data(), tables.slot_ord.size()));
    HIP_TRY(ctx, buf.upload(&d_long, tables.long_slots.data(), tables.long_slots.size()));
    HIP_TRY(ctx, buf.upload(&d_entries, tables.entries.data(), (size_t)n_terms));
    HIP_TRY(ctx, buf.upload(&d_table, table, (size_t)n_basis * width));
    HIP_TRY(ctx, buf.upload(&d_box, box.data(), box.size()));
    HIP_TRY(ctx, buf.upload(&d_starts, starts, (size_t)n_starts * m));
    HIP_TRY(ctx, buf.upload(&d_betas, betas, (size_t)n_draws * p.n_coef));
    HIP_TRY(ctx, buf.get(&d_x, N * m));
    HIP_TRY(ctx, buf.get(&d_f, N));
    HIP_TRY(ctx, buf.get(&d_it, N));
    HIP_TRY(ctx, buf.get(&d_st, N));
    double *d_trace = nullptr;
    const size_t stride = (size_t)OpTraceAt::of(n_inputs).end;
    if (trace) {                                                       // NaN everywhere, running = 0
        std::fill(trace, trace + N * stride, std::nan(""));
        for (size_t i = 0; i < N; ++i) trace[i * stride + OP_TR_RUNNING] = 0.0;
        HIP_TRY(ctx, buf.upload(&d_trace, trace, N * stride));
    }

    decltype(&model_optimize_kernel<true, false>) kernel = nullptr;
    bool raised = false;
    if (trace)
        HIP_TRY(ctx, op_pick(model_optimize_kernel<true, true>, model_optimize_kernel<false, true>, n_starts, lds_bytes,
                             &kernel, &raised));
    else
        HIP_TRY(ctx, op_pick(model_optimize_kernel<true, false>, model_optimize_kernel<false, false>, n_starts, lds_bytes,
                             &kernel, &raised));
    const int grid = (int)((N + OP_LANES - 1) / OP_LANES);
    {
        // per iterate and solve roughly: 40 flops and 9 + 18 LDS accesses per term, 6 flops per factor and degree
        TimedRegion timed(ctx, FOKL_K_OPTIMIZE, 8.0 * (double)N * (m + 3.0) + 8.0 * (double)n_draws * p.n_coef,
                          (double)N * 40.0 * std::max(1, n_terms));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(OP_LANES), lds_bytes, ctx->stream, p, d_src, d_ord, d_entries, d_long,
                           d_table, d_box, d_starts, d_betas, d_x, d_f, d_it, d_st, d_trace, trace_it);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(x, d_x, N * m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(f, d_f, N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(iterations, d_it, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(status, d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (trace) HIP_TRY(ctx, hipMemcpy(trace, d_trace, N * stride * sizeof(double), hipMemcpyDeviceToHost));
    int64_t *rep = ctx->optimize_report;
    rep[0] = n_starts % OP_LANES == 0 ? FOKL_OPTIMIZE_UNIFORM : FOKL_OPTIMIZE_PER_LANE;
    rep[1] = grid;
    rep[2] = (int64_t)lds_bytes;
    rep[3] = raised;
    rep[4] = p.n_slots;
    rep[5] = (int64_t)tables.long_slots.size();
    rep[6] = p.n_solves;
    rep[7] = 1;
    rep[8] = trace != nullptr;
    return FOKL_OK;
}

extern "C" int fokl_model_optimize(fokl_ctx *ctx, int n_inputs, int n_terms, const int32_t *mtx, int n_draws,
                                   const double *betas, const double *table, int n_basis, int width, const double *lo,
                                   const double *hi, int n_starts, const double *starts, double sign, int max_iter,
                                   double tol, double *x, double *f, int32_t *iterations, int32_t *status)
{
    return model_optimize_run("fokl_model_optimize: ", ctx, n_inputs, n_terms, mtx, n_draws, betas, table, n_basis, width, lo,
                              hi, n_starts, starts, sign, max_iter, tol, x, f, iterations, status, 0, nullptr);
}

extern "C" int fokl_model_optimize_trace(fokl_ctx *ctx, int n_inputs, int n_terms, const int32_t *mtx, int n_draws,
                                         const double *betas, const double *table, int n_basis, int width,
                                         const double *lo, const double *hi, int n_starts, const double *starts,
                                         double sign, int max_iter, double tol, double *x, double *f,
                                         int32_t *iterations, int32_t *status, int trace_iteration, double *trace)
{
    const std::string who = "fokl_model_optimize_trace: ";
    if (ctx) std::memset(ctx->optimize_report, 0, sizeof ctx->optimize_report);
    if (!trace || trace_iteration < 0) return fail(ctx, FOKL_ERR_ARG, who + "null trace or negative iteration");
    return model_optimize_run(who, ctx, n_inputs, n_terms, mtx, n_draws, betas, table, n_basis, width, lo, hi, n_starts,
                              starts, sign, max_iter, tol, x, f, iterations, status, trace_iteration, trace);
}

extern "C" int fokl_optimize_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_optimize_report: null argument");
    std::memcpy(out, ctx->optimize_report, sizeof ctx->optimize_report);
    return FOKL_OK;
}

// dynamics.steady_states (textually included by fokl_hip.hip, after fokl_simulate_stiff_device.inc): where simulate's system
// comes to rest.  A damped Newton iteration on F(y) = 0 per member (operating point, posterior draw, start), F and its
// Jacobian being simulate_stiff's with a step of 1, clamps and slope rule included.
//
// The statement of the arithmetic is dynamics.steady_states_host (fokl_gpy_amd/dynamics.py, module docstring); this file
// follows it operation for operation: only + - * /, ceil, comparisons and integer bookkeeping, under the tree's
// -ffp-contract=off, so every member's record equals the host's bit for bit.
//
// steady_states_kernel<NS> has simulate_stiff_kernel's layout and LDS rows: one lane per member (draw e from start s is
// member e S + s), one wavefront per workgroup; blockIdx.y is the operating point, whose forcing factors the workgroup forms
// once.  stf_stage, stf_lu and stf_solve are used as they are; sim_stage forms the trial points' F.  W = -J (1 on the diagonal
// of a held row), the pivot rows and delta are per-lane registers; column d of J goes to device memory from the pass that
// forms it, so the last evaluation's J is what stays there.  Both loops are for loops with the plan's bounds (max_iter + 1
// evaluations, max_halvings + 1 trial points); a lane that has ended idles under the exec mask until the slowest lane of its
// wavefront is through.  No atomics, nothing shared between lanes: member m of a large run is member m run alone.
//
// The points are cut into launches of at most FOKL_STEADY_POINTS_PER_LAUNCH (default 4 096; and of what stays resident: one
// launch's records); a launch writes [point][item][member], the host reorders to [point][member][item].  The cut changes no bit.

namespace fokl {

constexpr int SDY_MAX_ITER = 200;
constexpr int SDY_MAX_HALVINGS = 30;

struct SteadyPlan {
    double ftol[SIM_MAX_STATES];
    int max_iter, max_halvings;
};

// dynamics._steady_ratio: max_j |F_j| / ftol_j by comparison from 0.0; a NaN is taken and kept
template <int NS>
__device__ __forceinline__ double sdy_ratio(const SteadyPlan &pl, const double (&F)[NS])
{
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double q = stf_abs(F[j]) / pl.ftol[j];
        r = (q > r || q != q) ? q : r;
    }
    return r;
}

// Points [q0, q0 + gridDim.y) of every member.  starts [NS][ld]; y_out [points][NS][ld], residual [points][ld], record
// [points][4][ld]: iterations, status, halvings, the held states as bits; jacobian [points][NS * NS][ld] or null.
// ld = members rounded up to 64 = 64 * gridDim.x: every lane owns a column of every buffer (the padding members have zero
// coefficients: F == 0, they end at their first evaluation).
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void steady_states_kernel(
    SimSystem sys, SteadyPlan pl, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const double *__restrict__ coef, const double *__restrict__ forcing,
    const double *__restrict__ starts, double *__restrict__ y_out, double *__restrict__ residual, int *__restrict__ record,
    double *__restrict__ jacobian, int64_t ld, int64_t q0)
{
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * SIM_LANES + lane;
    const size_t point = blockIdx.y;
    const int n_norm_state = sys.n_norm - sys.n_norm_forcing;
    double *fac = lds + lane;                                          // [1 + n_factors][64]: slot 0 is 1.0
    double *xn = lds + (size_t)(1 + sys.n_factors) * SIM_LANES + lane; // [n_norm - n_norm_forcing][64]
    double *cf = xn + n_norm_state * SIM_LANES;                        // [n_coef][64]
    double *tfac = cf + sys.n_coef * SIM_LANES;                        // [1 + n_factors][64]: the tangents of fac ...
    double *txn = tfac + (1 + sys.n_factors) * SIM_LANES;              // [n_norm - n_norm_forcing][64]: ... and of xn
    fac[0] = 1.0;
    for (int f = 0; f <= sys.n_forcing_factors; ++f) tfac[f * SIM_LANES] = 0.0;   // 1.0 and the forcing factors do not move with y
    for (int c = 0; c < sys.n_coef; ++c) cf[c * SIM_LANES] = coef[(size_t)c * ld + e];
    const double *frow = forcing + (size_t)(q0 + (int64_t)point) * sys.n_forcing_cols;   // the operating point: once
    bool forcing_acted = false;
    for (int f = 0; f < sys.n_forcing_factors; ++f) {
        const int n = tab.fac_norm[f];
        const double v = sim_clamp((frow[-(tab.norm_src[n] + 1)] - tab.norm_lo[n]) / tab.norm_span[n], forcing_acted);
        fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                       ? sim_cubic(tab.spline, tab.fac_row[f], v)
                                       : sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v);
    }
    double y[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = starts[(size_t)j * ld + e];
    double *jac = jacobian ? jacobian + point * (NS * NS) * ld + e : nullptr;
    int status = -1, iterations = 0, halvings = 0;
    unsigned wall = 0;
    double r = 0.0;
    for (int it = 0; it <= pl.max_iter && status < 0; ++it) {          // per lane: the others wait under the exec mask
        double W[NS][NS], F[NS], col[NS];
        unsigned moving = 0;                                           // bit k: J[k][d] != 0 for some d
#pragma unroll 1
        for (int d = 0; d < NS; ++d) {                                 // column d of J = dF/dy; F = F(y) from every pass
            stf_stage<NS>(sys, tab, xn, fac, txn, tfac, cf, y, d, F, col);
#pragma unroll
            for (int c = 0; c < NS; ++c)
                if (c == d) {                                          // wave-uniform
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        W[k][c] = -col[k];
                        if (jac) jac[(size_t)(k * NS + c) * ld] = col[k];
                    }
                }
#pragma unroll
            for (int k = 0; k < NS; ++k) moving |= (col[k] != 0 ? 1u : 0u) << k;
        }
        r = sdy_ratio<NS>(pl, F);
        wall = 0;
#pragma unroll
        for (int k = 0; k < NS; ++k) wall |= ((F[k] == 0 && !((moving >> k) & 1u)) ? 1u : 0u) << k;
        status = !(r < HUGE_VAL) ? 3 : r <= 1.0 ? 0 : it == pl.max_iter ? 1 : -1;
        if (status < 0) {
            int row[NS];
            double delta[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                W[k][k] = ((wall >> k) & 1u) ? 1.0 : W[k][k];
                delta[k] = F[k];
            }
            stf_lu<NS>(W, row);
            stf_solve<NS>(W, row, delta);
#pragma unroll
            for (int k = 0; k < NS; ++k) delta[k] = ((wall >> k) & 1u) ? 0.0 : delta[k];
            bool found = false;
            for (int b = 0; b <= pl.max_halvings && !found; ++b) {     // the first trial point that lowers r
                const double scale = sim_pow2_neg(b);
                double yt[NS], Ft[NS];
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double v = y[j] + delta[j] * scale;
                    v = v < sys.box_lo[j] ? sys.box_lo[j] : v;
                    v = v > sys.box_hi[j] ? sys.box_hi[j] : v;
                    yt[j] = v;
                }
                sim_stage<NS, SIM_LANES, true>(sys, tab, xn, fac, cf, yt, Ft, 1.0);
                const double rt = sdy_ratio<NS>(pl, Ft);
                if (rt < r) {
                    found = true;
                    halvings += b;
#pragma unroll
                    for (int j = 0; j < NS; ++j) y[j] = yt[j];
                }
            }
            if (found) {
                ++iterations;
            } else {
                status = 2;
                halvings += pl.max_halvings + 1;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) y_out[(point * NS + j) * ld + e] = y[j];
    residual[point * ld + e] = r;
    int *rec = record + point * 4 * ld + e;
    rec[0] = iterations;
    rec[ld] = status;
    rec[2 * ld] = halvings;
    rec[3 * ld] = (int)wall;
}

}  // namespace fokl

namespace {

// What fokl_steady_states refuses of n_steps = the operating points (sim_check's steps_test)
int sdy_points_fit(fokl_ctx *ctx, const std::string &who, const fokl_system &s)
{
    if (s.n_steps < 1) return fail(ctx, FOKL_ERR_ARG, who + "at least one operating point is needed (n_steps >= 1)");
    if (s.n_steps > (int64_t)1 << 30) return fail(ctx, FOKL_ERR_ARG, who + "too many operating points");
    return FOKL_OK;
}

}  // namespace

extern "C" int fokl_steady_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_steady_report: null argument");
    std::memcpy(out, ctx->steady_report, sizeof ctx->steady_report);
    return FOKL_OK;
}

extern "C" int fokl_steady_states(fokl_ctx *ctx, const fokl_system *system, const double *ftol, int max_iter, int max_halvings,
                                  double *y, double *residual, int32_t *iterations, int8_t *status, int32_t *halvings,
                                  uint8_t *on_wall, double *jacobian)
{
    const std::string who = "fokl_steady_states: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->steady_report, 0, sizeof ctx->steady_report);
    const bool own_ok = ftol && y && residual && iterations && status && halvings && on_wall;
    if (const int refused = sim_check(ctx, who, system, own_ok, sdy_points_fit)) return refused;
    const fokl_system &s = *system;
    if (max_iter < 1 || max_iter > SDY_MAX_ITER)
        return fail(ctx, FOKL_ERR_ARG, who + "max_iter must lie in 1.." + std::to_string(SDY_MAX_ITER));
    if (max_halvings < 0 || max_halvings > SDY_MAX_HALVINGS)
        return fail(ctx, FOKL_ERR_ARG, who + "max_halvings must lie in 0.." + std::to_string(SDY_MAX_HALVINGS));
    SteadyPlan pl{};
    for (int j = 0; j < s.n_states; ++j) {
        if (!(ftol[j] > 0) || !std::isfinite(ftol[j]))
            return fail(ctx, FOKL_ERR_ARG, who + "ftol must be positive and finite for every state");
        pl.ftol[j] = ftol[j];
    }
    pl.max_iter = max_iter;
    pl.max_halvings = max_halvings;
    SimSystem sys{};
    int n_bern_factors = 0;
    if (const int refused = sim_plan(ctx, who, s, sys, n_bern_factors)) return refused;
    // simulate_stiff's LDS rows and bound
    const size_t lds_rows = 2 * ((size_t)1 + s.n_factors + (s.n_norm - s.n_norm_forcing)) + s.n_coef;
    const size_t lds_bytes = lds_rows * SIM_LANES * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_rows) + " values per member in LDS (2 x (1 + "
                                           "factors + normalised states) + coefficients: simulate's and one set of tangent rows), "
                                           "a wavefront's " + std::to_string(SIM_LDS_BUDGET / 1024) + " KB hold " +
                                           std::to_string(SIM_LDS_BUDGET / (SIM_LANES * sizeof(double))));

    const int NS = s.n_states;
    const int64_t Q = s.n_steps;
    const size_t E = (size_t)s.n_members, ld = (E + SIM_LANES - 1) / SIM_LANES * SIM_LANES;
    const size_t jac_rows = jacobian ? (size_t)NS * NS : 0;
    // points per launch: what stays resident is one launch's records; FOKL_STEADY_POINTS_PER_LAUNCH overrides the bound
    // (tests: the cut changes no bit of the result)
    const size_t point_bytes = ld * ((NS + 1 + jac_rows) * sizeof(double) + 4 * sizeof(int));
    const int64_t resident = (int64_t)(((size_t)256 << 20) / point_bytes);
    const int64_t per_launch = std::max<int64_t>(
        1, std::min<int64_t>({(int64_t)env_int("FOKL_STEADY_POINTS_PER_LAUNCH", 4096), resident, (int64_t)65535, Q}));

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    SimTables tab{};
    int *d_record = nullptr;
    double *d_coef = nullptr, *d_forcing = nullptr, *d_starts = nullptr, *d_y = nullptr, *d_residual = nullptr, *d_jacobian = nullptr;
    HIP_TRY(ctx, sim_upload(buf, s, tab, d_forcing));
    HIP_TRY(ctx, sim_upload_padded(buf, &d_coef, s.coef, (size_t)s.n_coef, E, ld));
    HIP_TRY(ctx, sim_upload_padded(buf, &d_starts, s.y0, (size_t)NS, E, ld));
    HIP_TRY(ctx, buf.get(&d_y, (size_t)per_launch * NS * ld));
    HIP_TRY(ctx, buf.get(&d_residual, (size_t)per_launch * ld));
    HIP_TRY(ctx, buf.get(&d_record, (size_t)per_launch * 4 * ld));
    if (jacobian) HIP_TRY(ctx, buf.get(&d_jacobian, (size_t)per_launch * jac_rows * ld));
    std::vector<double> h_y((size_t)per_launch * NS * ld), h_residual((size_t)per_launch * ld),
        h_jacobian((size_t)per_launch * jac_rows * ld);
    std::vector<int> h_record((size_t)per_launch * 4 * ld);

    const int grid = (int)(ld / SIM_LANES);
    const auto launch = [&](int64_t q0, size_t points) {
        return sim_dispatch(NS, [&](auto ns) {
            const auto kernel = steady_states_kernel<decltype(ns)::value>;
            if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
            hipLaunchKernelGGL(kernel, dim3(grid, (unsigned)points), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, pl,
                               tab.norm_src, tab.norm_lo, tab.norm_span, tab.fac_norm, tab.fac_row, tab.fac_degree, tab.entries,
                               tab.spline, tab.bern, (const double *)d_coef, (const double *)d_forcing, (const double *)d_starts,
                               d_y, d_residual, d_record, d_jacobian, (int64_t)ld, q0);
            return hipGetLastError();
        });
    };
    int64_t launches = 0, sum_iterations = 0, sum_halvings = 0;
    for (int64_t q0 = 0; q0 < Q; q0 += per_launch) {
        const size_t points = (size_t)std::min<int64_t>(per_launch, Q - q0);
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)ld * points * (2.0 * NS + 1.0 + jac_rows), 0.0);
            HIP_TRY(ctx, launch(q0, points));
            ++launches;
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(h_y.data(), d_y, points * NS * ld * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(h_residual.data(), d_residual, points * ld * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(h_record.data(), d_record, points * 4 * ld * sizeof(int), hipMemcpyDeviceToHost));
        if (jacobian)
            HIP_TRY(ctx, hipMemcpy(h_jacobian.data(), d_jacobian, points * jac_rows * ld * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < points; ++p)                            // [point][item][ld] -> [point][member][item]
            for (size_t m = 0; m < E; ++m) {
                const size_t at = ((size_t)q0 + p) * E + m;
                const int *rec = h_record.data() + p * 4 * ld + m;
                for (int j = 0; j < NS; ++j) {
                    y[at * NS + j] = h_y[(p * NS + j) * ld + m];
                    on_wall[at * NS + j] = (uint8_t)((rec[3 * ld] >> j) & 1);
                }
                residual[at] = h_residual[p * ld + m];
                iterations[at] = rec[0];
                status[at] = (int8_t)rec[ld];
                halvings[at] = rec[2 * ld];
                sum_iterations += rec[0];
                sum_halvings += rec[2 * ld];
                for (size_t c = 0; c < jac_rows; ++c) jacobian[at * jac_rows + c] = h_jacobian[(p * jac_rows + c) * ld + m];
            }
    }
    int64_t *rep = ctx->steady_report;
    rep[0] = NS;
    rep[1] = s.n_members;
    rep[2] = (int64_t)grid * Q;
    rep[3] = (int64_t)lds_bytes;
    rep[4] = launches;
    rep[5] = Q;
    rep[6] = sum_iterations;
    rep[7] = sum_halvings;
    return FOKL_OK;
}

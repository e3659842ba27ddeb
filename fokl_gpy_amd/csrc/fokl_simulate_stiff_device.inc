// dynamics.simulate_stiff (textually included by fokl_hip.hip, after fokl_simulate_adaptive_device.inc): simulate's system
// under simulate_adaptive's per-lane dyadic step control, the step being the linearly implicit Rodas3 (four stages, order 3
// with an embedded order 2, gamma = 1 / 2, L-stable), so a member whose fast mode has decayed is no longer held to it.
//
// The statement of the arithmetic is dynamics.simulate_stiff_host (fokl_gpy_amd/dynamics.py, module docstring); this file
// follows it operation for operation: only + - * /, ceil, comparisons and integer bookkeeping, under the tree's
// -ffp-contract=off, so every member's trajectory and record equal the host's bit for bit.
//
// simulate_stiff_kernel<NS> has simulate_adaptive_kernel's layout: one lane per member, one wavefront per workgroup; the
// member's factors, normalised states and coefficients in LDS as [item][lane], touched by their own lane only; level,
// position and record per lane; a lane that has covered its output step idles under the exec mask.  New:
//   * stf_stage: ctl_stage (fokl_control_device.inc) with [coefficient][lane] coefficients and a step of 1.  It carries ONE
//     tangent direction, so the Jacobian is NS passes, column d from the pass with d y_j = (j == d), and the LDS addition is
//     one set of tangent rows: bytes = (2 (1 + factors + normalised states) + coefficients) x 64 lanes x 8.  The tangent rows
//     of slot 0 and of the forcing factors are zeroed once and never written again.  Every pass forms F(y) by the value
//     operations of sim_stage, so F(y) is the last pass's;
//   * W = (2 / g) I - J, its row exchanges and the four permuted solves live in registers: every index is a compile-time
//     constant after unrolling and a lane's pivot row acts through compare-and-select, never through an address (a register
//     array indexed by a per-lane value would go to scratch memory);
//   * the four solves share one loop body (the stage index is wave-uniform), as the stages of the explicit kernels do.
// One trial: NS tangent passes, two value passes (sim_stage with the lane's own step 1.0), one factorisation, four solves.
//
// The time axis is cut into launches of max(1, FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH >> max_halvings) output steps (default
// 65 536 substeps), so a launch's worst case -- every lane forced to the finest level -- is bounded.  The state and the
// per-lane values are carried in device memory between launches; the cut changes no bit.  No atomics: member e of a large run
// is member e run alone.  Points are written as [state][point][member] for ensemble_band_kernel / ensemble_transpose_kernel.

namespace fokl {

// a factor's value and slope as control's tangent pass forms them (defined in fokl_control_device.inc, further down)
__device__ __forceinline__ double ctl_cubic(const double *__restrict__ table, int row, double v, double &slope);
__device__ __forceinline__ double ctl_horner(const double *__restrict__ c, int degree, double v, double &slope);

__device__ __forceinline__ double stf_abs(double x) { return x < 0 ? -x : x; }

// F(at) with a step of 1 and column `dir` of its Jacobian (dir is wave-uniform); true if a clamp or the slope rule acted
template <int NS>
__device__ __forceinline__ bool stf_stage(const SimSystem &sys, const SimTables &tab, double *xn, double *fac, double *txn,
                                          double *tfac, const double *cf, const double (&at)[NS], int dir, double (&F)[NS],
                                          double (&col)[NS])
{
    bool acted = false;
#pragma unroll
    for (int j = 0; j < NS; ++j)
        for (int n = sys.norm_begin[j]; n < sys.norm_begin[j + 1]; ++n) {
            bool clamped = false;
            const double v = sim_clamp((at[j] - tab.norm_lo[n]) / tab.norm_span[n], clamped);
            xn[(n - sys.n_norm_forcing) * SIM_LANES] = v;
            txn[(n - sys.n_norm_forcing) * SIM_LANES] = clamped ? 0.0 : (j == dir ? 1.0 : 0.0) / tab.norm_span[n];
            acted = acted || clamped;
        }
    for (int f = sys.n_forcing_factors; f < sys.n_factors; ++f) {
        const int n = (tab.fac_norm[f] - sys.n_norm_forcing) * SIM_LANES;
        double slope;
        fac[(f + 1) * SIM_LANES] = f < sys.n_state_splines_end
                                       ? ctl_cubic(tab.spline, tab.fac_row[f], xn[n], slope)
                                       : ctl_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], xn[n], slope);
        tfac[(f + 1) * SIM_LANES] = slope * txn[n];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int4 *ent = tab.entries + sys.entry_begin[k];
        double delta = 0.0, phi = 1.0, tdelta = 0.0, tphi = 0.0;
        for (int t = 0; t < sys.entry_count[k]; ++t) {
            const int4 d = ent[t];
            tphi = tphi * fac[d.x * SIM_LANES] + phi * tfac[d.x * SIM_LANES];
            phi = phi * fac[d.x * SIM_LANES];
            tphi = tphi * fac[d.y * SIM_LANES] + phi * tfac[d.y * SIM_LANES];
            phi = phi * fac[d.y * SIM_LANES];
            tphi = tphi * fac[d.z * SIM_LANES] + phi * tfac[d.z * SIM_LANES];
            phi = phi * fac[d.z * SIM_LANES];
            const bool ends = d.w >= 0;                                 // wave-uniform
            const double c = cf[max(d.w, 0) * SIM_LANES];
            const double with = delta + c * phi, twith = tdelta + c * tphi;
            delta = ends ? with : delta;
            tdelta = ends ? twith : tdelta;
            phi = ends ? 1.0 : phi;
            tphi = ends ? 0.0 : tphi;
        }
        double s = delta + cf[sys.constant[k] * SIM_LANES], ts = tdelta;
        const bool outwards = (at[k] >= sys.box_hi[k] && s > 0) || (at[k] <= sys.box_lo[k] && s < 0);
        if (outwards) {
            s = 0;
            ts = 0;
        }
        acted = acted || outwards;
        F[k] = s;
        col[k] = ts;
    }
    return acted;
}

// dynamics.stiff_lu: W becomes U on and above the diagonal and the multipliers below it; row[c] is the row exchanged with
// row c in column c.  Returns the number of exchanges.
template <int NS>
__device__ __forceinline__ int stf_lu(double (&W)[NS][NS], int (&row)[NS])
{
    int exchanges = 0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        double best = stf_abs(W[c][c]);
        int pick = c;
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const double a = stf_abs(W[r][c]);
            const bool take = a > best;
            best = take ? a : best;
            pick = take ? r : pick;
        }
        row[c] = pick;
        exchanges += pick != c;
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const bool here = pick == r;
#pragma unroll
            for (int j = c; j < NS; ++j) {                             // the multipliers left of column c stay
                const double upper = W[c][j];
                W[c][j] = here ? W[r][j] : upper;
                W[r][j] = here ? upper : W[r][j];
            }
        }
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const double l = W[r][c] / W[c][c];
            W[r][c] = l;
#pragma unroll
            for (int j = c + 1; j < NS; ++j) W[r][j] = W[r][j] - l * W[c][j];
        }
    }
    return exchanges;
}

// dynamics.stiff_solve: b becomes W^-1 b
template <int NS>
__device__ __forceinline__ void stf_solve(const double (&W)[NS][NS], const int (&row)[NS], double (&b)[NS])
{
#pragma unroll
    for (int c = 0; c < NS; ++c) {
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const bool here = row[c] == r;
            const double upper = b[c];
            b[c] = here ? b[r] : upper;
            b[r] = here ? upper : b[r];
        }
#pragma unroll
        for (int r = c + 1; r < NS; ++r) b[r] = b[r] - W[r][c] * b[c];
    }
#pragma unroll
    for (int c = NS - 1; c >= 0; --c) {
        b[c] = b[c] / W[c][c];
#pragma unroll
        for (int r = 0; r < c; ++r) b[r] = b[r] - W[r][c] * b[c];
    }
}

// lane_i32 [4][ld]: level, first_saturation, first_unresolved, max_level; lane_i64 [3][ld]: steps, rejected, swaps;
// error [ld]; levels [all steps][ld] or null.  The rest as simulate_adaptive_kernel.
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void simulate_stiff_kernel(
    SimSystem sys, SimAdaptive ad, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const double *__restrict__ coef, const double *__restrict__ forcing,
    double *__restrict__ state, int *__restrict__ lane_i32, long long *__restrict__ lane_i64, double *__restrict__ error,
    signed char *__restrict__ levels, double *__restrict__ points, int64_t ld, int64_t t0, int steps, int chunk_points,
    int write_first)
{
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * SIM_LANES + lane;
    const int n_norm_state = sys.n_norm - sys.n_norm_forcing;
    double *fac = lds + lane;                                          // [1 + n_factors][64]: slot 0 is 1.0
    double *xn = lds + (size_t)(1 + sys.n_factors) * SIM_LANES + lane; // [n_norm - n_norm_forcing][64]
    double *cf = xn + n_norm_state * SIM_LANES;                        // [n_coef][64]
    double *tfac = cf + sys.n_coef * SIM_LANES;                        // [1 + n_factors][64]: the tangents of fac ...
    double *txn = tfac + (1 + sys.n_factors) * SIM_LANES;              // [n_norm - n_norm_forcing][64]: ... and of xn
    fac[0] = 1.0;
    for (int f = 0; f <= sys.n_forcing_factors; ++f) tfac[f * SIM_LANES] = 0.0;   // 1.0 and the forcing factors do not move with y
    for (int c = 0; c < sys.n_coef; ++c) cf[c * SIM_LANES] = coef[(size_t)c * ld + e];
    double y[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = state[(size_t)j * ld + e];
    int k = lane_i32[e], first = lane_i32[ld + e], unresolved = lane_i32[2 * ld + e], deepest = lane_i32[3 * ld + e];
    long long taken = lane_i64[e], rejected = lane_i64[ld + e], swaps = lane_i64[2 * ld + e];
    double worst = error[e];
    const int top = ad.max_halvings, full = 1 << top;
    if (write_first) {
#pragma unroll
        for (int j = 0; j < NS; ++j) points[(size_t)j * chunk_points * ld + e] = y[j];
    }
    double *out = points + (write_first ? ld : 0) + e;
    for (int s = 0; s < steps; ++s) {
        const double *frow = forcing + (size_t)(t0 + s) * sys.n_forcing_cols;   // the same row serves the whole step
        bool forcing_acted = false;
        for (int f = 0; f < sys.n_forcing_factors; ++f) {
            const int n = tab.fac_norm[f];
            const double v = sim_clamp((frow[-(tab.norm_src[n] + 1)] - tab.norm_lo[n]) / tab.norm_span[n], forcing_acted);
            fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                           ? sim_cubic(tab.spline, tab.fac_row[f], v)
                                           : sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v);
        }
        if (first < 0 && forcing_acted) first = (int)(t0 + s);
        int pos = 0, step_level = 0;
        while (pos < full) {                                           // per lane: the others wait under the exec mask
            const double g = sys.h * sim_pow2_neg(k);
            const double c2 = 2.0 / g, c4 = 4.0 / g, ig = 1.0 / g, c83 = 8.0 / 3.0;
            double W[NS][NS], F0[NS], col[NS];
            int row[NS];
            bool acted = false;
#pragma unroll 1
            for (int d = 0; d < NS; ++d) {                             // column d of J = dF/dy; F0 = F(y) from every pass
                const bool pass_acted = stf_stage<NS>(sys, tab, xn, fac, txn, tfac, cf, y, d, F0, col);
                acted = acted || pass_acted;
#pragma unroll
                for (int c = 0; c < NS; ++c)
                    if (c == d) {                                      // wave-uniform
#pragma unroll
                        for (int r = 0; r < NS; ++r) W[r][c] = r == c ? c2 - col[r] : -col[r];
                    }
            }
            const int exchanges = stf_lu<NS>(W, row);
            double K1[NS], K2[NS], K3[NS], b[NS], w[NS], Fw[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) K1[j] = K2[j] = K3[j] = w[j] = Fw[j] = 0.0;
            // st 0: K1 = solve(F0); 1: K2 = solve(F0 + c4 K1); 2: w = y + 2 K1, K3 = solve(F(w) + (K1 - K2) ig);
            // 3: w = w + K3, K4 = solve(F(w) + ((K1 - K2) - c83 K3) ig), left in b
#pragma unroll 1
            for (int st = 0; st < 4; ++st) {
                if (st >= 2) {
#pragma unroll
                    for (int j = 0; j < NS; ++j) w[j] = st == 2 ? y[j] + 2.0 * K1[j] : w[j] + K3[j];
                    const bool stage_acted = sim_stage<NS, SIM_LANES, true>(sys, tab, xn, fac, cf, w, Fw, 1.0);
                    acted = acted || stage_acted;
                }
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    b[j] = st == 0   ? F0[j]
                           : st == 1 ? F0[j] + c4 * K1[j]
                           : st == 2 ? Fw[j] + (K1[j] - K2[j]) * ig
                                     : Fw[j] + ((K1[j] - K2[j]) - c83 * K3[j]) * ig;
                stf_solve<NS>(W, row, b);
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    K1[j] = st == 0 ? b[j] : K1[j];
                    K2[j] = st == 1 ? b[j] : K2[j];
                    K3[j] = st == 2 ? b[j] : K3[j];
                }
            }
            bool ok = true, easy = true;
            double r = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                w[j] = w[j] + b[j];                                    // y_new = y4 + K4
                const double d = stf_abs(b[j]);
                const double a = stf_abs(y[j]), c = stf_abs(w[j]);
                const double sc = ad.atol[j] + ad.rtol * (c > a ? c : a);
                ok = ok && d <= sc;
                easy = easy && 16.0 * d <= sc;
                const double q = d / sc;
                r = q > r ? q : r;
            }
            if (ok || k == top) {
#pragma unroll
                for (int j = 0; j < NS; ++j) y[j] = w[j];
                pos += full >> k;
                ++taken;
                swaps += exchanges;
                if (!ok && unresolved < 0) unresolved = (int)(t0 + s);
                if (acted && first < 0) first = (int)(t0 + s);
                worst = r > worst ? r : worst;
                step_level = k > step_level ? k : step_level;
                if (easy && k > ad.min_halvings && (pos & ((1 << (top - k + 1)) - 1)) == 0) --k;
            } else {
                ++k;
                ++rejected;
            }
        }
        deepest = step_level > deepest ? step_level : deepest;
        if (levels) levels[(size_t)(t0 + s) * ld + e] = (signed char)step_level;
#pragma unroll
        for (int j = 0; j < NS; ++j) out[((size_t)j * chunk_points + s) * ld] = y[j];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) state[(size_t)j * ld + e] = y[j];
    lane_i32[e] = k;
    lane_i32[ld + e] = first;
    lane_i32[2 * ld + e] = unresolved;
    lane_i32[3 * ld + e] = deepest;
    lane_i64[e] = taken;
    lane_i64[ld + e] = rejected;
    lane_i64[2 * ld + e] = swaps;
    error[e] = worst;
}

}  // namespace fokl

namespace {

template <int NS>
hipError_t sim_stiff_launch(fokl_ctx *ctx, int grid, size_t lds_bytes, const SimSystem &sys, const SimAdaptive &ad,
                            const SimTables &tab, const double *coef, const double *forcing, double *state, int *lane_i32,
                            long long *lane_i64, double *error, signed char *levels, double *points, int64_t ld, int64_t t0,
                            int steps, int chunk_points, int write_first)
{
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(simulate_stiff_kernel<NS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)SIM_LDS_BUDGET);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(simulate_stiff_kernel<NS>, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, ad, tab.norm_src,
                       tab.norm_lo, tab.norm_span, tab.fac_norm, tab.fac_row, tab.fac_degree, tab.entries, tab.spline, tab.bern,
                       coef, forcing, state, lane_i32, lane_i64, error, levels, points, ld, t0, steps, chunk_points,
                       write_first);
    return hipGetLastError();
}

}  // namespace

extern "C" int fokl_simulate_stiff_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_simulate_stiff_report: null argument");
    std::memcpy(out, ctx->simulate_stiff_report, sizeof ctx->simulate_stiff_report);
    return FOKL_OK;
}

extern "C" int fokl_simulate_stiff(fokl_ctx *ctx, int n_members, int n_states, int64_t n_steps, double h, int n_forcing_cols,
                                   const double *forcing, int n_norm_forcing, int n_norm, const int32_t *norm_src,
                                   const double *norm_lo, const double *norm_span, int n_forcing_factors, int n_factors,
                                   const int32_t *fac_norm, const int32_t *fac_kind, const int32_t *fac_row,
                                   const int32_t *fac_degree, int n_spline_rows, const double *spline_table, int n_bern_rows,
                                   const double *bern_table, int n_entries, const int32_t *entries, const int32_t *entry_begin,
                                   const int32_t *entry_count, const int32_t *constant, int n_coef, const double *coef,
                                   const double *y0, const double *box, int cut, double rtol, const double *atol,
                                   int min_halvings, int max_halvings, double *mean, double *bounds, double *members,
                                   int32_t *first_saturation, int64_t *taken, int64_t *rejected, int64_t *swaps,
                                   int32_t *max_level, double *error, int32_t *first_unresolved, int8_t *levels)
{
    const std::string who = "fokl_simulate_stiff: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->simulate_stiff_report, 0, sizeof ctx->simulate_stiff_report);
    if (n_members <= 0 || n_states <= 0 || n_steps < 0 || n_forcing_cols < 0 || n_norm_forcing < 0 || n_norm < n_norm_forcing ||
        n_forcing_factors < 0 || n_factors < n_forcing_factors || n_spline_rows < 0 || n_bern_rows < 0 || n_entries < 0 ||
        n_coef < n_states || !entry_begin || !entry_count || !constant || !coef || !y0 || !box || !mean || !first_saturation ||
        !atol || !taken || !rejected || !swaps || !max_level || !error || !first_unresolved ||
        (n_norm > 0 && (!norm_src || !norm_lo || !norm_span)) || (n_factors > 0 && (!fac_norm || !fac_kind || !fac_row || !fac_degree)) ||
        (n_entries > 0 && !entries) || (n_spline_rows > 0 && !spline_table) || (n_bern_rows > 0 && !bern_table) ||
        (n_forcing_cols > 0 && n_steps > 0 && !forcing))
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer, negative size or empty system");
    if (n_states > SIM_MAX_STATES)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_states) + " states, the kernel is built for at most " +
                                           std::to_string(SIM_MAX_STATES));
    if (n_steps + 1 > (int64_t)1 << 30) return fail(ctx, FOKL_ERR_ARG, who + "too many steps");
    if (!(h > 0) || !std::isfinite(h)) return fail(ctx, FOKL_ERR_ARG, who + "h must be positive and finite");
    if (bounds && (cut < 1 || cut >= n_members)) return fail(ctx, FOKL_ERR_ARG, who + "bounds need 1 <= cut < n_members");
    if (bounds && n_members > GI_BAND_MAX_MEMBERS)
        return fail(ctx, FOKL_ERR_ARG, who + "bounds are formed over at most " + std::to_string(GI_BAND_MAX_MEMBERS) +
                                           " members (mean and members have no limit)");
    if (!(rtol >= 0) || !std::isfinite(rtol)) return fail(ctx, FOKL_ERR_ARG, who + "rtol must be finite and not negative");
    SimAdaptive ad{};
    ad.rtol = rtol;
    for (int j = 0; j < n_states; ++j) {
        if (!(atol[j] >= 0) || !std::isfinite(atol[j]))
            return fail(ctx, FOKL_ERR_ARG, who + "atol must be finite and not negative for every state");
        if (rtol == 0 && atol[j] == 0)
            return fail(ctx, FOKL_ERR_ARG, who + "rtol == 0 needs a positive atol for every state");
        ad.atol[j] = atol[j];
    }
    if (min_halvings < 0 || max_halvings < min_halvings || max_halvings > SIM_MAX_HALVINGS)
        return fail(ctx, FOKL_ERR_ARG, who + "the levels need 0 <= min_halvings <= max_halvings <= " +
                                           std::to_string(SIM_MAX_HALVINGS));
    ad.min_halvings = min_halvings;
    ad.max_halvings = max_halvings;

    SimSystem sys{};
    int n_bern_factors = 0;
    if (const int refused = sim_plan(ctx, who, n_states, h, n_forcing_cols, n_norm_forcing, n_norm, norm_src, norm_lo, norm_span,
                                     n_forcing_factors, n_factors, fac_norm, fac_kind, fac_row, fac_degree, n_spline_rows,
                                     n_bern_rows, n_entries, entries, entry_begin, entry_count, constant, n_coef, box, sys,
                                     n_bern_factors))
        return refused;
    // sim_plan's LDS bound for this caller: simulate's rows and one set of tangent rows
    const size_t lds_rows = 2 * ((size_t)1 + n_factors + (n_norm - n_norm_forcing)) + n_coef;
    const size_t lds_bytes = lds_rows * SIM_LANES * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_rows) + " values per member in LDS (2 x (1 + "
                                           "factors + normalised states) + coefficients: simulate's and one set of tangent rows), "
                                           "a wavefront's " + std::to_string(SIM_LDS_BUDGET / 1024) + " KB hold " +
                                           std::to_string(SIM_LDS_BUDGET / (SIM_LANES * sizeof(double))));

    const int64_t n_points = n_steps + 1;
    const size_t E = (size_t)n_members, ld = (E + SIM_LANES - 1) / SIM_LANES * SIM_LANES;
    std::vector<double> coef_ld((size_t)n_coef * ld, 0.0), state((size_t)n_states * ld, 0.0);
    for (size_t c = 0; c < (size_t)n_coef; ++c) std::memcpy(coef_ld.data() + c * ld, coef + c * E, E * sizeof(double));
    for (size_t k = 0; k < (size_t)n_states; ++k) std::memcpy(state.data() + k * ld, y0 + k * E, E * sizeof(double));
    std::vector<int32_t> lane_i32(4 * ld, -1);                        // level, first_saturation, first_unresolved, max_level
    std::fill(lane_i32.begin(), lane_i32.begin() + ld, min_halvings);
    std::fill(lane_i32.begin() + 3 * ld, lane_i32.end(), 0);
    std::vector<long long> lane_i64(3 * ld, 0);                       // steps, rejected, swaps
    std::vector<double> lane_error(ld, 0.0);

    // output steps per launch: the worst case of a launch is every lane at the finest level, 2^max_halvings substeps per
    // step; FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH overrides the bound on it (tests: the cut changes no bit of the result)
    int64_t per_launch = std::max(1, env_int("FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH", 65536) >> max_halvings);
    const int64_t resident = ((int64_t)256 << 20) / (int64_t)((size_t)n_states * ld * sizeof(double));
    per_launch = std::max<int64_t>(1, std::min(per_launch, resident - 1));
    const int chunk_cap = (int)std::min<int64_t>(per_launch + 1, n_points);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    int *d_norm_src = nullptr, *d_fac_norm = nullptr, *d_fac_row = nullptr, *d_fac_degree = nullptr, *d_lane_i32 = nullptr;
    long long *d_lane_i64 = nullptr;
    signed char *d_levels = nullptr;
    int4 *d_entries = nullptr;
    double *d_norm_lo = nullptr, *d_norm_span = nullptr, *d_spline = nullptr, *d_bern = nullptr, *d_coef = nullptr,
           *d_forcing = nullptr, *d_state = nullptr, *d_error = nullptr, *d_points = nullptr, *d_mean = nullptr,
           *d_bounds = nullptr, *d_members = nullptr;
    HIP_TRY(ctx, buf.upload(&d_norm_src, norm_src, (size_t)n_norm));
    HIP_TRY(ctx, buf.upload(&d_norm_lo, norm_lo, (size_t)n_norm));
    HIP_TRY(ctx, buf.upload(&d_norm_span, norm_span, (size_t)n_norm));
    HIP_TRY(ctx, buf.upload(&d_fac_norm, fac_norm, (size_t)n_factors));
    HIP_TRY(ctx, buf.upload(&d_fac_row, fac_row, (size_t)n_factors));
    HIP_TRY(ctx, buf.upload(&d_fac_degree, fac_degree, (size_t)n_factors));
    HIP_TRY(ctx, buf.upload(&d_entries, entries, (size_t)n_entries));
    HIP_TRY(ctx, buf.upload(&d_spline, spline_table, (size_t)n_spline_rows * SIM_PIECES * 4));
    HIP_TRY(ctx, buf.upload(&d_bern, bern_table, (size_t)n_bern_rows * SIM_BERN_WIDTH));
    HIP_TRY(ctx, buf.upload(&d_coef, coef_ld.data(), coef_ld.size()));
    HIP_TRY(ctx, buf.upload(&d_forcing, forcing, (size_t)n_steps * n_forcing_cols));
    HIP_TRY(ctx, buf.upload(&d_state, state.data(), state.size()));
    HIP_TRY(ctx, buf.upload(&d_lane_i32, lane_i32.data(), lane_i32.size()));
    HIP_TRY(ctx, buf.upload(&d_lane_i64, lane_i64.data(), lane_i64.size()));
    HIP_TRY(ctx, buf.upload(&d_error, lane_error.data(), lane_error.size()));
    if (levels) HIP_TRY(ctx, buf.get(&d_levels, (size_t)n_steps * ld));
    HIP_TRY(ctx, buf.get(&d_points, (size_t)n_states * chunk_cap * ld));
    HIP_TRY(ctx, buf.get(&d_mean, (size_t)n_states * n_points));
    if (bounds) HIP_TRY(ctx, buf.get(&d_bounds, (size_t)n_states * n_points * 2));
    if (members) HIP_TRY(ctx, buf.get(&d_members, E * n_states * chunk_cap));
    const SimTables tab{d_norm_src, d_norm_lo, d_norm_span, d_fac_norm, d_fac_row, d_fac_degree, d_entries, d_spline, d_bern};

    int npow2 = 2;
    while (npow2 < n_members) npow2 <<= 1;
    const size_t band_lds = bounds ? (size_t)npow2 * sizeof(double) : 0;
    if (band_lds > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(ensemble_band_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, GI_BAND_MAX_MEMBERS * (int)sizeof(double)));

    const int grid = (int)(ld / SIM_LANES);
    int64_t launches = 0;
    for (int64_t t0 = 0, p_first = 0; p_first < n_points;) {
        const int write_first = t0 == 0;
        const int steps = (int)std::min<int64_t>(per_launch, n_steps - t0);
        const int chunk_points = steps + write_first;
        {
            // bytes as simulate's; the work depends on the levels the members choose and is not known here
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)ld * n_states * (chunk_points + 2.0), 0.0);
            hipError_t launched = hipSuccess;
#define SIM_CASE(NS)                                                                                                        \
    case NS:                                                                                                                \
        launched = sim_stiff_launch<NS>(ctx, grid, lds_bytes, sys, ad, tab, d_coef, d_forcing, d_state, d_lane_i32,         \
                                        d_lane_i64, d_error, d_levels, d_points, (int64_t)ld, t0, steps, chunk_points,      \
                                        write_first);                                                                       \
        break;
            switch (n_states) {
                SIM_CASE(1) SIM_CASE(2) SIM_CASE(3) SIM_CASE(4) SIM_CASE(5) SIM_CASE(6) SIM_CASE(7) SIM_CASE(8)
            }
#undef SIM_CASE
            HIP_TRY(ctx, launched);
            ++launches;
        }
        {
            const int rows = n_states * chunk_points;
            const int band_grid = std::min(rows, cu_count(ctx) * (band_lds > 32 * 1024 ? 1 : 4));
            TimedRegion timed(ctx, FOKL_K_BAND, 8.0 * (double)rows * (E + 3.0), (double)rows * E);
            hipLaunchKernelGGL(ensemble_band_kernel, dim3(band_grid), dim3(GI_BAND_THREADS), band_lds, ctx->stream,
                               d_points, (int64_t)ld, n_members, n_states, chunk_points, n_points, p_first, npow2, cut,
                               d_mean, d_bounds);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (members) {
            hipLaunchKernelGGL(ensemble_transpose_kernel, dim3((n_members + 31) / 32, (chunk_points + 31) / 32, n_states),
                               dim3(256), 0, ctx->stream, d_points, (int64_t)ld, n_members, n_states, chunk_points,
                               d_members);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy2D(members + p_first, (size_t)n_points * sizeof(double), d_members,
                                     (size_t)chunk_points * sizeof(double), (size_t)chunk_points * sizeof(double),
                                     E * n_states, hipMemcpyDeviceToHost));
        }
        t0 += steps;
        p_first += chunk_points;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(mean, d_mean, (size_t)n_states * n_points * sizeof(double), hipMemcpyDeviceToHost));
    if (bounds)
        HIP_TRY(ctx, hipMemcpy(bounds, d_bounds, (size_t)n_states * n_points * 2 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(lane_i32.data(), d_lane_i32, lane_i32.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(lane_i64.data(), d_lane_i64, lane_i64.size() * sizeof(long long), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(error, d_error, E * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(first_saturation, lane_i32.data() + ld, E * sizeof(int32_t));
    std::memcpy(first_unresolved, lane_i32.data() + 2 * ld, E * sizeof(int32_t));
    std::memcpy(max_level, lane_i32.data() + 3 * ld, E * sizeof(int32_t));
    int64_t total_steps = 0, total_rejected = 0, total_swaps = 0;
    for (size_t e = 0; e < E; ++e) {
        total_steps += taken[e] = lane_i64[e];
        total_rejected += rejected[e] = lane_i64[ld + e];
        total_swaps += swaps[e] = lane_i64[2 * ld + e];
    }
    if (levels && n_steps > 0) {                                      // [step][ld] on the device -> [member][step]
        std::vector<int8_t> by_step((size_t)n_steps * ld);
        HIP_TRY(ctx, hipMemcpy(by_step.data(), d_levels, by_step.size(), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < E; ++e)
            for (int64_t s = 0; s < n_steps; ++s) levels[e * (size_t)n_steps + s] = by_step[(size_t)s * ld + e];
    }
    int64_t *rep = ctx->simulate_stiff_report;
    rep[0] = n_states;
    rep[1] = n_members;
    rep[2] = grid;
    rep[3] = launches;
    rep[4] = per_launch;
    rep[5] = (int64_t)lds_bytes;
    rep[6] = min_halvings;
    rep[7] = max_halvings;
    rep[8] = total_steps;
    rep[9] = total_rejected;
    rep[10] = total_swaps;
    return FOKL_OK;
}

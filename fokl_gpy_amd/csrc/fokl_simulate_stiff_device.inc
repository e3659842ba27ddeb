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

extern "C" int fokl_simulate_stiff_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_simulate_stiff_report: null argument");
    std::memcpy(out, ctx->simulate_stiff_report, sizeof ctx->simulate_stiff_report);
    return FOKL_OK;
}

extern "C" int fokl_simulate_stiff(fokl_ctx *ctx, const fokl_system *system, int cut, double rtol, const double *atol,
                                   int min_halvings, int max_halvings, double *mean, double *bounds, double *members,
                                   int32_t *first_saturation, int64_t *taken, int64_t *rejected, int64_t *swaps,
                                   int32_t *max_level, double *error, int32_t *first_unresolved, int8_t *levels)
{
    const std::string who = "fokl_simulate_stiff: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->simulate_stiff_report, 0, sizeof ctx->simulate_stiff_report);
    const bool own_ok = mean && first_saturation && atol && taken && rejected && swaps && max_level && error && first_unresolved;
    if (const int refused = sim_check(ctx, who, system, own_ok, sim_steps_fit)) return refused;
    const fokl_system &s = *system;
    const SimOutputs out{cut, mean, bounds, members};
    if (const int refused = sim_outputs_check(ctx, who, s, out)) return refused;
    SimAdaptive ad{};
    if (const int refused = sim_adaptive_check(ctx, who, s.n_states, rtol, atol, min_halvings, max_halvings, ad)) return refused;
    SimSystem sys{};
    int n_bern_factors = 0;
    if (const int refused = sim_plan(ctx, who, s, sys, n_bern_factors)) return refused;
    // sim_plan's LDS bound for this caller: simulate's rows and one set of tangent rows
    const size_t lds_rows = 2 * ((size_t)1 + s.n_factors + (s.n_norm - s.n_norm_forcing)) + s.n_coef;
    const size_t lds_bytes = lds_rows * SIM_LANES * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_rows) + " values per member in LDS (2 x (1 + "
                                           "factors + normalised states) + coefficients: simulate's and one set of tangent rows), "
                                           "a wavefront's " + std::to_string(SIM_LDS_BUDGET / 1024) + " KB hold " +
                                           std::to_string(SIM_LDS_BUDGET / (SIM_LANES * sizeof(double))));

    const SimRecord rec{first_saturation, max_level, first_unresolved, error, levels, 3, {taken, rejected, swaps}};
    int grid = 0;
    int64_t per_launch = 0, launches = 0, totals[3] = {};
    if (const int failed = sim_adaptive_run(
            ctx, s, sys, ad, lds_bytes, "FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH", out, rec,
            [](auto ns) { return simulate_stiff_kernel<decltype(ns)::value>; }, grid, per_launch, launches, totals))
        return failed;
    int64_t *rep = ctx->simulate_stiff_report;
    rep[0] = s.n_states;
    rep[1] = s.n_members;
    rep[2] = grid;
    rep[3] = launches;
    rep[4] = per_launch;
    rep[5] = (int64_t)lds_bytes;
    rep[6] = min_halvings;
    rep[7] = max_halvings;
    rep[8] = totals[0];
    rep[9] = totals[1];
    rep[10] = totals[2];
    return FOKL_OK;
}

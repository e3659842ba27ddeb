// dynamics.simulate_adaptive (textually included by fokl_hip.hip, after fokl_simulate_device.inc): simulate's system and
// simulate's Runge-Kutta step, with the substep chosen per member by step doubling on a dyadic grid.
//
// The statement of the arithmetic is dynamics.simulate_adaptive_host (fokl_gpy_amd/dynamics.py, module docstring); this
// file follows it operation for operation: only + - * /, ceil, comparisons and integer bookkeeping, under the tree's
// -ffp-contract=off, so every member's trajectory and record equal the host's bit for bit.
//
// simulate_adaptive_kernel<NS> has simulate_ensemble_kernel's layout: one lane per member, one wavefront per workgroup, the
// member's factors, normalised states and coefficients in LDS as [item][lane] touched by their own lane only, the wiring and
// the tables at wave-uniform addresses.  What is new is per lane: the level k, the position pos inside the output step, the
// counters (pairs, rejected), the largest accepted error ratio, max_level, first_unresolved and first_saturation.  Inside an
// output step a lane loops until ITS pos reaches FULL = 2^max_halvings; a finished lane idles under the exec mask until the
// slowest lane of the wavefront is through.  sim_stage's loop bounds are wave-uniform, so nothing else diverges; it takes the
// lane's own substep through its OWN_STEP variant.
// One trial is three steps of the scheme (from y with 2 g, from y with g, from there with g): twelve stage evaluations.
//
// The time axis is cut into launches of max(1, FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH >> max_halvings) steps (default
// 65 536 pairs), so a launch's worst case -- every lane forced to the finest level -- is bounded.  The state and the per-lane
// values are carried in device memory between launches; the cut changes no bit.  No atomics: member e of a large run is
// member e run alone.  Points are written as [state][point][member] for ensemble_band_kernel / ensemble_transpose_kernel.

namespace fokl {

constexpr int SIM_MAX_HALVINGS = 12;

struct SimAdaptive {
    double rtol;
    double atol[SIM_MAX_STATES];
    int min_halvings, max_halvings;
};

// 2^-n for 0 <= n <= 1022 from its bits: an exact scaling, no library call
__device__ __forceinline__ double sim_pow2_neg(int n) { return __longlong_as_double((long long)(1023 - n) << 52); }

// lane_i32 [4][ld]: level, first_saturation, first_unresolved, max_level; lane_i64 [2][ld]: pairs, rejected; error [ld];
// levels [all steps][ld] or null.  The rest as simulate_ensemble_kernel.
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void simulate_adaptive_kernel(
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
    double *fac = lds + lane;                                          // [1 + n_factors][64]: slot 0 is 1.0
    double *xn = lds + (size_t)(1 + sys.n_factors) * SIM_LANES + lane; // [n_norm - n_norm_forcing][64]
    double *cf = xn + (sys.n_norm - sys.n_norm_forcing) * SIM_LANES;   // [n_coef][64]
    fac[0] = 1.0;
    for (int c = 0; c < sys.n_coef; ++c) cf[c * SIM_LANES] = coef[(size_t)c * ld + e];
    double y[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = state[(size_t)j * ld + e];
    int k = lane_i32[e], first = lane_i32[ld + e], unresolved = lane_i32[2 * ld + e], deepest = lane_i32[3 * ld + e];
    long long pairs = lane_i64[e], rejected = lane_i64[ld + e];
    double worst = error[e];
    const int top = ad.max_halvings, full = 1 << top;
    if (write_first) {
#pragma unroll
        for (int j = 0; j < NS; ++j) points[(size_t)j * chunk_points * ld + e] = y[j];
    }
    double *out = points + (write_first ? ld : 0) + e;
    for (int s = 0; s < steps; ++s) {
        const double *row = forcing + (size_t)(t0 + s) * sys.n_forcing_cols;    // the same row serves the whole step
        bool forcing_acted = false;
        for (int f = 0; f < sys.n_forcing_factors; ++f) {
            const int n = tab.fac_norm[f];
            const double v = sim_clamp((row[-(tab.norm_src[n] + 1)] - tab.norm_lo[n]) / tab.norm_span[n], forcing_acted);
            fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                           ? sim_cubic(tab.spline, tab.fac_row[f], v)
                                           : sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v);
        }
        if (first < 0 && forcing_acted) first = (int)(t0 + s);
        int pos = 0, step_level = 0;
        while (pos < full) {                                           // per lane: the others wait under the exec mask
            const double g = sys.h * sim_pow2_neg(k + 1);
            double y1[NS], w[NS], at[NS], dy[NS] = {}, sum[NS] = {};
#pragma unroll
            for (int j = 0; j < NS; ++j) w[j] = y[j];
            bool acted = false;
            // part 0: y -> y1 with 2 g; part 1: y -> ya with g; part 2: ya -> y2 with g (w holds y, then ya, then y2)
#pragma unroll 1
            for (int part = 0; part < 3; ++part) {
                const double hh = part == 0 ? 2.0 * g : g;
#pragma unroll 1
                for (int st = 0; st < 4; ++st) {
                    const double reach = st == 3 ? 1.0 : 0.5, weight = (st == 1 || st == 2) ? 2.0 : 1.0;
#pragma unroll
                    for (int j = 0; j < NS; ++j) at[j] = st == 0 ? w[j] : w[j] + dy[j] * reach;
                    const bool stage_acted = sim_stage<NS, SIM_LANES, true>(sys, tab, xn, fac, cf, at, dy, hh);
                    acted = acted || (stage_acted && part > 0);
#pragma unroll
                    for (int j = 0; j < NS; ++j) sum[j] = st == 0 ? dy[j] : sum[j] + weight * dy[j];
                }
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const double next = w[j] + sum[j] / 6;
                    if (part == 0) y1[j] = next;
                    else w[j] = next;
                }
            }
            bool ok = true, easy = true;
            double r = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                double d = w[j] - y1[j];
                d = d < 0 ? -d : d;
                const double a = y[j] < 0 ? -y[j] : y[j], b = w[j] < 0 ? -w[j] : w[j];
                const double limit = 15.0 * (ad.atol[j] + ad.rtol * (b > a ? b : a));
                ok = ok && d <= limit;
                easy = easy && 64.0 * d <= limit;
                const double q = d / limit;
                r = q > r ? q : r;
            }
            if (ok || k == top) {
#pragma unroll
                for (int j = 0; j < NS; ++j) y[j] = w[j];
                pos += full >> k;
                ++pairs;
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
    lane_i64[e] = pairs;
    lane_i64[ld + e] = rejected;
    error[e] = worst;
}

}  // namespace fokl

namespace {

template <int NS>
hipError_t sim_adaptive_launch(fokl_ctx *ctx, int grid, size_t lds_bytes, const SimSystem &sys, const SimAdaptive &ad,
                               const SimTables &tab, const double *coef, const double *forcing, double *state, int *lane_i32,
                               long long *lane_i64, double *error, signed char *levels, double *points, int64_t ld, int64_t t0,
                               int steps, int chunk_points, int write_first)
{
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(simulate_adaptive_kernel<NS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)SIM_LDS_BUDGET);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(simulate_adaptive_kernel<NS>, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, ad, tab.norm_src,
                       tab.norm_lo, tab.norm_span, tab.fac_norm, tab.fac_row, tab.fac_degree, tab.entries, tab.spline, tab.bern,
                       coef, forcing, state, lane_i32, lane_i64, error, levels, points, ld, t0, steps, chunk_points,
                       write_first);
    return hipGetLastError();
}

}  // namespace

extern "C" int fokl_simulate_adaptive_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_simulate_adaptive_report: null argument");
    std::memcpy(out, ctx->simulate_adaptive_report, sizeof ctx->simulate_adaptive_report);
    return FOKL_OK;
}

extern "C" int fokl_simulate_adaptive(fokl_ctx *ctx, int n_members, int n_states, int64_t n_steps, double h,
                                      int n_forcing_cols, const double *forcing, int n_norm_forcing, int n_norm,
                                      const int32_t *norm_src, const double *norm_lo, const double *norm_span,
                                      int n_forcing_factors, int n_factors, const int32_t *fac_norm,
                                      const int32_t *fac_kind, const int32_t *fac_row, const int32_t *fac_degree,
                                      int n_spline_rows, const double *spline_table, int n_bern_rows,
                                      const double *bern_table, int n_entries, const int32_t *entries,
                                      const int32_t *entry_begin, const int32_t *entry_count, const int32_t *constant,
                                      int n_coef, const double *coef, const double *y0, const double *box, int cut,
                                      double rtol, const double *atol, int min_halvings, int max_halvings, double *mean,
                                      double *bounds, double *members, int32_t *first_saturation, int64_t *pairs,
                                      int64_t *rejected, int32_t *max_level, double *error, int32_t *first_unresolved,
                                      int8_t *levels)
{
    const std::string who = "fokl_simulate_adaptive: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->simulate_adaptive_report, 0, sizeof ctx->simulate_adaptive_report);
    if (n_members <= 0 || n_states <= 0 || n_steps < 0 || n_forcing_cols < 0 || n_norm_forcing < 0 || n_norm < n_norm_forcing ||
        n_forcing_factors < 0 || n_factors < n_forcing_factors || n_spline_rows < 0 || n_bern_rows < 0 || n_entries < 0 ||
        n_coef < n_states || !entry_begin || !entry_count || !constant || !coef || !y0 || !box || !mean || !first_saturation ||
        !atol || !pairs || !rejected || !max_level || !error || !first_unresolved ||
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
    const size_t lds_rows = (size_t)1 + n_factors + (n_norm - n_norm_forcing) + n_coef;
    const size_t lds_bytes = lds_rows * SIM_LANES * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_rows) + " values per member in LDS (1 + factors + "
                                           "normalised states + coefficients), a wavefront's " + std::to_string(SIM_LDS_BUDGET / 1024) +
                                           " KB hold " + std::to_string(SIM_LDS_BUDGET / (SIM_LANES * sizeof(double))));

    const int64_t n_points = n_steps + 1;
    const size_t E = (size_t)n_members, ld = (E + SIM_LANES - 1) / SIM_LANES * SIM_LANES;
    std::vector<double> coef_ld((size_t)n_coef * ld, 0.0), state((size_t)n_states * ld, 0.0);
    for (size_t c = 0; c < (size_t)n_coef; ++c) std::memcpy(coef_ld.data() + c * ld, coef + c * E, E * sizeof(double));
    for (size_t k = 0; k < (size_t)n_states; ++k) std::memcpy(state.data() + k * ld, y0 + k * E, E * sizeof(double));
    std::vector<int32_t> lane_i32(4 * ld, -1);                        // level, first_saturation, first_unresolved, max_level
    std::fill(lane_i32.begin(), lane_i32.begin() + ld, min_halvings);
    std::fill(lane_i32.begin() + 3 * ld, lane_i32.end(), 0);
    std::vector<long long> lane_i64(2 * ld, 0);                       // pairs, rejected
    std::vector<double> lane_error(ld, 0.0);

    // steps per launch: the worst case of a launch is every lane at the finest level, 2^max_halvings pairs per step;
    // FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH overrides the bound on it (tests: the cut changes no bit of the result)
    int64_t per_launch = std::max(1, env_int("FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH", 65536) >> max_halvings);
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
        launched = sim_adaptive_launch<NS>(ctx, grid, lds_bytes, sys, ad, tab, d_coef, d_forcing, d_state, d_lane_i32,      \
                                           d_lane_i64, d_error, d_levels, d_points, (int64_t)ld, t0, steps, chunk_points,   \
                                           write_first);                                                                    \
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
    int64_t total_pairs = 0, total_rejected = 0;
    for (size_t e = 0; e < E; ++e) {
        total_pairs += pairs[e] = lane_i64[e];
        total_rejected += rejected[e] = lane_i64[ld + e];
    }
    if (levels && n_steps > 0) {                                      // [step][ld] on the device -> [member][step]
        std::vector<int8_t> by_step((size_t)n_steps * ld);
        HIP_TRY(ctx, hipMemcpy(by_step.data(), d_levels, by_step.size(), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < E; ++e)
            for (int64_t s = 0; s < n_steps; ++s) levels[e * (size_t)n_steps + s] = by_step[(size_t)s * ld + e];
    }
    int64_t *rep = ctx->simulate_adaptive_report;
    rep[0] = n_states;
    rep[1] = n_members;
    rep[2] = grid;
    rep[3] = launches;
    rep[4] = per_launch;
    rep[5] = (int64_t)lds_bytes;
    rep[6] = n_factors - n_bern_factors;
    rep[7] = n_bern_factors;
    rep[8] = min_halvings;
    rep[9] = max_halvings;
    rep[10] = total_pairs;
    rep[11] = total_rejected;
    return FOKL_OK;
}

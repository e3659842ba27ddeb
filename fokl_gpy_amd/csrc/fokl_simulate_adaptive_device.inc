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

// What simulate_adaptive and simulate_stiff refuse of their tolerances and levels, and the kernels' copy of them
int sim_adaptive_check(fokl_ctx *ctx, const std::string &who, int n_states, double rtol, const double *atol, int min_halvings,
                       int max_halvings, SimAdaptive &ad)
{
    if (!(rtol >= 0) || !std::isfinite(rtol)) return fail(ctx, FOKL_ERR_ARG, who + "rtol must be finite and not negative");
    ad = SimAdaptive{};
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
    return FOKL_OK;
}

// The members' record of an adaptive call: `n_counters` int64 rows of the kernel's lane_i64 (2 or 3) and the rest
struct SimRecord {
    int32_t *first_saturation, *max_level, *first_unresolved;
    double *error;
    int8_t *levels;
    int n_counters;
    int64_t *counters[3];
};

// What simulate_adaptive and simulate_stiff run after their checks: the per-lane arrays up, sim_run over the caller's kernel
// (kernel_of(ns): its instance for ns states; both take simulate_adaptive_kernel's arguments), the record and its totals
// back.  bound_env: the environment variable that bounds a launch's substeps.
template <class KernelOf>
int sim_adaptive_run(fokl_ctx *ctx, const fokl_system &s, const SimSystem &sys, const SimAdaptive &ad, size_t lds_bytes,
                     const char *bound_env, const SimOutputs &out, const SimRecord &rec, KernelOf kernel_of, int &grid,
                     int64_t &per_launch, int64_t &launches, int64_t (&totals)[3])
{
    const int64_t n_steps = s.n_steps;
    const size_t E = (size_t)s.n_members, ld = (E + SIM_LANES - 1) / SIM_LANES * SIM_LANES;
    std::vector<int32_t> lane_i32(4 * ld, -1);                        // level, first_saturation, first_unresolved, max_level
    std::fill(lane_i32.begin(), lane_i32.begin() + ld, ad.min_halvings);
    std::fill(lane_i32.begin() + 3 * ld, lane_i32.end(), 0);
    std::vector<long long> lane_i64((size_t)rec.n_counters * ld, 0);
    const std::vector<double> lane_error(ld, 0.0);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    SimTables tab{};
    int *d_lane_i32 = nullptr;
    long long *d_lane_i64 = nullptr;
    signed char *d_levels = nullptr;
    double *d_coef = nullptr, *d_forcing = nullptr, *d_state = nullptr, *d_error = nullptr;
    HIP_TRY(ctx, sim_upload(buf, s, tab, d_forcing));
    HIP_TRY(ctx, sim_upload_padded(buf, &d_coef, s.coef, (size_t)s.n_coef, E, ld));
    HIP_TRY(ctx, sim_upload_padded(buf, &d_state, s.y0, (size_t)s.n_states, E, ld));
    HIP_TRY(ctx, buf.upload(&d_lane_i32, lane_i32.data(), lane_i32.size()));
    HIP_TRY(ctx, buf.upload(&d_lane_i64, lane_i64.data(), lane_i64.size()));
    HIP_TRY(ctx, buf.upload(&d_error, lane_error.data(), lane_error.size()));
    if (rec.levels) HIP_TRY(ctx, buf.get(&d_levels, (size_t)n_steps * ld));

    // output steps per launch: the worst case of a launch is every lane at the finest level, 2^max_halvings substeps per step;
    // bound_env overrides the bound on it (tests: the cut changes no bit of the result).  The work depends on the levels the
    // members choose and is not known here.
    grid = (int)(ld / SIM_LANES);
    const auto launch = [&](double *points, int64_t t0, int steps, int chunk_points, int write_first) {
        return sim_dispatch(s.n_states, [&](auto ns) {
            const auto kernel = kernel_of(ns);
            if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, ad, tab.norm_src, tab.norm_lo,
                               tab.norm_span, tab.fac_norm, tab.fac_row, tab.fac_degree, tab.entries, tab.spline, tab.bern,
                               (const double *)d_coef, (const double *)d_forcing, d_state, d_lane_i32, d_lane_i64, d_error,
                               d_levels, points, (int64_t)ld, t0, steps, chunk_points, write_first);
            return hipGetLastError();
        });
    };
    if (const int failed = sim_run(ctx, s, ld, std::max(1, env_int(bound_env, 65536) >> ad.max_halvings), out, 0.0, buf, launch,
                                   per_launch, launches))
        return failed;
    HIP_TRY(ctx, hipMemcpy(lane_i32.data(), d_lane_i32, lane_i32.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(lane_i64.data(), d_lane_i64, lane_i64.size() * sizeof(long long), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(rec.error, d_error, E * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(rec.first_saturation, lane_i32.data() + ld, E * sizeof(int32_t));
    std::memcpy(rec.first_unresolved, lane_i32.data() + 2 * ld, E * sizeof(int32_t));
    std::memcpy(rec.max_level, lane_i32.data() + 3 * ld, E * sizeof(int32_t));
    for (int c = 0; c < rec.n_counters; ++c) {
        totals[c] = 0;
        for (size_t e = 0; e < E; ++e) totals[c] += rec.counters[c][e] = lane_i64[c * ld + e];
    }
    if (rec.levels && n_steps > 0) {                                  // [step][ld] on the device -> [member][step]
        std::vector<int8_t> by_step((size_t)n_steps * ld);
        HIP_TRY(ctx, hipMemcpy(by_step.data(), d_levels, by_step.size(), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < E; ++e)
            for (int64_t step = 0; step < n_steps; ++step) rec.levels[e * (size_t)n_steps + step] = by_step[(size_t)step * ld + e];
    }
    return FOKL_OK;
}

}  // namespace

extern "C" int fokl_simulate_adaptive_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_simulate_adaptive_report: null argument");
    std::memcpy(out, ctx->simulate_adaptive_report, sizeof ctx->simulate_adaptive_report);
    return FOKL_OK;
}

extern "C" int fokl_simulate_adaptive(fokl_ctx *ctx, const fokl_system *system, int cut, double rtol, const double *atol,
                                      int min_halvings, int max_halvings, double *mean, double *bounds, double *members,
                                      int32_t *first_saturation, int64_t *pairs, int64_t *rejected, int32_t *max_level,
                                      double *error, int32_t *first_unresolved, int8_t *levels)
{
    const std::string who = "fokl_simulate_adaptive: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->simulate_adaptive_report, 0, sizeof ctx->simulate_adaptive_report);
    const bool own_ok = mean && first_saturation && atol && pairs && rejected && max_level && error && first_unresolved;
    if (const int refused = sim_check(ctx, who, system, own_ok, sim_steps_fit)) return refused;
    const fokl_system &s = *system;
    const SimOutputs out{cut, mean, bounds, members};
    if (const int refused = sim_outputs_check(ctx, who, s, out)) return refused;
    SimAdaptive ad{};
    if (const int refused = sim_adaptive_check(ctx, who, s.n_states, rtol, atol, min_halvings, max_halvings, ad)) return refused;
    SimSystem sys{};
    int n_bern_factors = 0;
    if (const int refused = sim_plan(ctx, who, s, sys, n_bern_factors)) return refused;
    const size_t lds_rows = (size_t)1 + s.n_factors + (s.n_norm - s.n_norm_forcing) + s.n_coef;
    const size_t lds_bytes = lds_rows * SIM_LANES * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_rows) + " values per member in LDS (1 + factors + "
                                           "normalised states + coefficients), a wavefront's " + std::to_string(SIM_LDS_BUDGET / 1024) +
                                           " KB hold " + std::to_string(SIM_LDS_BUDGET / (SIM_LANES * sizeof(double))));

    const SimRecord rec{first_saturation, max_level, first_unresolved, error, levels, 2, {pairs, rejected, nullptr}};
    int grid = 0;
    int64_t per_launch = 0, launches = 0, totals[3] = {};
    if (const int failed = sim_adaptive_run(
            ctx, s, sys, ad, lds_bytes, "FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH", out, rec,
            [](auto ns) { return simulate_adaptive_kernel<decltype(ns)::value>; }, grid, per_launch, launches, totals))
        return failed;
    int64_t *rep = ctx->simulate_adaptive_report;
    rep[0] = s.n_states;
    rep[1] = s.n_members;
    rep[2] = grid;
    rep[3] = launches;
    rep[4] = per_launch;
    rep[5] = (int64_t)lds_bytes;
    rep[6] = s.n_factors - n_bern_factors;
    rep[7] = n_bern_factors;
    rep[8] = min_halvings;
    rep[9] = max_halvings;
    rep[10] = totals[0];
    rep[11] = totals[1];
    return FOKL_OK;
}

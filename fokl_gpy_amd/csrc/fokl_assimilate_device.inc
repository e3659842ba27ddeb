// dynamics.assimilate (textually included by fokl_hip.hip, after fokl_simulate_device.inc): a bootstrap particle filter of a
// system of fitted models against measurements, 64 particles per posterior draw, every draw at once.
//
// The statement of the arithmetic is dynamics.assimilate_host (fokl_gpy_amd/dynamics.py, module docstring).  A step of a
// particle is a step of simulate_ensemble_kernel's member -- sim_stage / sim_cubic / sim_horner of fokl_simulate_device.inc,
// with the coefficient stride 1 -- so without noise a particle equals dynamics.simulate_host's member bit for bit; what
// passes through exp / log / cos (the weights, the evidence, the normals) agrees with the host to the two maths
// libraries' last bits.  Compiled under the tree's -ffp-contract=off: nothing is fused.
//
// assimilate_kernel<NS>: one wavefront per workgroup and posterior draw, lane = particle.  A particle's states and its
// weight are registers.  LDS holds, as in simulate_ensemble_kernel, what is a lane's own as [item][lane] (slot 0 = 1.0, the
// factor values, the stage's normalised states), then one exchange row of 64 values, then the draw's coefficients ONCE
// ([coefficient], read at a wave-uniform address): bytes = (1 + factors + normalised states) x 64 x 8 + 64 x 8 + n_coef x 8.
// Cross-lane work, in the orders the statement fixes:
//   * a sum or a max over the particles is the xor butterfly with offsets 32, 16, 8, 4, 2, 1 (__shfl_xor): + and fmax are
//     commutative, so every lane ends with the same bits and what is decided from them is wave-uniform;
//   * the inclusive prefix sum of the weights is the Hillis-Steele scan with offsets 1, 2, 4, 8, 16, 32 (__shfl_up);
//   * the ancestor count reads the 64 prefix sums from the exchange row (broadcast reads), and the gather passes one
//     state at a time through it.
// No atomics, plain stores: the same arguments give the same bits.
//
// The time axis is cut into launches of at most FOKL_ASSIMILATE_STEPS_PER_LAUNCH steps (default 512); particles, weights,
// the saturation and the collapse record live in device memory between launches, the per-observation rows (whose evidence
// increments the host accumulates in observation order) in the output buffers.  The cut changes no bit.

#include "fokl_philox.h"

namespace fokl {

constexpr int ASM_STAT_EXTRA = 3;             // a row of statistics: NS means, NS variances, ESS, evidence increment, resampled
constexpr double ASM_LW_FLOOR = -745.0;       // below it exp() of the best particle's log weight is no positive double

struct AsmProblem {
    int n_observed, n_obs, n_draws;
    int obs_state[SIM_MAX_STATES];            // observed column o reads state obs_state[o]
    double obs_sd[SIM_MAX_STATES];
    double q[SIM_MAX_STATES];                 // process_sd[j] * sqrt(h), from the host
    double y0_sd[SIM_MAX_STATES];
    double threshold;                         // resample_below * 64
    uint32_t seed;
};

__device__ __forceinline__ double asm_sum(double v)
{
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) v = v + __shfl_xor(v, offset);
    return v;
}

__device__ __forceinline__ double asm_max(double v)
{
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) v = fmax(v, __shfl_xor(v, offset));
    return v;
}

__device__ __forceinline__ double asm_scan(double v, int lane)
{
#pragma unroll
    for (int offset = 1; offset <= 32; offset <<= 1) {
        const double below = __shfl_up(v, offset);
        if (lane >= offset) v = v + below;
    }
    return v;
}

// Point `point` of the time axis carries observation row r: weight, report, resample (module docstring, 4 - 6).
template <int NS>
__device__ __forceinline__ void asm_observe(const AsmProblem &ap, uint32_t draw_id, size_t e, int lane, int64_t point, int r,
                                            const double *__restrict__ data, const double *__restrict__ obs_const,
                                            double *ex, double (&y)[NS], double &W, int &collapsed,
                                            double *__restrict__ stats, double *__restrict__ particles_out,
                                            double *__restrict__ weights_out)
{
    const double *row = data + (size_t)r * ap.n_observed;
    int present = 0;
    double ss = 0.0;
    for (int o = 0; o < ap.n_observed; ++o) {                          // wave-uniform: the row and its NaN entries
        const double d = row[o];
        if (d != d) continue;
        double yo = y[0];
#pragma unroll
        for (int j = 1; j < NS; ++j) yo = ap.obs_state[o] == j ? y[j] : yo;
        const double z = (d - yo) / ap.obs_sd[o];
        ss = ss + z * z;
        ++present;
    }
    double increment = 0.0;
    if (present > 0) {
        const double lw = -0.5 * ss;
        const double m = asm_max(lw);
        const double g = W * exp(lw - m);
        const double G = asm_sum(g);
        const bool alive = G > 0.0 && G < INFINITY && m >= ASM_LW_FLOOR;
        if (__builtin_amdgcn_readfirstlane((int)alive)) {
            W = g / G;
            increment = (m + log(G)) - obs_const[r];
        } else {
            W = 1.0 / SIM_LANES;
            increment = -INFINITY;
            if (collapsed < 0) collapsed = r;
        }
    }
    const double ess = 1.0 / asm_sum(W * W);
    double *out = stats + (e * ap.n_obs + (size_t)r) * (2 * NS + ASM_STAT_EXTRA);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double mu = asm_sum(W * y[j]);
        const double dev = y[j] - mu;
        const double var = asm_sum(W * (dev * dev));
        if (lane == 0) {
            out[j] = mu;
            out[NS + j] = var;
        }
    }
    if (particles_out) {
        const size_t at = (e * ap.n_obs + (size_t)r) * SIM_LANES + lane;
#pragma unroll
        for (int j = 0; j < NS; ++j) particles_out[at * NS + j] = y[j];
        weights_out[at] = W;
    }
    const bool resample = present > 0 && increment != -INFINITY && __builtin_amdgcn_readfirstlane((int)(ess < ap.threshold));
    if (lane == 0) {
        out[2 * NS] = ess;
        out[2 * NS + 1] = increment;
        out[2 * NS + 2] = resample ? 1.0 : 0.0;
    }
    if (!resample) return;
    const double u = asm_uniform(ap.seed, draw_id, (uint32_t)point, ASM_PURPOSE_RESAMPLE, 0u);
    const double c = asm_scan(W, lane);
    ex[lane] = c;
    __syncthreads();
    const double target = ((double)lane + u) / (double)SIM_LANES * ex[SIM_LANES - 1];
    int a = 0;
    for (int k = 0; k < SIM_LANES; ++k) a += ex[k] <= target ? 1 : 0;
    a = min(a, SIM_LANES - 1);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        ex[lane] = y[j];
        __syncthreads();
        y[j] = ex[a];
        __syncthreads();
    }
    W = 1.0 / SIM_LANES;
}

// Steps [t0, t0 + steps) of every draw's particles; with `first` also point 0 (the start and an observation there).
// particles [draws][NS][64], weights [draws][64], flags [draws][2] (first saturation, collapse) in / out; coef [draws][n_coef];
// y0 [NS][draws]; obs_row [points] (-1: none); data [n_obs][n_observed] (NaN: missing); obs_const [n_obs].
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void assimilate_kernel(
    SimSystem sys, AsmProblem ap, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const double *__restrict__ coef, const double *__restrict__ forcing,
    const double *__restrict__ y0, const uint32_t *__restrict__ draw_ids, const int *__restrict__ obs_row,
    const double *__restrict__ data, const double *__restrict__ obs_const, double *__restrict__ particles,
    double *__restrict__ weights, int *__restrict__ flags, double *__restrict__ stats, double *__restrict__ particles_out,
    double *__restrict__ weights_out, int64_t t0, int steps, int first)
{
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const size_t e = blockIdx.x;
    const uint32_t draw_id = draw_ids[e];
    double *fac = lds + lane;                                          // [1 + n_factors][64]: slot 0 is 1.0
    double *xn = lds + (size_t)(1 + sys.n_factors) * SIM_LANES + lane; // [n_norm - n_norm_forcing][64]
    double *ex = lds + (size_t)(1 + sys.n_factors + sys.n_norm - sys.n_norm_forcing) * SIM_LANES;    // [64]: the exchange row
    double *cf = ex + SIM_LANES;                                       // [n_coef]: the draw's, shared by its particles
    fac[0] = 1.0;
    for (int c = lane; c < sys.n_coef; c += SIM_LANES) cf[c] = coef[e * sys.n_coef + c];
    __syncthreads();
    double y[NS], at[NS], dy[NS] = {}, sum[NS] = {};
    double W;
    int saturated = flags[2 * e], collapsed = flags[2 * e + 1];
    if (first) {
#pragma unroll
        for (int j = 0; j < NS; ++j)
            y[j] = y0[(size_t)j * ap.n_draws + e] +
                   ap.y0_sd[j] * asm_normal(ap.seed, draw_id, 0u, ASM_PURPOSE_INIT, (uint32_t)(SIM_LANES * j + lane));
        W = 1.0 / SIM_LANES;
        const int r = obs_row[0];
        if (r >= 0)
            asm_observe<NS>(ap, draw_id, e, lane, 0, r, data, obs_const, ex, y, W, collapsed, stats, particles_out, weights_out);
    } else {
#pragma unroll
        for (int j = 0; j < NS; ++j) y[j] = particles[(e * NS + j) * SIM_LANES + lane];
        W = weights[e * SIM_LANES + lane];
    }
    for (int s = 0; s < steps; ++s) {
        const int64_t step = t0 + s;
        const double *row = forcing + (size_t)step * sys.n_forcing_cols;    // the same row serves the four stages
        bool acted = false;
        for (int f = 0; f < sys.n_forcing_factors; ++f) {
            const int n = tab.fac_norm[f];
            const double v = sim_clamp((row[-(tab.norm_src[n] + 1)] - tab.norm_lo[n]) / tab.norm_span[n], acted);
            fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                           ? sim_cubic(tab.spline, tab.fac_row[f], v)
                                           : sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v);
        }
        // simulate_ensemble_kernel's four stages, operation for operation
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            const double reach = st == 3 ? 1.0 : 0.5, weight = (st == 1 || st == 2) ? 2.0 : 1.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) at[j] = st == 0 ? y[j] : y[j] + dy[j] * reach;
            const bool stage_acted = sim_stage<NS, 1>(sys, tab, xn, fac, cf, at, dy);
            acted = acted || stage_acted;
#pragma unroll
            for (int j = 0; j < NS; ++j) sum[j] = st == 0 ? dy[j] : sum[j] + weight * dy[j];
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            y[j] += sum[j] / 6;
            if (ap.q[j] != 0.0)                                         // wave-uniform
                y[j] = y[j] + ap.q[j] * asm_normal(ap.seed, draw_id, (uint32_t)(step + 1), (uint32_t)j, (uint32_t)lane);
        }
        if (saturated < 0 && __any((int)acted)) saturated = (int)step;
        const int r = obs_row[step + 1];
        if (r >= 0)
            asm_observe<NS>(ap, draw_id, e, lane, step + 1, r, data, obs_const, ex, y, W, collapsed, stats, particles_out,
                            weights_out);
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) particles[(e * NS + j) * SIM_LANES + lane] = y[j];
    weights[e * SIM_LANES + lane] = W;
    if (lane == 0) {
        flags[2 * e] = saturated;
        flags[2 * e + 1] = collapsed;
    }
}

}  // namespace fokl

extern "C" int fokl_assimilate_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_assimilate_report: null argument");
    std::memcpy(out, ctx->assimilate_report, sizeof ctx->assimilate_report);
    return FOKL_OK;
}

extern "C" int fokl_assimilate_ensemble(fokl_ctx *ctx, const fokl_system *system, const uint32_t *draw_ids, int n_observed,
                                        const int32_t *obs_state, const double *obs_sd, int n_obs, const int32_t *obs_row,
                                        const double *data, const double *obs_const, const double *process_q,
                                        const double *y0_sd, double threshold, uint32_t seed, double *stats,
                                        double *particles_out, double *weights_out, int32_t *first_saturation,
                                        int32_t *collapsed)
{
    const std::string who = "fokl_assimilate_ensemble: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->assimilate_report, 0, sizeof ctx->assimilate_report);
    const bool own_ok = draw_ids && obs_state && obs_sd && obs_row && data && obs_const && process_q && y0_sd && stats &&
                        first_saturation && collapsed && (particles_out == nullptr) == (weights_out == nullptr);
    if (const int refused = sim_check(ctx, who, system, own_ok, sim_steps_fit)) return refused;
    const fokl_system &s = *system;
    const int n_draws = s.n_members, n_states = s.n_states, n_factors = s.n_factors, n_coef = s.n_coef;
    const int64_t n_steps = s.n_steps;
    const double *y0 = s.y0;

    SimSystem sys{};
    int n_bern_factors = 0;
    if (const int refused = sim_plan(ctx, who, s, sys, n_bern_factors)) return refused;

    // ---- the observations: every index and every scale the kernel follows ----
    const int64_t n_points = n_steps + 1;
    if (n_observed < 1 || n_observed > n_states)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_observed) + " observed states of " + std::to_string(n_states));
    if (n_obs < 1 || n_obs > n_points)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_obs) + " observations on " + std::to_string(n_points) +
                                           " points: at least one, at most one per point");
    AsmProblem ap{};
    for (int o = 0; o < n_observed; ++o) {
        if (obs_state[o] < 0 || obs_state[o] >= n_states)
            return fail(ctx, FOKL_ERR_ARG, who + "an observed column reads outside the states");
        for (int before = 0; before < o; ++before)
            if (obs_state[before] == obs_state[o]) return fail(ctx, FOKL_ERR_ARG, who + "a state is observed twice");
        if (!(obs_sd[o] > 0) || !std::isfinite(obs_sd[o]))
            return fail(ctx, FOKL_ERR_ARG, who + "obs_sd must be positive and finite");
        ap.obs_state[o] = obs_state[o];
        ap.obs_sd[o] = obs_sd[o];
    }
    for (int j = 0; j < n_states; ++j) {
        if (!(process_q[j] >= 0) || !std::isfinite(process_q[j]) || !(y0_sd[j] >= 0) || !std::isfinite(y0_sd[j]))
            return fail(ctx, FOKL_ERR_ARG, who + "the process noise and y0_sd must be non-negative and finite");
        ap.q[j] = process_q[j];
        ap.y0_sd[j] = y0_sd[j];
    }
    if (!(threshold >= 0) || !(threshold <= SIM_LANES))
        return fail(ctx, FOKL_ERR_ARG, who + "the resampling threshold lies outside [0, 64] particles");
    int next_row = 0;
    for (int64_t point = 0; point < n_points; ++point) {
        if (obs_row[point] == -1) continue;
        if (obs_row[point] != next_row)
            return fail(ctx, FOKL_ERR_ARG, who + "the observation table must hold the rows 0, 1, ... in the order of the points "
                                                 "(-1: none)");
        ++next_row;
    }
    if (next_row != n_obs)
        return fail(ctx, FOKL_ERR_ARG, who + "the observation table holds " + std::to_string(next_row) + " rows, data " +
                                           std::to_string(n_obs));
    for (int r = 0; r < n_obs; ++r)
        if (!std::isfinite(obs_const[r])) return fail(ctx, FOKL_ERR_ARG, who + "a row's normalising constant is not finite");
    for (size_t i = 0; i < (size_t)n_states * n_draws; ++i)
        if (!std::isfinite(y0[i])) return fail(ctx, FOKL_ERR_ARG, who + "y0 is not finite");
    ap.n_observed = n_observed;
    ap.n_obs = n_obs;
    ap.n_draws = n_draws;
    ap.threshold = threshold;
    ap.seed = seed;

    const size_t lds_lane_rows = (size_t)1 + n_factors + (s.n_norm - s.n_norm_forcing);
    const size_t lds_bytes = (lds_lane_rows + 1) * SIM_LANES * sizeof(double) + (size_t)n_coef * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_bytes) + " bytes of LDS ((1 + " +
                                           std::to_string(n_factors) + " factors + " + std::to_string(s.n_norm - s.n_norm_forcing) +
                                           " normalised states + the exchange row) x 64 x 8 + " + std::to_string(n_coef) +
                                           " coefficients x 8), a wavefront has " + std::to_string(SIM_LDS_BUDGET));

    const int per_launch = std::max(1, env_int("FOKL_ASSIMILATE_STEPS_PER_LAUNCH", 512));
    const size_t E = (size_t)n_draws, row_len = 2 * (size_t)n_states + ASM_STAT_EXTRA;

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    SimTables tab{};
    int *d_flags = nullptr, *d_obs_row = nullptr;
    uint32_t *d_ids = nullptr;
    double *d_coef = nullptr, *d_forcing = nullptr, *d_y0 = nullptr, *d_data = nullptr, *d_const = nullptr, *d_particles = nullptr,
           *d_weights = nullptr, *d_stats = nullptr, *d_pout = nullptr, *d_wout = nullptr;
    std::vector<int32_t> never(2 * E, -1);
    HIP_TRY(ctx, sim_upload(buf, s, tab, d_forcing));
    HIP_TRY(ctx, buf.upload(&d_coef, s.coef, E * n_coef));
    HIP_TRY(ctx, buf.upload(&d_y0, y0, E * n_states));
    HIP_TRY(ctx, buf.upload(&d_ids, draw_ids, E));
    HIP_TRY(ctx, buf.upload(&d_obs_row, obs_row, (size_t)n_points));
    HIP_TRY(ctx, buf.upload(&d_data, data, (size_t)n_obs * n_observed));
    HIP_TRY(ctx, buf.upload(&d_const, obs_const, (size_t)n_obs));
    HIP_TRY(ctx, buf.upload(&d_flags, never.data(), never.size()));
    HIP_TRY(ctx, buf.get(&d_particles, E * n_states * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_weights, E * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_stats, E * n_obs * row_len));
    if (particles_out) {
        HIP_TRY(ctx, buf.get(&d_pout, E * n_obs * SIM_LANES * n_states));
        HIP_TRY(ctx, buf.get(&d_wout, E * n_obs * SIM_LANES));
    }

    const double stage_flops = 8.0 * sim_terms_per_stage(sys, n_states) + 20.0 * (n_factors - s.n_forcing_factors);
    int64_t launches = 0, t0 = 0;
    do {
        const int first = t0 == 0;
        const int steps = (int)std::min<int64_t>(per_launch, n_steps - t0);
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)E * SIM_LANES * (n_states + 1.0) * 2.0,
                              (double)E * SIM_LANES * steps * 4.0 * stage_flops);
            const hipError_t launched = sim_dispatch(n_states, [&](auto ns) {
                const auto kernel = assimilate_kernel<decltype(ns)::value>;
                if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
                hipLaunchKernelGGL(kernel, dim3(n_draws), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, ap, tab.norm_src,
                                   tab.norm_lo, tab.norm_span, tab.fac_norm, tab.fac_row, tab.fac_degree, tab.entries, tab.spline,
                                   tab.bern, (const double *)d_coef, (const double *)d_forcing, (const double *)d_y0,
                                   (const uint32_t *)d_ids, (const int *)d_obs_row, (const double *)d_data,
                                   (const double *)d_const, d_particles, d_weights, d_flags, d_stats, d_pout, d_wout, t0, steps,
                                   first);
                return hipGetLastError();
            });
            HIP_TRY(ctx, launched);
            ++launches;
        }
        t0 += steps;
    } while (t0 < n_steps);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(stats, d_stats, E * n_obs * row_len * sizeof(double), hipMemcpyDeviceToHost));
    if (particles_out) {
        HIP_TRY(ctx, hipMemcpy(particles_out, d_pout, E * n_obs * SIM_LANES * n_states * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(weights_out, d_wout, E * n_obs * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
    }
    HIP_TRY(ctx, hipMemcpy(never.data(), d_flags, never.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < E; ++e) {
        first_saturation[e] = never[2 * e];
        collapsed[e] = never[2 * e + 1];
    }
    int64_t *rep = ctx->assimilate_report;
    rep[0] = n_states;
    rep[1] = n_draws;
    rep[2] = n_draws;
    rep[3] = (int64_t)lds_bytes;
    rep[4] = launches;
    rep[5] = per_launch;
    rep[6] = n_obs;
    rep[7] = n_factors - n_bern_factors;
    rep[8] = n_bern_factors;
    return FOKL_OK;
}

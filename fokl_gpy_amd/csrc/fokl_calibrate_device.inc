// dynamics.calibrate (textually included by fokl_hip.hip, after fokl_assimilate_device.inc): which initial states and which
// constant parameters produced a measured run of a system of fitted models -- one affine-invariant ensemble of 128 walkers
// over the unknowns per posterior draw, every draw at once.
//
// The statement of the arithmetic and of the sampler is dynamics.calibrate_host (fokl_gpy_amd/dynamics.py, module
// docstring).  The sampler is infer.py's (stretch moves, a differential-evolution jump every few iterations, counter-based
// Philox numbers); the target is a whole trajectory of simulate_ensemble_kernel's member -- sim_stage / sim_cubic /
// sim_horner of fokl_simulate_device.inc with the coefficient stride 1 -- so a walker's lp equals the host's bit for bit:
// only + - * /, ceil and comparisons go into it, compiled under the tree's -ffp-contract=off.  What passes through log and
// cos (the acceptance test, the jump's normal) agrees with the host to the two maths libraries' last bits.
//
// calibrate_kernel<NS>: one wavefront per workgroup and posterior draw.  Lane l is walker l while half 0 moves and walker
// 64 + l while half 1 moves: infer_inputs_kernel's mapping (lane = walker) leaves the lanes of the resting half idle, which a
// target that costs a trajectory cannot afford; here every half step is 64 trajectories on 64 lanes.  LDS holds what is a
// lane's own as [item][lane] -- slot 0 = 1.0, the factor values, the stage's normalised states (simulate's rows), then 7 d
// rows: the positions of the lane's two walkers (half 0, half 1), the proposal, and per half the running sum and sum of
// squares -- and the draw's coefficients once (read at a wave-uniform address):
//   bytes = (1 + factors + normalised states + 7 d) x 64 x 8 + n_coef x 8.
// lp, the saturation flag and the accept counters of a lane's two walkers are registers.  A partner's position is an LDS
// read at a computed lane of the half that does not move; a workgroup barrier (one wavefront) sits between the halves.
// A factor that reads a parameter is evaluated once per evaluation, one that reads a real forcing column once per step;
// the branch between them is wave-uniform.  No scratch, no atomics: the same arguments give the same bits, and draw e
// alone equals draw e of the full run.
//
// The iterations are cut into launches of max(1, FOKL_CALIBRATE_STEPS_PER_LAUNCH / (2 n_steps)) iterations (default
// 65 536 steps); positions, lp, flags, sums and counters live in device memory between launches.  The cut changes no bit.

#include "fokl_philox.h"

namespace fokl {

constexpr int CAL_WALKERS = FOKL_CALIBRATE_WALKERS;
constexpr int CAL_MAX_UNKNOWN = FOKL_CALIBRATE_MAX_UNKNOWN;
constexpr double CAL_JITTER = 1e-5;            // x (hi - lo): the jump move's normal

struct CalProblem {
    int d, n_observed, n_obs, n_draws, burnin, draws, thin, kept, jump_every;
    int obs_state[SIM_MAX_STATES];            // observed column o reads state obs_state[o]
    double obs_hp[SIM_MAX_STATES];            // 0.5 / obs_sd^2
    int state_unknown[SIM_MAX_STATES];        // the unknown that is state j's initial value, -1: y0's
    double lo[CAL_MAX_UNKNOWN], hi[CAL_MAX_UNKNOWN], prior_mean[CAL_MAX_UNKNOWN], prior_prec[CAL_MAX_UNKNOWN];
    uint32_t seed;
};

// ss = ss + hp_o (r r) over the present entries of row r in the order of the observed columns
template <int NS>
__device__ __forceinline__ double cal_observe(const CalProblem &cp, const double *__restrict__ row, const double (&y)[NS], double ss)
{
    for (int o = 0; o < cp.n_observed; ++o) {                          // wave-uniform: the row and its NaN entries
        const double v = row[o];
        if (v != v) continue;
        double yo = y[0];
#pragma unroll
        for (int j = 1; j < NS; ++j) yo = cp.obs_state[o] == j ? y[j] : yo;
        const double r = v - yo;
        ss = ss + cp.obs_hp[o] * (r * r);
    }
    return ss;
}

// lp of the point pt [d][64] (the lane's own column) along the draw's trajectory; `acted`: a clamp or the slope rule acted.
// trajectory (or null): the lane's [NS][n_steps + 1] points.
template <int NS>
__device__ __forceinline__ double cal_target(const SimSystem &sys, const CalProblem &cp, const SimTables &tab,
                                             const int *__restrict__ norm_param, double *xn, double *fac, const double *cf,
                                             const double *__restrict__ forcing, const double *__restrict__ y0, size_t e,
                                             const int *__restrict__ obs_row, const double *__restrict__ data, int64_t n_steps,
                                             const double *pt, bool &acted, double *__restrict__ trajectory)
{
    double y[NS], at[NS], dy[NS] = {}, sum[NS] = {};
    acted = false;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int i = cp.state_unknown[j];                             // wave-uniform
        y[j] = i >= 0 ? pt[i * SIM_LANES] : y0[(size_t)j * cp.n_draws + e];
    }
    for (int f = 0; f < sys.n_forcing_factors; ++f) {                  // the factors of the parameters: once per evaluation
        const int n = tab.fac_norm[f], i = norm_param[n];
        if (i < 0) continue;
        const double v = sim_clamp((pt[i * SIM_LANES] - tab.norm_lo[n]) / tab.norm_span[n], acted);
        fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                       ? sim_cubic(tab.spline, tab.fac_row[f], v)
                                       : sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v);
    }
    double ss = 0.0;
    if (trajectory) {
#pragma unroll
        for (int j = 0; j < NS; ++j) trajectory[(size_t)j * (n_steps + 1)] = y[j];
    }
    if (obs_row[0] >= 0) ss = cal_observe<NS>(cp, data + (size_t)obs_row[0] * cp.n_observed, y, ss);
    for (int64_t step = 0; step < n_steps; ++step) {
        const double *row = forcing + (size_t)step * sys.n_forcing_cols;
        for (int f = 0; f < sys.n_forcing_factors; ++f) {              // the factors of the real forcing columns: once per step
            const int n = tab.fac_norm[f];
            if (norm_param[n] >= 0) continue;
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
        for (int j = 0; j < NS; ++j) y[j] += sum[j] / 6;
        if (trajectory) {
#pragma unroll
            for (int j = 0; j < NS; ++j) trajectory[(size_t)j * (n_steps + 1) + step + 1] = y[j];
        }
        const int r = obs_row[step + 1];
        if (r >= 0) ss = cal_observe<NS>(cp, data + (size_t)r * cp.n_observed, y, ss);
    }
    double pp = 0.0;
    for (int i = 0; i < cp.d; ++i) {
        const double dl = pt[i * SIM_LANES] - cp.prior_mean[i];
        pp = pp + cp.prior_prec[i] * (dl * dl);
    }
    return -ss - 0.5 * pp;
}

// Iterations [t0, t0 + iterations) of every draw's ensemble; with `first` also the starts and their lp.  In / out between
// launches: position [draws][128][d], lp_state [draws][128], sat_state [draws][128], acc [draws][128][2][d] (the running sums
// of the current half of the kept iterations), accept_out [draws][128][2], evals_out [draws].  With `trajectories` the final
// ensemble is integrated once more and its points are written as [draws][128][NS][n_steps + 1].
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void calibrate_kernel(
    SimSystem sys, CalProblem cp, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const int *__restrict__ norm_param, const double *__restrict__ coef,
    const double *__restrict__ forcing, const double *__restrict__ y0, const uint32_t *__restrict__ draw_ids,
    const int *__restrict__ obs_row, const double *__restrict__ data, const double *__restrict__ starts,
    double *__restrict__ position, double *__restrict__ lp_state, int *__restrict__ sat_state, double *__restrict__ acc_state,
    double *__restrict__ x_out, double *__restrict__ lp_out, int *__restrict__ sat_out, double *__restrict__ sums_out,
    int *__restrict__ accept_out, long long *__restrict__ evals_out, int *__restrict__ invalid_out,
    double *__restrict__ trajectories, int64_t n_steps, int t0, int iterations, int first)
{
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, d = cp.d;
    const size_t e = blockIdx.x;
    const uint32_t draw_id = draw_ids[e];
    double *fac = lds + lane;                                          // [1 + n_factors][64]: slot 0 is 1.0
    double *xn = lds + (size_t)(1 + sys.n_factors) * SIM_LANES + lane; // [n_norm - n_norm_forcing][64]
    double *xs = xn + (size_t)(sys.n_norm - sys.n_norm_forcing) * SIM_LANES;    // [2][d][64]: walker lane, walker 64 + lane
    double *pr = xs + (size_t)2 * d * SIM_LANES;                       // [d][64]: the proposal
    double *acc = pr + (size_t)d * SIM_LANES;                          // [2][2][d][64]: per half the sum and the sum of squares
    double *cf = lds + (size_t)(1 + sys.n_factors + sys.n_norm - sys.n_norm_forcing + 7 * d) * SIM_LANES;   // [n_coef]
    const double *all = xs - lane;                                     // walker w = 64 hf + l: all[(hf d + i) 64 + l]
    fac[0] = 1.0;
    for (int c = lane; c < sys.n_coef; c += SIM_LANES) cf[c] = coef[e * sys.n_coef + c];
    __syncthreads();

    const auto target = [&](const double *pt, bool &acted, double *trajectory) {
        return cal_target<NS>(sys, cp, tab, norm_param, xn, fac, cf, forcing, y0, e, obs_row, data, n_steps, pt, acted, trajectory);
    };

    double lp0, lp1;
    bool sat0, sat1;
    int stretch0, stretch1, jump0, jump1;
    long long evals;
    const size_t w0 = e * CAL_WALKERS + lane, w1 = w0 + SIM_LANES;     // the lane's two walkers
    if (first) {
        for (int i = 0; i < d; ++i) {
            xs[i * SIM_LANES] = starts[(size_t)lane * d + i];
            xs[(d + i) * SIM_LANES] = starts[(size_t)(SIM_LANES + lane) * d + i];
        }
        for (int i = 0; i < 4 * d; ++i) acc[i * SIM_LANES] = 0.0;
        lp0 = target(xs, sat0, nullptr);
        lp1 = target(xs + (size_t)d * SIM_LANES, sat1, nullptr);
        stretch0 = stretch1 = jump0 = jump1 = 0;
        evals = CAL_WALKERS;
        const double infinity = INFINITY;
        const bool bad = !(lp0 > -infinity && lp0 < infinity) || !(lp1 > -infinity && lp1 < infinity);
        const int any_bad = __any((int)bad);
        if (lane == 0) invalid_out[e] = any_bad ? 1 : 0;
    } else {
        for (int i = 0; i < d; ++i) {
            xs[i * SIM_LANES] = position[w0 * d + i];
            xs[(d + i) * SIM_LANES] = position[w1 * d + i];
        }
        for (int i = 0; i < 2 * d; ++i) {
            acc[i * SIM_LANES] = acc_state[w0 * 2 * d + i];
            acc[(2 * d + i) * SIM_LANES] = acc_state[w1 * 2 * d + i];
        }
        lp0 = lp_state[w0];
        lp1 = lp_state[w1];
        sat0 = sat_state[w0] != 0;
        sat1 = sat_state[w1] != 0;
        stretch0 = accept_out[w0 * 2];
        jump0 = accept_out[w0 * 2 + 1];
        stretch1 = accept_out[w1 * 2];
        jump1 = accept_out[w1 * 2 + 1];
        evals = evals_out[e];
    }
    __syncthreads();

    const int first_half = cp.draws / 2;
    for (int t = t0; t < t0 + iterations; ++t) {
        const bool jump = cp.jump_every > 0 && t % cp.jump_every == cp.jump_every - 1;
        for (int half = 0; half < 2; ++half) {
            const uint32_t walker = (uint32_t)(SIM_LANES * half + lane);
            double *mine = xs + (size_t)half * d * SIM_LANES;
            const double *others = all + (size_t)(1 - half) * d * SIM_LANES;    // the half that does not move: others[i 64 + lane']
            const double u1 = cal_uniform(cp.seed, draw_id, (uint32_t)t, INF_PURPOSE_PARTNER, walker);
            const double u2 = cal_uniform(cp.seed, draw_id, (uint32_t)t, INF_PURPOSE_STRETCH, walker);
            const double u3 = cal_uniform(cp.seed, draw_id, (uint32_t)t, INF_PURPOSE_ACCEPT, walker);
            bool inside = true;
            double log_z = 0.0;
            if (!jump) {
                const int j = min((int)(64.0 * u1), SIM_LANES - 1);
                const double z = ((1.0 + u2) * (1.0 + u2)) * 0.5;
                log_z = (double)(d - 1) * log(z);
                for (int i = 0; i < d; ++i) {
                    const double xj = others[i * SIM_LANES + j], xw = mine[i * SIM_LANES];
                    const double v = xj + z * (xw - xj);
                    pr[i * SIM_LANES] = v;
                    inside = inside && v > cp.lo[i] && v < cp.hi[i];
                }
            } else {
                const int a = min((int)(64.0 * u1), SIM_LANES - 1);
                const int b = (a + 1 + min((int)(63.0 * u2), SIM_LANES - 2)) % SIM_LANES;
                for (int i = 0; i < d; ++i) {
                    const double n = cal_normal(cp.seed, draw_id, (uint32_t)t, INF_PURPOSE_JITTER, (uint32_t)(CAL_WALKERS * i) + walker);
                    const double xa = others[i * SIM_LANES + a], xb = others[i * SIM_LANES + b];
                    const double v = (mine[i * SIM_LANES] + (xa - xb)) + (CAL_JITTER * (cp.hi[i] - cp.lo[i])) * n;
                    pr[i * SIM_LANES] = v;
                    inside = inside && v > cp.lo[i] && v < cp.hi[i];
                }
            }
            const unsigned long long evaluated = __ballot((int)inside);
            evals += __popcll(evaluated);
            if (evaluated != 0ull) {                                   // wave-uniform: nothing is integrated where no lane is inside
                if (!inside)                                           // integrates where it stands; the result is dropped
                    for (int i = 0; i < d; ++i) pr[i * SIM_LANES] = mine[i * SIM_LANES];
                bool sat_y;
                const double lp_y = target(pr, sat_y, nullptr);
                const double lp_x = half ? lp1 : lp0;
                const bool accept = inside && log(u3) < (log_z + lp_y) - lp_x;
                if (accept) {
                    for (int i = 0; i < d; ++i) mine[i * SIM_LANES] = pr[i * SIM_LANES];
                    if (half) {
                        lp1 = lp_y;
                        sat1 = sat_y;
                        stretch1 += jump ? 0 : 1;
                        jump1 += jump ? 1 : 0;
                    } else {
                        lp0 = lp_y;
                        sat0 = sat_y;
                        stretch0 += jump ? 0 : 1;
                        jump0 += jump ? 1 : 0;
                    }
                }
            }
            __syncthreads();                                           // the moves are in place before the other half reads them
        }
        if (t < cp.burnin) continue;
        const int r = t - cp.burnin;
        for (int half = 0; half < 2; ++half) {
            const size_t w = half ? w1 : w0;
            double *sums = sums_out + w * (size_t)4 * d;               // [2][2][d]
            double *a = acc + (size_t)half * 2 * d * SIM_LANES;
            const double *mine = xs + (size_t)half * d * SIM_LANES;
            if (r == first_half && first_half > 0)
                for (int i = 0; i < 2 * d; ++i) {
                    sums[i] = a[i * SIM_LANES];
                    a[i * SIM_LANES] = 0.0;
                }
            for (int i = 0; i < d; ++i) {
                const double c = mine[i * SIM_LANES] - 0.5 * (cp.lo[i] + cp.hi[i]);
                a[i * SIM_LANES] = a[i * SIM_LANES] + c;
                a[(d + i) * SIM_LANES] = a[(d + i) * SIM_LANES] + c * c;
            }
            if (x_out && r % cp.thin == 0) {
                const size_t row = (e * cp.kept + (size_t)(r / cp.thin)) * CAL_WALKERS + SIM_LANES * half + lane;
                for (int i = 0; i < d; ++i) x_out[row * d + i] = mine[i * SIM_LANES];
                lp_out[row] = half ? lp1 : lp0;
                sat_out[row] = (half ? sat1 : sat0) ? 1 : 0;
            }
            if (r == cp.draws - 1)
                for (int i = 0; i < 2 * d; ++i) sums[2 * d + i] = a[i * SIM_LANES];
        }
    }

    if (trajectories) {                                                // the replay of the final ensemble: the same evaluation
        bool dropped;
        const size_t len = (size_t)NS * (n_steps + 1);
        (void)target(xs, dropped, trajectories + w0 * len);
        (void)target(xs + (size_t)d * SIM_LANES, dropped, trajectories + w1 * len);
    }
    for (int i = 0; i < d; ++i) {
        position[w0 * d + i] = xs[i * SIM_LANES];
        position[w1 * d + i] = xs[(d + i) * SIM_LANES];
    }
    for (int i = 0; i < 2 * d; ++i) {
        acc_state[w0 * 2 * d + i] = acc[i * SIM_LANES];
        acc_state[w1 * 2 * d + i] = acc[(2 * d + i) * SIM_LANES];
    }
    lp_state[w0] = lp0;
    lp_state[w1] = lp1;
    sat_state[w0] = sat0 ? 1 : 0;
    sat_state[w1] = sat1 ? 1 : 0;
    accept_out[w0 * 2] = stretch0;
    accept_out[w0 * 2 + 1] = jump0;
    accept_out[w1 * 2] = stretch1;
    accept_out[w1 * 2 + 1] = jump1;
    if (lane == 0) evals_out[e] = evals;
}

}  // namespace fokl

extern "C" int fokl_calibrate_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_calibrate_report: null argument");
    std::memcpy(out, ctx->calibrate_report, sizeof ctx->calibrate_report);
    return FOKL_OK;
}

extern "C" int fokl_calibrate_ensemble(fokl_ctx *ctx, const fokl_system *system, const fokl_calibrate_problem *problem,
                                       double *x_out, double *lp_out, int32_t *saturated_out, double *sums_out,
                                       int32_t *accept_out, int64_t *evals_out, int32_t *invalid_out, double *trajectories)
{
    const std::string who = "fokl_calibrate_ensemble: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->calibrate_report, 0, sizeof ctx->calibrate_report);
    const bool own_ok = problem && problem->unknown_src && problem->lo && problem->hi && problem->prior_mean &&
                        problem->prior_prec && problem->starts && problem->obs_state && problem->obs_hp && problem->obs_row &&
                        problem->data && problem->draw_ids && sums_out && accept_out && evals_out && invalid_out &&
                        (x_out == nullptr) == (lp_out == nullptr) && (x_out == nullptr) == (saturated_out == nullptr) &&
                        (system == nullptr || system->n_norm_forcing <= 0 || problem->norm_param);
    if (const int refused = sim_check(ctx, who, system, own_ok, sim_steps_fit)) return refused;
    const fokl_system &s = *system;
    const fokl_calibrate_problem &q = *problem;
    const int n_draws = s.n_members, n_states = s.n_states, n_factors = s.n_factors, n_coef = s.n_coef, d = q.n_unknown;
    const int64_t n_steps = s.n_steps, n_points = n_steps + 1;

    SimSystem sys{};
    int n_bern_factors = 0;
    if (const int refused = sim_plan(ctx, who, s, sys, n_bern_factors)) return refused;

    // ---- the observations: every index and every scale the kernel follows (fokl_assimilate_ensemble's refusals) ----
    if (q.n_observed < 1 || q.n_observed > n_states)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(q.n_observed) + " observed states of " + std::to_string(n_states));
    if (q.n_obs < 1 || q.n_obs > n_points)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(q.n_obs) + " observations on " + std::to_string(n_points) +
                                           " points: at least one, at most one per point");
    CalProblem cp{};
    for (int o = 0; o < q.n_observed; ++o) {
        if (q.obs_state[o] < 0 || q.obs_state[o] >= n_states)
            return fail(ctx, FOKL_ERR_ARG, who + "an observed column reads outside the states");
        for (int before = 0; before < o; ++before)
            if (q.obs_state[before] == q.obs_state[o]) return fail(ctx, FOKL_ERR_ARG, who + "a state is observed twice");
        if (!(q.obs_hp[o] > 0) || !std::isfinite(q.obs_hp[o]))
            return fail(ctx, FOKL_ERR_ARG, who + "obs_hp = 0.5 / obs_sd^2 must be positive and finite");
        cp.obs_state[o] = q.obs_state[o];
        cp.obs_hp[o] = q.obs_hp[o];
    }
    int next_row = 0;
    for (int64_t point = 0; point < n_points; ++point) {
        if (q.obs_row[point] == -1) continue;
        if (q.obs_row[point] != next_row)
            return fail(ctx, FOKL_ERR_ARG, who + "the observation table must hold the rows 0, 1, ... in the order of the points "
                                                 "(-1: none)");
        ++next_row;
    }
    if (next_row != q.n_obs)
        return fail(ctx, FOKL_ERR_ARG, who + "the observation table holds " + std::to_string(next_row) + " rows, data " +
                                           std::to_string(q.n_obs));
    for (size_t i = 0; i < (size_t)q.n_obs * q.n_observed; ++i)
        if (std::isinf(q.data[i])) return fail(ctx, FOKL_ERR_ARG, who + "data holds an infinite value (a missing measurement is NaN)");
    for (size_t i = 0; i < (size_t)n_states * n_draws; ++i)
        if (!std::isfinite(s.y0[i])) return fail(ctx, FOKL_ERR_ARG, who + "y0 is not finite");

    // ---- the unknowns ----
    if (d < 1 || d > CAL_MAX_UNKNOWN)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(d) + " unknowns, the kernel is built for 1 to " + std::to_string(CAL_MAX_UNKNOWN));
    for (int j = 0; j < SIM_MAX_STATES; ++j) cp.state_unknown[j] = -1;
    for (int i = 0; i < d; ++i) {
        const int src = q.unknown_src[i];
        if (src >= n_states || -(int64_t)src - 1 >= s.n_forcing_cols)
            return fail(ctx, FOKL_ERR_ARG, who + "unknown " + std::to_string(i) + " lies outside the " + std::to_string(n_states) +
                                               " states and the " + std::to_string(s.n_forcing_cols) + " forcing columns");
        for (int before = 0; before < i; ++before)
            if (q.unknown_src[before] == src)
                return fail(ctx, FOKL_ERR_ARG, who + "unknowns " + std::to_string(before) + " and " + std::to_string(i) + " are the same: an unknown is named twice");
        if (src >= 0) {
            cp.state_unknown[src] = i;
        } else {
            bool read = false;
            for (int n = 0; n < s.n_norm_forcing; ++n) read = read || s.norm_src[n] == src;
            if (!read) return fail(ctx, FOKL_ERR_ARG, who + "no model reads the parameter that is unknown " + std::to_string(i));
        }
        if (!(q.lo[i] < q.hi[i]) || !std::isfinite(q.lo[i]) || !std::isfinite(q.hi[i]))
            return fail(ctx, FOKL_ERR_ARG, who + "lo < hi, both finite, is needed at unknown " + std::to_string(i) + ": its box is empty or not finite");
        if (!(q.prior_prec[i] >= 0.0) || !std::isfinite(q.prior_prec[i]) || !std::isfinite(q.prior_mean[i]))
            return fail(ctx, FOKL_ERR_ARG, who + "the prior of unknown " + std::to_string(i) + " needs a finite mean and a finite precision >= 0 (a negative precision is refused)");
        cp.lo[i] = q.lo[i];
        cp.hi[i] = q.hi[i];
        cp.prior_mean[i] = q.prior_mean[i];
        cp.prior_prec[i] = q.prior_prec[i];
    }
    for (int n = 0; n < s.n_norm_forcing; ++n) {
        int expected = -1;
        for (int i = 0; i < d; ++i) expected = q.unknown_src[i] == s.norm_src[n] ? i : expected;
        if (q.norm_param[n] != expected)
            return fail(ctx, FOKL_ERR_ARG, who + "norm_param[" + std::to_string(n) + "] = " + std::to_string(q.norm_param[n]) +
                                               " but the unknowns' columns say " + std::to_string(expected) +
                                               " (an unknown parameter is no column of forcing, and a column of forcing no unknown)");
    }
    for (int w = 0; w < CAL_WALKERS; ++w)
        for (int i = 0; i < d; ++i)
            if (!(q.starts[(size_t)w * d + i] > q.lo[i] && q.starts[(size_t)w * d + i] < q.hi[i]))
                return fail(ctx, FOKL_ERR_ARG, who + "start " + std::to_string(w) + " is not strictly inside the box at unknown " + std::to_string(i));
    if (q.thin < 1 || q.draws_kept < 1 || q.burnin < 0 || q.jump_every < 0 || q.draws_kept > (1 << 30) || q.burnin > (1 << 30))
        return fail(ctx, FOKL_ERR_ARG, who + "thin >= 1, 1 <= draws_kept <= 2^30, 0 <= burnin <= 2^30 and jump_every >= 0 are needed");
    cp.d = d;
    cp.n_observed = q.n_observed;
    cp.n_obs = q.n_obs;
    cp.n_draws = n_draws;
    cp.burnin = q.burnin;
    cp.draws = q.draws_kept;
    cp.thin = q.thin;
    cp.kept = (q.draws_kept + q.thin - 1) / q.thin;
    cp.jump_every = q.jump_every;
    cp.seed = q.seed;

    const size_t n_norm_state = (size_t)(s.n_norm - s.n_norm_forcing);
    const size_t lds_lane_rows = (size_t)1 + n_factors + n_norm_state + (size_t)7 * d;
    const size_t lds_bytes = lds_lane_rows * SIM_LANES * sizeof(double) + (size_t)n_coef * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the problem needs " + std::to_string(lds_bytes) + " bytes of LDS ((1 + " +
                                           std::to_string(n_factors) + " factors + " + std::to_string(n_norm_state) +
                                           " normalised states + 7 x " + std::to_string(d) + " unknowns) x 64 x 8 + " +
                                           std::to_string(n_coef) + " coefficients x 8), a wavefront has " +
                                           std::to_string(SIM_LDS_BUDGET));

    const size_t E = (size_t)n_draws, W = E * CAL_WALKERS;
    const size_t rows = x_out ? E * cp.kept * CAL_WALKERS : 0;
    const size_t traj = trajectories ? W * n_states * (size_t)n_points : 0;
    const size_t want_bytes = (rows * (d + 1) + traj + W * (size_t)(7 * d + 1) + E * n_coef + (size_t)n_steps * s.n_forcing_cols) * sizeof(double) +
                              (rows + W * 3 + E * 4) * sizeof(int32_t) + E * 8;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_CALIBRATE_FREE_BYTES", &free_bytes));
    if (want_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + "the call wants " + std::to_string(want_bytes) + " bytes on the device and 64 MiB to spare (" +
                                           std::to_string(rows * (d + 1) * sizeof(double) + rows * sizeof(int32_t)) +
                                           " bytes of kept rows = draws x kept x 128 x ((d + 1) x 8 + 4), " +
                                           std::to_string(traj * sizeof(double)) + " of trajectories), the device has " +
                                           std::to_string(free_bytes) + " free (thin more, keep no rows, or run the draws in parts)");

    const int64_t iterations = (int64_t)q.burnin + q.draws_kept;
    const int64_t step_cap = std::max(1, env_int("FOKL_CALIBRATE_STEPS_PER_LAUNCH", 65536));
    const int64_t per_launch = std::max<int64_t>(1, step_cap / (2 * std::max<int64_t>(1, n_steps)));

    DeviceBuffers buf;
    SimTables tab{};
    int *d_param = nullptr, *d_obs_row = nullptr, *d_sat = nullptr, *d_sat_out = nullptr, *d_accept = nullptr, *d_invalid = nullptr;
    uint32_t *d_ids = nullptr;
    long long *d_evals = nullptr;
    double *d_coef = nullptr, *d_forcing = nullptr, *d_y0 = nullptr, *d_data = nullptr, *d_starts = nullptr, *d_position = nullptr,
           *d_lp = nullptr, *d_acc = nullptr, *d_x = nullptr, *d_lp_out = nullptr, *d_sums = nullptr, *d_traj = nullptr;
    HIP_TRY(ctx, sim_upload(buf, s, tab, d_forcing));
    HIP_TRY(ctx, buf.upload(&d_param, q.norm_param, (size_t)s.n_norm_forcing));
    HIP_TRY(ctx, buf.upload(&d_coef, s.coef, E * n_coef));
    HIP_TRY(ctx, buf.upload(&d_y0, s.y0, E * n_states));
    HIP_TRY(ctx, buf.upload(&d_ids, q.draw_ids, E));
    HIP_TRY(ctx, buf.upload(&d_obs_row, q.obs_row, (size_t)n_points));
    HIP_TRY(ctx, buf.upload(&d_data, q.data, (size_t)q.n_obs * q.n_observed));
    HIP_TRY(ctx, buf.upload(&d_starts, q.starts, (size_t)CAL_WALKERS * d));
    HIP_TRY(ctx, buf.get(&d_position, W * d));
    HIP_TRY(ctx, buf.get(&d_lp, W));
    HIP_TRY(ctx, buf.get(&d_sat, W));
    HIP_TRY(ctx, buf.get(&d_acc, W * 2 * d));
    HIP_TRY(ctx, buf.get(&d_sums, W * 4 * d));
    HIP_TRY(ctx, buf.get(&d_accept, W * 2));
    HIP_TRY(ctx, buf.get(&d_evals, E));
    HIP_TRY(ctx, buf.get(&d_invalid, E));
    if (x_out) {
        HIP_TRY(ctx, buf.get(&d_x, rows * d));
        HIP_TRY(ctx, buf.get(&d_lp_out, rows));
        HIP_TRY(ctx, buf.get(&d_sat_out, rows));
    }
    if (trajectories) HIP_TRY(ctx, buf.get(&d_traj, traj));
    HIP_TRY(ctx, hipMemsetAsync(d_sums, 0, W * 4 * d * sizeof(double), ctx->stream));

    const double stage_flops = 8.0 * sim_terms_per_stage(sys, n_states) + 20.0 * (n_factors - s.n_forcing_factors);
    hipError_t err = hipSuccess;
    StreamStopwatch watch(ctx, err);
    const int t0 = watch.mark();
    int64_t launches = 0;
    const auto launch = [&](int64_t t0, int count, int first, double *points) {
        TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)W * (7.0 * d + 2.0) * 2.0,
                          (double)W * (count + (points ? 1.0 : 0.0) + first) * (double)n_steps * 4.0 * stage_flops);
        ++launches;
        return sim_dispatch(n_states, [&](auto ns) {
            const auto kernel = calibrate_kernel<decltype(ns)::value>;
            if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
            hipLaunchKernelGGL(kernel, dim3(n_draws), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, cp, tab.norm_src, tab.norm_lo,
                               tab.norm_span, tab.fac_norm, tab.fac_row, tab.fac_degree, tab.entries, tab.spline, tab.bern,
                               (const int *)d_param, (const double *)d_coef, (const double *)d_forcing, (const double *)d_y0,
                               (const uint32_t *)d_ids, (const int *)d_obs_row, (const double *)d_data, (const double *)d_starts,
                               d_position, d_lp, d_sat, d_acc, d_x, d_lp_out, d_sat_out, d_sums, d_accept, d_evals, d_invalid,
                               points, n_steps, (int)t0, count, first);
            return hipGetLastError();
        });
    };
    for (int64_t t0 = 0; err == hipSuccess && t0 < iterations; t0 += per_launch)
        err = launch(t0, (int)std::min<int64_t>(per_launch, iterations - t0), t0 == 0, nullptr);
    if (err == hipSuccess && trajectories) err = launch(iterations, 0, 0, d_traj);
    const int t1 = watch.mark();
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    const double kernel_us = watch.us(t0, t1);
    if (err == hipSuccess && x_out) err = hipMemcpy(x_out, d_x, rows * d * sizeof(double), hipMemcpyDeviceToHost);
    if (err == hipSuccess && x_out) err = hipMemcpy(lp_out, d_lp_out, rows * sizeof(double), hipMemcpyDeviceToHost);
    if (err == hipSuccess && x_out) err = hipMemcpy(saturated_out, d_sat_out, rows * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(sums_out, d_sums, W * 4 * d * sizeof(double), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(accept_out, d_accept, W * 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(evals_out, d_evals, E * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(invalid_out, d_invalid, E * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (err == hipSuccess && trajectories) err = hipMemcpy(trajectories, d_traj, traj * sizeof(double), hipMemcpyDeviceToHost);
    if (err != hipSuccess) return fail(ctx, FOKL_ERR_HIP, who + hipGetErrorString(err));

    int64_t evaluations = 0;
    for (size_t e = 0; e < E; ++e) evaluations += evals_out[e];
    int64_t *rep = ctx->calibrate_report;
    rep[0] = n_states;
    rep[1] = n_draws;
    rep[2] = (int64_t)lds_bytes;
    rep[3] = launches;
    rep[4] = per_launch;
    rep[5] = evaluations;
    rep[6] = (int64_t)std::llround(kernel_us);
    rep[7] = iterations;
    return FOKL_OK;
}

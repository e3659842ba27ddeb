// Unknown inputs of a Bernoulli-polynomial model inferred from observed outputs (textually included by fokl_hip.hip behind
// fokl_optimize_core.inc): for every posterior draw one affine-invariant ensemble of 64 walkers over the unknown inputs.
// The sampler is stated in numpy by fokl_gpy_amd/infer.py (sample_host; the module docstring is the statement); this file
// is that statement on the model evaluation of fokl_optimize_core.inc (op_factors / op_terms, value only), restricted to
// the unknown columns.  Compiled under the tree's -ffp-contract=off: nothing is fused.
//
// infer_inputs_kernel: one wavefront per workgroup and posterior draw, lane = walker (FOKL_INFER_WALKER_PER_LANE).  An
// iteration updates walkers 0..31 and then walkers 32..63; the half that does not move evaluates its own position and
// drops the result, so control flow is wave-uniform and 32 lanes idle per half-step.  What is a walker's own sits in LDS
// as [item][lane]: the factor values (op_factors' three rows per distinct (input, order) factor, the first one used), the
// position, the proposal and the running sums of the current half of the kept iterations -- 3 n_slots + 4 d rows of 512
// bytes, 80 KB for 16 inputs with two orders each.  A partner's position is an LDS read at a computed lane, always in the
// half that does not move; a workgroup barrier (one wavefront: free) puts a half's moves in place before the other half
// reads them.  lp stays in a register.  What the problem is
// -- the draw's coefficients premultiplied by the known inputs' products (one row of n_terms + 1 per observation), h, y,
// the term entries, the table, the box and the prior -- is wave-uniform: scalar loads.  No scratch, no atomics.

#include "fokl_philox.h"

namespace fokl {

constexpr int INF_HALF = OP_LANES / 2;
constexpr double INF_JITTER = 1e-5;                                    // x (hi - lo): the jump move's normal

struct InfProblem {
    int d, n_slots, n_entries, n_coef, width, K, burnin, draws, thin, kept, jump_every, first_draw;
    uint32_t seed;
};

// box [2][d] (lo, hi), prior [2][d] (mean, precision), starts [64][d], w [draws][K][n_coef], h [draws], y [K], draw_ids
// [draws]; the outputs as fokl_infer_inputs documents them (x_out / lp_out may be null).  Workgroup b runs draw
// first_draw + b.
__global__ __launch_bounds__(OP_LANES) void infer_inputs_kernel(InfProblem p, const int *__restrict__ slot_var,
                                                                const int *__restrict__ slot_ord,
                                                                const int4 *__restrict__ entries,
                                                                const int *__restrict__ long_slots,
                                                                const double *__restrict__ table,
                                                                const double *__restrict__ box,
                                                                const double *__restrict__ prior,
                                                                const double *__restrict__ starts,
                                                                const double *__restrict__ w, const double *__restrict__ h,
                                                                const double *__restrict__ y,
                                                                const uint32_t *__restrict__ draw_ids,
                                                                double *__restrict__ x_out, double *__restrict__ lp_out,
                                                                double *__restrict__ sums_out, int *__restrict__ accept_out,
                                                                long long *__restrict__ evals_out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, d = p.d;
    const size_t e = (size_t)p.first_draw + blockIdx.x;
    const uint32_t draw_id = draw_ids[e];
    const double he = h[e];
    const double *we = w + e * (size_t)p.K * p.n_coef;
    double *fac = lds + lane;                                          // [3 n_slots][64]
    double *xs = fac + (size_t)3 * p.n_slots * OP_LANES;               // [d][64] each: position, proposal, sum, sum of squares
    double *pr = xs + d * OP_LANES;
    double *acc = pr + d * OP_LANES;
    const double *all = xs - lane;                                     // every walker's position: all[i * 64 + walker]

    // lp at the point pt [d][64]: k ascending, then i ascending
    auto target = [&](const double *pt) {
        op_factors<0, false, false>(p.n_slots, slot_var, slot_ord, nullptr, table, p.width, d, box, pt, pt, 0.0, fac);
        double ss = 0.0;
        for (int k = 0; k < p.K; ++k) {
            double f, noise;
            op_terms<0>(p.n_entries, slot_var, entries, long_slots, we + (size_t)k * p.n_coef, 1.0, 1.0, fac, nullptr, nullptr,
                        f, noise);
            const double r = y[k] - f;
            ss = ss + r * r;
        }
        double pp = 0.0;
        for (int i = 0; i < d; ++i) {
            const double dl = pt[i * OP_LANES] - prior[i];
            pp = pp + prior[d + i] * (dl * dl);
        }
        return -he * ss - 0.5 * pp;
    };

    for (int i = 0; i < d; ++i) {
        xs[i * OP_LANES] = starts[(size_t)lane * d + i];
        acc[i * OP_LANES] = 0.0;
        acc[(d + i) * OP_LANES] = 0.0;
    }
    double lp = target(xs);
    long long evals = OP_LANES;
    int accepted_stretch = 0, accepted_jump = 0;
    const int iterations = p.burnin + p.draws, first_half = p.draws / 2;
    double *sums = sums_out + (e * OP_LANES + lane) * (size_t)4 * d;   // [2][2][d]
    __syncthreads();
    for (int t = 0; t < iterations; ++t) {
        const bool jump = p.jump_every > 0 && t % p.jump_every == p.jump_every - 1;
        for (int half = 0; half < 2; ++half) {
            const bool moving = (lane >> 5) == half;
            const int other = INF_HALF * (1 - half);
            const double u1 = inf_uniform(p.seed, draw_id, (uint32_t)t, INF_PURPOSE_PARTNER, (uint32_t)lane);
            const double u2 = inf_uniform(p.seed, draw_id, (uint32_t)t, INF_PURPOSE_STRETCH, (uint32_t)lane);
            const double u3 = inf_uniform(p.seed, draw_id, (uint32_t)t, INF_PURPOSE_ACCEPT, (uint32_t)lane);
            bool inside = true;
            double log_z = 0.0;
            if (!jump) {
                const int j = other + min((int)(32.0 * u1), INF_HALF - 1);
                const double z = ((1.0 + u2) * (1.0 + u2)) * 0.5;
                log_z = (double)(d - 1) * log(z);
                for (int i = 0; i < d; ++i) {
                    const double xj = all[i * OP_LANES + j], xw = xs[i * OP_LANES];
                    const double v = xj + z * (xw - xj);
                    pr[i * OP_LANES] = v;
                    inside = inside && v > box[i] && v < box[d + i];
                }
            } else {
                const int a = min((int)(32.0 * u1), INF_HALF - 1);
                const int b = (a + 1 + min((int)(31.0 * u2), INF_HALF - 2)) % INF_HALF;
                for (int i = 0; i < d; ++i) {
                    const double n = inf_normal(p.seed, draw_id, (uint32_t)t, INF_PURPOSE_JITTER, (uint32_t)(OP_LANES * i + lane));
                    const double xa = all[i * OP_LANES + other + a], xb = all[i * OP_LANES + other + b];
                    const double v = (xs[i * OP_LANES] + (xa - xb)) + (INF_JITTER * (box[d + i] - box[i])) * n;
                    pr[i * OP_LANES] = v;
                    inside = inside && v > box[i] && v < box[d + i];
                }
            }
            const bool evaluated = moving && inside;
            if (!evaluated)                                            // evaluates where it stands; the result is dropped
                for (int i = 0; i < d; ++i) pr[i * OP_LANES] = xs[i * OP_LANES];
            const double lp_y = target(pr);
            const bool accept = evaluated && log(u3) < (log_z + lp_y) - lp;
            evals += __popcll(__ballot(evaluated));
            if (accept) {
                for (int i = 0; i < d; ++i) xs[i * OP_LANES] = pr[i * OP_LANES];
                lp = lp_y;
                accepted_stretch += jump ? 0 : 1;
                accepted_jump += jump ? 1 : 0;
            }
            __syncthreads();                                           // the moves are in place before the other half reads them
        }
        if (t < p.burnin) continue;
        const int r = t - p.burnin;
        if (r == first_half && first_half > 0)
            for (int i = 0; i < 2 * d; ++i) {
                sums[i] = acc[i * OP_LANES];
                acc[i * OP_LANES] = 0.0;
            }
        for (int i = 0; i < d; ++i) {
            const double c = xs[i * OP_LANES] - 0.5 * (box[i] + box[d + i]);
            acc[i * OP_LANES] = acc[i * OP_LANES] + c;
            acc[(d + i) * OP_LANES] = acc[(d + i) * OP_LANES] + c * c;
        }
        if (x_out && r % p.thin == 0) {
            const size_t row = (e * p.kept + (size_t)(r / p.thin)) * OP_LANES + lane;
            for (int i = 0; i < d; ++i) x_out[row * d + i] = xs[i * OP_LANES];
            lp_out[row] = lp;
        }
    }
    for (int i = 0; i < 2 * d; ++i) sums[2 * d + i] = acc[i * OP_LANES];
    accept_out[(e * OP_LANES + lane) * 2] = accepted_stretch;
    accept_out[(e * OP_LANES + lane) * 2 + 1] = accepted_jump;
    if (lane == 0) evals_out[e] = evals;
}

}  // namespace fokl

extern "C" int fokl_infer_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_infer_report: null argument");
    std::memcpy(out, ctx->infer_report, sizeof ctx->infer_report);
    return FOKL_OK;
}

extern "C" int fokl_infer_inputs(fokl_ctx *ctx, int d, int n_terms, const int32_t *mtx_u, int n_draws, const double *betas,
                                 const double *h, const uint32_t *draw_ids, const double *table, int n_basis, int width,
                                 const double *lo, const double *hi, const double *prior_mean, const double *prior_prec, int K,
                                 const double *y, const double *known_prod, const double *starts, int burnin, int draws,
                                 int thin, int jump_every, uint32_t seed, int64_t term_cap, double *x_out, double *lp_out,
                                 double *sums_out, int32_t *accept_out, int64_t *evals_out)
{
    using namespace fokl;
    const std::string who = "fokl_infer_inputs: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->infer_report, 0, sizeof ctx->infer_report);
    if (d < 1 || d > OP_MAX_INPUTS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(d) + " unknown inputs, the kernel is built for 1 to " +
                                           std::to_string(OP_MAX_INPUTS));
    if (K < 1) return fail(ctx, FOKL_ERR_ARG, who + "K = " + std::to_string(K) + " observations, at least 1 is needed");
    if (thin < 1 || draws < 1 || burnin < 0 || jump_every < 0 || draws > (1 << 30) || burnin > (1 << 30))
        return fail(ctx, FOKL_ERR_ARG, who + "thin >= 1, 1 <= draws <= 2^30, 0 <= burnin <= 2^30 and jump_every >= 0 are needed");
    if (n_terms < 0 || n_draws <= 0 || n_basis <= 0 || width <= 0 || term_cap < 0 || (n_terms > 0 && !mtx_u) || !betas || !h ||
        !table || !lo || !hi || !prior_mean || !prior_prec || !y || !known_prod || !starts || !sums_out || !accept_out ||
        !evals_out || (x_out == nullptr) != (lp_out == nullptr))
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer or empty problem (x_out and lp_out are given or left out together)");
    for (int i = 0; i < d; ++i) {
        if (!(lo[i] < hi[i]) || !(std::fabs(lo[i]) <= DBL_MAX) || !(std::fabs(hi[i]) <= DBL_MAX))
            return fail(ctx, FOKL_ERR_ARG, who + "lo < hi, both finite, is needed at unknown " + std::to_string(i) +
                                               " (a fixed input is a known input)");
        if (!(prior_prec[i] >= 0.0) || !(prior_prec[i] <= DBL_MAX) || !(std::fabs(prior_mean[i]) <= DBL_MAX))
            return fail(ctx, FOKL_ERR_ARG, who + "the prior of unknown " + std::to_string(i) +
                                               " needs a finite mean and a finite precision >= 0");
    }
    for (int s = 0; s < OP_LANES; ++s)
        for (int i = 0; i < d; ++i)
            if (!(starts[(size_t)s * d + i] > lo[i] && starts[(size_t)s * d + i] < hi[i]))
                return fail(ctx, FOKL_ERR_ARG, who + "start " + std::to_string(s) + " is not strictly inside the box at unknown " +
                                                   std::to_string(i));
    for (int e = 0; e < n_draws; ++e)
        if (!(h[e] > 0.0) || !(h[e] <= DBL_MAX))
            return fail(ctx, FOKL_ERR_ARG, who + "h[" + std::to_string(e) + "] = 0.5 / sigma^2 must be positive and finite");
    for (int k = 0; k < K; ++k)
        if (!(std::fabs(y[k]) <= DBL_MAX)) return fail(ctx, FOKL_ERR_ARG, who + "y[" + std::to_string(k) + "] is not finite");
    OpTables tables;
    if (!op_pack_model(mtx_u, d, n_terms, nullptr, nullptr, nullptr, n_basis, width, tables))
        return fail(ctx, FOKL_ERR_ARG, who + "basis order outside the coefficient table of " + std::to_string(n_basis) + " orders");
    InfProblem p{};
    p.d = d;
    p.n_slots = (int)tables.slot_var.size();
    p.n_entries = n_terms;
    p.n_coef = n_terms + 1;
    p.width = width;
    p.K = K;
    p.burnin = burnin;
    p.draws = draws;
    p.thin = thin;
    p.kept = (draws + thin - 1) / thin;
    p.jump_every = jump_every;
    p.seed = seed;
    const size_t lds_rows = (size_t)3 * p.n_slots + (size_t)4 * d;
    const size_t lds_bytes = lds_rows * OP_LANES * sizeof(double);
    if (lds_bytes > OP_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(p.n_slots) + " distinct (input, order) factors and " +
                                           std::to_string(d) + " unknowns need " + std::to_string(lds_rows) +
                                           " values per walker, a wavefront's LDS holds " +
                                           std::to_string(OP_LDS_BUDGET / (OP_LANES * sizeof(double))));
    // the draw's coefficients times the known inputs' products: one row per (draw, observation)
    const size_t E = (size_t)n_draws, nc = (size_t)p.n_coef;
    const size_t rows = x_out ? E * p.kept * OP_LANES : 0;
    const size_t want_bytes = (rows * (d + 1) + E * K * nc + E * OP_LANES * 4 * d) * sizeof(double) + E * OP_LANES * 2 * sizeof(int32_t) +
                              E * 24;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_INFER_FREE_BYTES", &free_bytes));
    if (want_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + "the call wants " + std::to_string(want_bytes) + " bytes on the device and 64 MiB to spare (" +
                                           std::to_string(rows * (d + 1) * sizeof(double)) + " bytes of kept rows = draws x kept x 64 x (d + 1) x 8, " +
                                           std::to_string(E * K * nc * sizeof(double)) + " of coefficients = draws x K x (terms + 1) x 8), the device has " +
                                           std::to_string(free_bytes) + " free (thin more, keep no rows, or run the draws in parts)");
    std::vector<double> wk(E * K * nc);
    for (size_t e = 0; e < E; ++e)
        for (size_t k = 0; k < (size_t)K; ++k)
            for (size_t t = 0; t < nc; ++t) {
                const double v = betas[e * nc + t] * known_prod[k * nc + t];
                if (!(std::fabs(v) <= DBL_MAX))
                    return fail(ctx, FOKL_ERR_ARG, who + "NaN or infinity in betas x known_prod at draw " + std::to_string(e) +
                                                       ", observation " + std::to_string(k) + ", coefficient " + std::to_string(t));
                wk[(e * K + k) * nc + t] = v;
            }
    std::vector<uint32_t> ids(E);
    for (size_t e = 0; e < E; ++e) ids[e] = draw_ids ? draw_ids[e] : (uint32_t)e;
    std::vector<double> box(lo, lo + d), prior(prior_mean, prior_mean + d);
    box.insert(box.end(), hi, hi + d);
    prior.insert(prior.end(), prior_prec, prior_prec + d);

    DeviceBuffers buf;
    int *d_var = nullptr, *d_ord = nullptr, *d_long = nullptr, *d_accept = nullptr;
    int4 *d_entries = nullptr;
    uint32_t *d_ids = nullptr;
    long long *d_evals = nullptr;
    double *d_table = nullptr, *d_box = nullptr, *d_prior = nullptr, *d_starts = nullptr, *d_w = nullptr, *d_h = nullptr,
           *d_y = nullptr, *d_x = nullptr, *d_lp = nullptr, *d_sums = nullptr;
    HIP_TRY(ctx, buf.upload(&d_var, tables.slot_var.data(), tables.slot_var.size()));
    HIP_TRY(ctx, buf.upload(&d_ord, tables.slot_ord.data(), tables.slot_ord.size()));
    HIP_TRY(ctx, buf.upload(&d_long, tables.long_slots.data(), tables.long_slots.size()));
    HIP_TRY(ctx, buf.upload(&d_entries, tables.entries.data(), (size_t)n_terms));
    HIP_TRY(ctx, buf.upload(&d_table, table, (size_t)n_basis * width));
    HIP_TRY(ctx, buf.upload(&d_box, box.data(), box.size()));
    HIP_TRY(ctx, buf.upload(&d_prior, prior.data(), prior.size()));
    HIP_TRY(ctx, buf.upload(&d_starts, starts, (size_t)OP_LANES * d));
    HIP_TRY(ctx, buf.upload(&d_w, wk.data(), wk.size()));
    HIP_TRY(ctx, buf.upload(&d_h, h, E));
    HIP_TRY(ctx, buf.upload(&d_y, y, (size_t)K));
    HIP_TRY(ctx, buf.upload(&d_ids, ids.data(), E));
    if (x_out) {
        HIP_TRY(ctx, buf.get(&d_x, rows * d));
        HIP_TRY(ctx, buf.get(&d_lp, rows));
    }
    HIP_TRY(ctx, buf.get(&d_sums, E * OP_LANES * 4 * d));
    HIP_TRY(ctx, buf.get(&d_accept, E * OP_LANES * 2));
    HIP_TRY(ctx, buf.get(&d_evals, E));
    HIP_TRY(ctx, hipMemsetAsync(d_sums, 0, E * OP_LANES * 4 * d * sizeof(double), ctx->stream));

    HIP_TRY(ctx, lds_opt_in(infer_inputs_kernel, lds_bytes, OP_LDS_BUDGET));
    // a launch is asked for at most `cap` term evaluations by a wavefront: whole draws, at least one
    const int64_t iterations = (int64_t)burnin + draws;
    const double per_draw = (2.0 * (double)iterations + 1.0) * (double)K * (double)std::max(1, n_terms);
    const int64_t cap = term_cap ? term_cap : FOKL_INFER_TERM_CAP;
    const int64_t per_launch = (int64_t)std::max(1.0, std::min((double)n_draws, std::floor((double)cap / per_draw)));
    hipError_t err = hipSuccess;
    StreamStopwatch watch(ctx, err);
    const int t0 = watch.mark();
    int64_t launches = 0;
    for (int64_t first = 0; err == hipSuccess && first < n_draws; first += per_launch) {
        const int grid = (int)std::min<int64_t>(per_launch, n_draws - first);
        p.first_draw = (int)first;
        // per evaluation and walker roughly: 6 flops per factor and degree, 4 flops and 3 LDS reads per term and observation
        TimedRegion timed(ctx, FOKL_K_INFER, 8.0 * (double)grid * ((double)p.kept * OP_LANES * (d + 1.0) * (x_out ? 1.0 : 0.0) + (double)K * nc),
                          (double)grid * OP_LANES * per_draw * 4.0);
        hipLaunchKernelGGL(infer_inputs_kernel, dim3(grid), dim3(OP_LANES), lds_bytes, ctx->stream, p, d_var, d_ord, d_entries,
                           d_long, d_table, d_box, d_prior, d_starts, d_w, d_h, d_y, d_ids, d_x, d_lp, d_sums, d_accept, d_evals);
        err = hipGetLastError();
        ++launches;
    }
    const int t1 = watch.mark();
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    const double kernel_us = watch.us(t0, t1);
    if (err == hipSuccess && x_out) err = hipMemcpy(x_out, d_x, rows * d * sizeof(double), hipMemcpyDeviceToHost);
    if (err == hipSuccess && x_out) err = hipMemcpy(lp_out, d_lp, rows * sizeof(double), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(sums_out, d_sums, E * OP_LANES * 4 * d * sizeof(double), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(accept_out, d_accept, E * OP_LANES * 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(evals_out, d_evals, E * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (err != hipSuccess) return fail(ctx, FOKL_ERR_HIP, who + hipGetErrorString(err));

    int64_t evaluations = 0;
    for (size_t e = 0; e < E; ++e) evaluations += evals_out[e];
    int64_t *rep = ctx->infer_report;
    rep[0] = FOKL_INFER_WALKER_PER_LANE;
    rep[1] = (int64_t)lds_rows;
    rep[2] = std::min<int64_t>(per_launch, n_draws);
    rep[3] = launches;
    rep[4] = (int64_t)std::llround(kernel_us);
    rep[5] = iterations;
    rep[6] = evaluations;
    rep[7] = per_launch;
    rep[8] = (int64_t)lds_bytes;
    return FOKL_OK;
}

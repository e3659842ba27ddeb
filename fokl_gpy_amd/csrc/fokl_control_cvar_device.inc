// dynamics.control_cvar (textually included by fokl_hip.hip, after fokl_control_pooled_device.inc): ONE control sequence for
// the whole posterior that protects its bad tail -- the smoothed Rockafellar-Uryasev risk
//     phi(z) = min_a  a + (1 / m) sum_e w_e s_eps(F_e(z) - a),   m = 1 - alpha,
// of dynamics.control's cost over the draws, minimised over one decision vector per start by control_pooled's projected
// Gauss-Newton iteration with phi, the q-weighted noise and g, and H = sum_e q_e H_e + the band draws' covariance of gradients.
//
// The statement of the arithmetic is dynamics.control_cvar_host (fokl_gpy_amd/dynamics.py, module docstring; cvar_smooth is
// the risk).  The tangent and trial launches are control_pooled's kernels as they stand (they take w only to skip a draw of
// weight 0), the accept launch is control_pooled_accept_kernel fed one "chunk" that holds phi per lane, and the stop test,
// Cholesky, trial points and Armijo decision are the __device__ functions of fokl_control_device.inc.  New here: the risk
// kernel, the chunk sums under per-start weights, and the step kernel that adds the covariance term.  Every sum over the draws
// runs in dynamics.pooled_sum's order (chunks of 64 consecutive draws, index order inside a chunk from 0.0, the chunks in
// chunk order from the first, a weight of 0 skipped); min and max are exact in any order.  No atomics.
//
// One iteration is seven launches on the context's stream, without a host round trip (n = 2 + D + D D, n2 = 1 + D + D D):
//   1  control_pooled_tangent_kernel<NS>  rows [s][e][n] = F, noise, g, H of draw e at start s's z
//   2  control_cvar_risk_kernel           grid starts: F_e = rows[s][e][0] -> a [s], phi [s], q [s][e], c [s][e]
//   3  control_cvar_chunk_kernel          one thread per entry: sums [s][chunk][n + n2] = the q-sums of the row entries, then
//                                         the c-sums of 1, g_d and g_d g_d'
//   4  control_cvar_step_kernel           grid starts, one wavefront: the chunk sums in chunk order, the covariance term, then
//                                         control_pooled_step_kernel's text -> the 62 trial points, slope, moved, phi, noise, g
//   5  control_pooled_trial_kernel<NS>    ft [s][e][64]: the cost of draw e at start s's trial point `lane`
//   6  control_cvar_risk_kernel           grid starts x 64: F_e = ft[s][e][lane] -> phi_t [s][lane] (and a_t, unused)
//   7  control_pooled_accept_kernel       with one chunk: the Armijo test on phi_t per lane, the first passing lane
// LDS of 2 and 6: (2 x 64 x ceil(draws / 64) + 2 x threads) x 8 bytes (F and w by [position in chunk][chunk], the exchange
// twice); of 4: (4 + D) x 64 x 8 bytes.  The LDS of 2 and 6 is the limit on the draws: 141 chunks = 9 024 draws with 192
// threads take exactly SIM_LDS_BUDGET, so the kernel's launch bound of 256 threads (256 chunks) is never reached.
// fokl_control_first_trial: as for the pooled solve, with phi_t and a_t of launch 6 in place of the launch-5 chunk sums.

namespace fokl {

constexpr int CTL_CVAR_BISECTIONS = 64;

__device__ __forceinline__ double cvar_clip01(double t) { return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t); }

// Launches 2 and 6: the smoothed risk of the costs F_e = values[(s n_draws + e) stride + column], column = blockIdx.x % columns,
// s = blockIdx.x / columns.  Thread t owns chunk t (draws 64 t .. 64 t + 63); blockDim.x >= n_chunks, a multiple of 64.
// phi, a [starts][columns]; q, c [starts][draws] (or null; only with columns == 1).
__global__ __launch_bounds__(256) void control_cvar_risk_kernel(const double *__restrict__ values, const double *__restrict__ w,
                                                                const int *__restrict__ status, int n_draws, int n_chunks,
                                                                int stride, int columns, double m, double eps,
                                                                double *__restrict__ phi, double *__restrict__ a_out,
                                                                double *__restrict__ q, double *__restrict__ c)
{
    const size_t s = blockIdx.x / (unsigned)columns;
    const int column = (int)(blockIdx.x % (unsigned)columns);
    if (status[s] >= 0) return;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x, T = blockDim.x;
    double *Fl = lds, *wl = Fl + (size_t)CTL_POOL_CHUNK * n_chunks, *ex = wl + (size_t)CTL_POOL_CHUNK * n_chunks;   // ex [2][T]
    // ---- F and w by [position in chunk][chunk]: thread t walks Fl[j n_chunks + t], no two threads on one bank row ----
    for (int k = t; k < CTL_POOL_CHUNK * n_chunks; k += T) {
        const int e = k;                                               // draw e sits at [e % 64][e / 64]
        const int at = (e % CTL_POOL_CHUNK) * n_chunks + e / CTL_POOL_CHUNK;
        const double we = e < n_draws ? w[e] : 0.0;
        wl[at] = we;
        Fl[at] = we != 0.0 ? values[(s * n_draws + e) * (size_t)stride + column] : 0.0;
    }
    __syncthreads();
    const bool mine = t < n_chunks;
    // ---- min, max and finiteness over the live draws ----
    double lo = INFINITY, hi = -INFINITY;
    bool bad = false;
    if (mine)
        for (int j = 0; j < CTL_POOL_CHUNK; ++j) {
            const double we = wl[j * n_chunks + t], F = Fl[j * n_chunks + t];
            if (we == 0.0) continue;
            bad = bad || !(F - F == 0.0);
            lo = F < lo ? F : lo;
            hi = F > hi ? F : hi;
        }
    bad = __syncthreads_or((int)bad) != 0;
    const size_t out = s * columns + column;
    if (bad) {                                                         // block-uniform: phi = a = NaN, q = c = 0
        if (t == 0) {
            phi[out] = NAN;
            a_out[out] = NAN;
        }
        if (q)
            for (int e = t; e < n_draws; e += T) {
                q[s * n_draws + e] = 0.0;
                c[s * n_draws + e] = 0.0;
            }
        return;
    }
    ex[t] = lo;
    ex[T + t] = hi;
    __syncthreads();
    for (int k = 0; k < n_chunks; ++k) {
        lo = ex[k] < lo ? ex[k] : lo;
        hi = ex[T + k] > hi ? ex[T + k] : hi;
    }
    lo = lo - eps;
    __syncthreads();
    // ---- 64 bisections of h(a) = sum_e w_e clip((F_e - a) / eps, 0, 1) = m; every thread keeps the same lo, hi ----
    for (int b = 0; b < CTL_CVAR_BISECTIONS; ++b) {
        const double mid = lo + 0.5 * (hi - lo);
        double *slot = ex + (b & 1) * T;
        if (mine) {
            double acc = 0.0;
            for (int j = 0; j < CTL_POOL_CHUNK; ++j) {
                const double we = wl[j * n_chunks + t];
                if (we == 0.0) continue;
                acc = acc + we * cvar_clip01((Fl[j * n_chunks + t] - mid) / eps);
            }
            slot[t] = acc;
        }
        __syncthreads();                                               // the other slot is free: its readers passed this barrier
        double h = slot[0];
        for (int k = 1; k < n_chunks; ++k) h = h + slot[k];
        if (h > m) lo = mid;
        else hi = mid;
    }
    const double a = hi;
    // ---- phi, and the soft tail weights of the draws ----
    __syncthreads();
    if (mine) {
        double acc = 0.0;
        for (int j = 0; j < CTL_POOL_CHUNK; ++j) {
            const double we = wl[j * n_chunks + t];
            const int e = t * CTL_POOL_CHUNK + j;
            if (we == 0.0) {
                if (q && e < n_draws) {
                    q[s * n_draws + e] = 0.0;
                    c[s * n_draws + e] = 0.0;
                }
                continue;
            }
            const double d = Fl[j * n_chunks + t] - a;
            const double plus = d <= 0.0 ? 0.0 : (d < eps ? (d * d) / (2.0 * eps) : d - 0.5 * eps);
            acc = acc + we * plus;
            if (q) {
                q[s * n_draws + e] = (we * cvar_clip01(d / eps)) / m;
                c[s * n_draws + e] = (d > 0.0 && d < eps) ? we / (m * eps) : 0.0;
            }
        }
        ex[t] = acc;
    }
    __syncthreads();
    if (t == 0) {
        double sum = ex[0];
        for (int k = 1; k < n_chunks; ++k) sum = sum + ex[k];
        phi[out] = a + sum / m;
        a_out[out] = a;
    }
}

// Launch 3: per (start, chunk) the sums under the start's own weights, one thread per entry i of n + n2:
//   i < n                     acc = acc + q_e rows[s][e][i]                     (a draw with q_e == 0 skipped)
//   i = n                     acc = acc + c_e                                   (a draw with c_e == 0 skipped, here and below)
//   i = n + 1 + d             acc = acc + c_e g_d
//   i = n + 1 + D + d D + d'  acc = acc + c_e (g_d g_d')
// sums [starts][chunks][n + n2].  Workgroup (s n_chunks + chunk) blocks_per_row + k.
__global__ __launch_bounds__(CTL_POOL_BLOCK) void control_cvar_chunk_kernel(const double *__restrict__ rows,
                                                                           const double *__restrict__ q,
                                                                           const double *__restrict__ c,
                                                                           const int *__restrict__ status,
                                                                           double *__restrict__ sums, int n_draws, int D,
                                                                           int n_chunks, int blocks_per_row)
{
    const size_t sc = blockIdx.x / (unsigned)blocks_per_row, s = sc / (size_t)n_chunks;
    const int chunk = (int)(sc % (size_t)n_chunks), i = (int)(blockIdx.x % (unsigned)blocks_per_row) * CTL_POOL_BLOCK + (int)threadIdx.x;
    const int n = 2 + D + D * D, total = n + 1 + D + D * D;
    if (status[s] >= 0 || i >= total) return;
    const int first = chunk * CTL_POOL_CHUNK, last = min(n_draws, first + CTL_POOL_CHUNK);
    const int j = i - n;                                               // >= 0: a band sum
    const int pair = j - 1 - D, da = j <= 0 ? 0 : (j <= D ? j - 1 : pair / D), db = j <= D ? -1 : pair % D;
    const double *weight = (j < 0 ? q : c) + s * n_draws;
    double acc = 0.0;
    for (int e = first; e < last; ++e) {
        const double we = weight[e];
        if (we == 0.0) continue;                                       // no multiply, no add: the row may hold anything
        const double *row = rows + (s * n_draws + e) * (size_t)n;
        double x;
        if (j < 0) x = row[i];
        else if (j == 0) x = 1.0;
        else if (db < 0) x = row[2 + da];
        else x = row[2 + da] * row[2 + db];
        acc = acc + we * x;
    }
    sums[sc * (size_t)total + i] = acc;
}

// Launch 4: control_pooled_step_kernel with phi of the risk kernel for F, the q-sums for noise, g and H, and the band draws'
// covariance of gradients added to H: H[d][d'] = Hq[d][d'] + (Scgg[d][d'] - (Scg[d] Scg[d']) / Sc), dropped where Sc == 0.
// phi [starts]; first [starts][n] (or null): phi, noise, g, H of iteration 0
__global__ __launch_bounds__(SIM_LANES) void control_cvar_step_kernel(
    CtlProblem cp, const double *__restrict__ sums, int n_chunks, const double *__restrict__ phi, const double *__restrict__ z,
    int *__restrict__ status, int *__restrict__ iterations, double *__restrict__ cost, double *__restrict__ cost_start,
    int *__restrict__ work, double *__restrict__ trial, double *__restrict__ slope_out, int *__restrict__ moved_out,
    double *__restrict__ pooled, double *__restrict__ first, int it)
{
    const size_t s = blockIdx.x;
    if (status[s] >= 0) return;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, D = cp.D, n = 2 + D + D * D, total = n + 1 + D + D * D;
    double *zs = lds + SIM_LANES, *Hl = lds + 4 * SIM_LANES + lane;    // ctl_pooled_step's layout: Hl[d' * 64] = H[lane][d']
    if (lane == 0) work[it] = 1;
    const double zl = lane < D ? z[s * D + lane] : 0.0;
    zs[lane] = zl;
    // ---- the chunk sums in chunk order from the first ----
    const double *cs = sums + s * (size_t)n_chunks * total;
    const double F = phi[s];
    double noise = cs[1], g = lane < D ? cs[2 + lane] : 0.0, sc = cs[n], scg = lane < D ? cs[n + 1 + lane] : 0.0;
    for (int k = 1; k < n_chunks; ++k) {
        noise = noise + cs[(size_t)k * total + 1];
        sc = sc + cs[(size_t)k * total + n];
        if (lane < D) {
            g = g + cs[(size_t)k * total + 2 + lane];
            scg = scg + cs[(size_t)k * total + n + 1 + lane];
        }
    }
    for (int d2 = 0; d2 < D; ++d2) {
        double h = 0.0;
        if (lane < D) {
            const int at = 2 + D + lane * D + d2, band = n + 1 + D + lane * D + d2;
            h = cs[at];
            double scgg = cs[band], scg2 = cs[n + 1 + d2];
            for (int k = 1; k < n_chunks; ++k) {
                h = h + cs[(size_t)k * total + at];
                scgg = scgg + cs[(size_t)k * total + band];
                scg2 = scg2 + cs[(size_t)k * total + n + 1 + d2];
            }
            if (sc != 0.0) h = h + (scgg - (scg * scg2) / sc);
        }
        Hl[d2 * SIM_LANES] = h;
    }
    ctl_pooled_step(cp, s, lane, it, F, noise, g, zl, lds, status, iterations, cost, cost_start, trial, slope_out, moved_out, pooled,
                    first);
}

}  // namespace fokl

namespace {

enum { CVAR_TANGENT = 0, CVAR_RISK = 1, CVAR_CHUNK = 2, CVAR_STEP = 3, CVAR_TRIAL = 4, CVAR_ACCEPT = 5, CVAR_KINDS = 6 };

}  // namespace

extern "C" int fokl_control_cvar_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_control_cvar_report: null argument");
    std::memcpy(out, ctx->control_cvar_report, sizeof ctx->control_cvar_report);
    return FOKL_OK;
}

extern "C" int fokl_control_cvar_solve(fokl_ctx *ctx, const fokl_system *system, const fokl_control_problem *problem,
                                       const double *draw_weights, double alpha, double smoothing, double epsilon, double *z,
                                       double *cost, double *cost_start, int32_t *status, int32_t *iterations,
                                       int32_t *descent_steps, int32_t *best_start, double *members, int32_t *first_saturation,
                                       double *cost_draws, double *epsilon_used, double *first_pooled, double *first_rows,
                                       double *first_a, double *first_q, double *first_c,
                                       const fokl_control_first_trial *first_trial)
{
    const std::string who = "fokl_control_cvar_solve: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->control_cvar_report, 0, sizeof ctx->control_cvar_report);
    const bool want_first = first_pooled != nullptr;
    const PooledOutputs out{z, cost, cost_start, status, iterations, descent_steps, best_start, members, first_saturation,
                            cost_draws, first_pooled, first_rows};
    if (!system || !problem || !draw_weights || !out.complete() || !epsilon_used || want_first != (first_a != nullptr) ||
        want_first != (first_q != nullptr) || want_first != (first_c != nullptr) ||
        (first_trial && alpha != 0.0 &&
         (!first_trial->trial || !first_trial->slope || !first_trial->moved || !first_trial->pooled || !first_trial->ft ||
          !first_trial->phi_t || !first_trial->a_t || !first_trial->z || !first_trial->status || !first_trial->descent)))
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer, negative size or empty system");
    if (!(alpha >= 0.0 && alpha < 1.0)) return fail(ctx, FOKL_ERR_ARG, who + "alpha must lie in [0, 1), got " + std::to_string(alpha));
    const bool relative = std::isnan(epsilon);                        // NaN: eps = smoothing x the pooled cost of start 0 at z0
    if (!(smoothing > 0) || !std::isfinite(smoothing))
        return fail(ctx, FOKL_ERR_ARG, who + "smoothing must be positive and finite, got " + std::to_string(smoothing));
    if (!relative && (!(epsilon > 0) || !std::isfinite(epsilon)))
        return fail(ctx, FOKL_ERR_ARG, who + "epsilon must be positive and finite (NaN: relative to the cost at the start), got " +
                                           std::to_string(epsilon));
    if (alpha == 0.0) {                                                // q = w, no a, no covariance term: control_pooled itself
        if (want_first) {
            const size_t starts = (size_t)std::max(problem->n_starts, 0), draws = (size_t)std::max(system->n_members, 0);
            for (size_t k = 0; k < starts; ++k) first_a[k] = NAN;
            for (size_t k = 0; k < starts * draws; ++k) {
                first_q[k] = draw_weights[k % draws];
                first_c[k] = 0.0;
            }
        }
        *epsilon_used = epsilon;
        return fokl_control_pooled_solve(ctx, system, problem, draw_weights, z, cost, cost_start, status, iterations, descent_steps,
                                         best_start, members, first_saturation, cost_draws, first_pooled, first_rows, first_trial);
    }
    SimSystem sys{};
    CtlProblem cp{};
    size_t lds_bytes = 0;
    int n_bern_factors = 0;
    if (const int refused = ctl_plan(ctx, who, system, problem, true, sys, cp, lds_bytes, n_bern_factors)) return refused;
    const fokl_system &s = *system;
    const int n_draws = s.n_members, n_states = s.n_states, n_starts = cp.n_starts, max_iter = cp.max_iter;
    if (const int refused = pooled_weights_check(ctx, who, n_draws, draw_weights)) return refused;

    PooledWork k(cp);
    const int D = k.D, n = k.n, n2 = 1 + D + D * D, n_chunks = k.n_chunks;
    const size_t S = k.S, B = k.B;
    const size_t step_lds = (size_t)(4 + D) * SIM_LANES * sizeof(double);
    const int risk_threads = ((n_chunks + SIM_LANES - 1) / SIM_LANES) * SIM_LANES;
    const size_t risk_lds = ((size_t)2 * CTL_POOL_CHUNK * n_chunks + 2 * (size_t)risk_threads) * sizeof(double);
    if (risk_threads > 256 || risk_lds > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG,
                    who + "the risk kernel keeps every draw's cost and weight in LDS: (2 x 64 x ceil(draws / 64) + 2 x threads) x 8 = " +
                        std::to_string(risk_lds) + " bytes for " + std::to_string(n_draws) + " draws, the limit is " +
                        std::to_string(SIM_LDS_BUDGET) + " (solve over fewer draws)");
    const double m = 1.0 - alpha;

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t workspace =
        (B * (size_t)(n + SIM_LANES + 2) + S * n_chunks * (size_t)(n + n2) + S * SIM_LANES * (size_t)(4 + D)) * sizeof(double);
    if (const int refused = pooled_workspace_fits(
            ctx, who, workspace, "FOKL_CONTROL_CVAR_FREE_BYTES",
            std::to_string(n_draws) + " draws x " + std::to_string(n_starts) + " starts x (2 + D + D x D + 64 + 2 = " +
                std::to_string(n + SIM_LANES + 2) + ") x 8, (3 + 2 D + 2 D x D = " + std::to_string(n + n2) +
                ") x 8 per start and chunk of 64 draws: " + std::to_string(n_chunks) + " chunks, and 64 x (4 + D) x 8 per start"))
        return refused;

    DeviceBuffers buf;
    CtlDevice dev{};
    HIP_TRY(ctx, ctl_upload(buf, s, *problem, dev));
    if (const int failed = k.alloc(ctx, buf, s, draw_weights, problem->z0, (size_t)(n + n2), want_first, first_trial != nullptr))
        return failed;
    double *d_phi = nullptr, *d_a = nullptr, *d_phi_t = nullptr, *d_a_t = nullptr, *d_q = nullptr, *d_c = nullptr;
    HIP_TRY(ctx, buf.get(&d_phi, S));
    HIP_TRY(ctx, buf.get(&d_a, S));
    HIP_TRY(ctx, buf.get(&d_phi_t, S * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_a_t, S * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_q, B));
    HIP_TRY(ctx, buf.get(&d_c, B));
    if (first_trial) {
        HIP_TRY(ctx, pooled_fill_nan(d_phi_t, S * SIM_LANES));
        HIP_TRY(ctx, pooled_fill_nan(d_a_t, S * SIM_LANES));
    }
    HIP_TRY(ctx, lds_opt_in(control_cvar_risk_kernel, risk_lds, SIM_LDS_BUDGET));

    const double pass_flops = (double)B * SIM_LANES * (double)s.n_steps * 4.0 * (8.0 * sim_terms_per_stage(sys, n_states) + 20.0 * s.n_factors);
    const int chunk_blocks = (n + n2 + CTL_POOL_BLOCK - 1) / CTL_POOL_BLOCK;
    PooledClock clock(ctx);
    CtlPoll poll;
    int64_t queued = 0;
    hipError_t launched = hipSuccess;
    double eps = epsilon;
    for (int it = 0; it <= max_iter; ++it) {
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (2.0 * (double)B * (n + SIM_LANES)), 3.0 * pass_flops);
            clock.before(CVAR_TANGENT);
            launched = pooled_tangent(ctx, n_states, (int)B, lds_bytes, sys, cp, dev, k.z, k.status, k.w, k.rows);
            clock.after();
            HIP_TRY(ctx, launched);
            if (it == 0 && relative) {
                // the one host read: the pooled cost of start 0 at its z0, in pooled_sum's order, fixes eps for the whole call
                HIP_TRY(ctx, pooled_chunks(ctx, k.rows, k.w, k.status, k.sums, n_draws, 1, n, n_chunks));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                std::vector<double> h_sums((size_t)n_chunks * n);
                HIP_TRY(ctx, hipMemcpy(h_sums.data(), k.sums, h_sums.size() * sizeof(double), hipMemcpyDeviceToHost));
                double at_start = h_sums[0];
                for (int c = 1; c < n_chunks; ++c) at_start = at_start + h_sums[(size_t)c * n];
                if (!std::isfinite(at_start) || at_start == 0.0)
                    return fail(ctx, FOKL_ERR_ARG,
                                who + "smoothing is relative to the pooled cost at the start, which is " + std::to_string(at_start) +
                                    ": with a cost of 0 or a non-finite cost there give epsilon in cost units");
                eps = smoothing * at_start;
            }
            clock.before(CVAR_RISK);
            hipLaunchKernelGGL(control_cvar_risk_kernel, dim3((unsigned)S), dim3(risk_threads), risk_lds, ctx->stream, k.rows, k.w,
                               k.status, n_draws, n_chunks, n, 1, m, eps, d_phi, d_a, d_q, d_c);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(CVAR_CHUNK);
            hipLaunchKernelGGL(control_cvar_chunk_kernel, dim3((unsigned)(S * n_chunks * chunk_blocks)), dim3(CTL_POOL_BLOCK), 0,
                               ctx->stream, k.rows, d_q, d_c, k.status, k.sums, n_draws, D, n_chunks, chunk_blocks);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            if (it == 0 && want_first) {                              // q, c and a of iteration 0, before a later one overwrites them
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                HIP_TRY(ctx, hipMemcpy(first_a, d_a, S * sizeof(double), hipMemcpyDeviceToHost));
                HIP_TRY(ctx, hipMemcpy(first_q, d_q, B * sizeof(double), hipMemcpyDeviceToHost));
                HIP_TRY(ctx, hipMemcpy(first_c, d_c, B * sizeof(double), hipMemcpyDeviceToHost));
            }
            clock.before(CVAR_STEP);
            hipLaunchKernelGGL(control_cvar_step_kernel, dim3((unsigned)S), dim3(SIM_LANES), step_lds, ctx->stream, cp, k.sums,
                               n_chunks, d_phi, k.z, k.status, k.iterations, k.cost, k.cost_start, k.work, k.trial, k.slope, k.moved,
                               k.pooled, k.fpool, it);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(CVAR_TRIAL);
            launched = pooled_trial(ctx, n_states, (int)B, lds_bytes, sys, cp, dev, k.trial, k.status, k.w, k.ft);
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(CVAR_RISK);
            hipLaunchKernelGGL(control_cvar_risk_kernel, dim3((unsigned)(S * SIM_LANES)), dim3(risk_threads), risk_lds, ctx->stream,
                               k.ft, k.w, k.status, n_draws, n_chunks, SIM_LANES, SIM_LANES, m, eps, d_phi_t, d_a_t,
                               (double *)nullptr, (double *)nullptr);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(CVAR_ACCEPT);
            hipLaunchKernelGGL(control_pooled_accept_kernel, dim3((unsigned)S), dim3(SIM_LANES), 0, ctx->stream, D, d_phi_t, 1,
                               k.trial, k.slope, k.moved, k.pooled, k.z, k.status, k.iterations, k.descent, it);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            ++queued;
        }
        if (it == 0 && first_trial) {
            if (const int failed = k.first_trial_out(ctx, *first_trial)) return failed;
            HIP_TRY(ctx, hipMemcpy(first_trial->phi_t, d_phi_t, S * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->a_t, d_a_t, S * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
        }
        bool stopped = false;
        if (const int failed = poll(ctx, it, max_iter, k.status, S, stopped)) return failed;
        if (stopped) break;
    }
    *epsilon_used = eps;
    int64_t worked = 0;
    if (const int failed = k.finish(ctx, who, s, sys, cp, lds_bytes, dev, pass_flops, out, worked)) return failed;
    int64_t *rep = ctx->control_cvar_report;
    k.report_head(rep, n_states, lds_bytes, step_lds);
    rep[7] = (int64_t)risk_lds;
    rep[8] = risk_threads;
    rep[9] = queued;
    rep[10] = worked;
    rep[11] = 7;
    clock.read(rep + 12);
    return FOKL_OK;
}

// dynamics.control_pooled (textually included by fokl_hip.hip, after fokl_control_device.inc): ONE control sequence for the
// whole posterior -- the expected cost F(z) = sum_e w_e F_e(z) of dynamics.control's cost over the draws, minimised over one
// decision vector per start by the same projected Gauss-Newton iteration with g = sum_e w_e g_e and H = sum_e w_e H_e.
//
// The statement of the arithmetic is dynamics.control_pooled_host (fokl_gpy_amd/dynamics.py, module docstring).  The
// tangent pass, the stop test, the Cholesky and its solves, the trial points and the Armijo decision are the __device__
// functions of fokl_control_device.inc, the very text control_iterate_kernel runs; what is new here is the coupling of the
// draws: the pooled sum (dynamics.pooled_sum) between the tangent pass and the Newton step, and again between the trial
// pass and the Armijo decision.  The sum's order is fixed by the draw index alone -- chunks of 64 consecutive draws, inside
// a chunk acc = acc + w_e x_e in index order from 0.0, the chunk sums added in chunk order from the first, a draw of weight
// 0 skipped entirely -- so no launch shape changes a bit, and there are no atomics.
//
// One iteration is six launches on the context's stream, without a host round trip (s = start, e = draw, n = 2 + D + D D):
//   1  control_pooled_tangent_kernel<NS>  grid draws x starts, one wavefront: the tangent pass of draw e at start s's z ->
//                                         rows [s][e][n] = F, noise, g [D], H [D][D] (entry [d][d'] as lane d forms it)
//   2  control_pooled_chunk_kernel        one thread per entry: rows [s][e][n] -> sums [s][chunk][n]
//   3  control_pooled_step_kernel         grid starts, one wavefront: the chunk sums in chunk order, stop test, active set,
//                                         Cholesky, the two solves -> the 62 trial points [s][d][lane], slope, moved, F, noise, g
//   4  control_pooled_trial_kernel<NS>    grid draws x starts, lane = trial: the value pass of draw e at the lane's point ->
//                                         Ft rows [s][e][64]
//   5  control_pooled_chunk_kernel        with n = 64
//   6  control_pooled_accept_kernel       grid starts: chunk-order sum, Armijo test per lane, ballot, the first passing lane ->
//                                         the new z, the descent count, or status 3
// A finished start (status >= 0) and, in 1 and 4, a draw of weight 0 return at once.  LDS of 1 and 4: control's formula;
// of 3: (4 + D) x 64 x 8 bytes (exchange, z, g, direction, H as [D][64]).
// For tests the host half can hand out what iteration 0 left in these buffers after launch 6 (fokl_control_first_trial in
// fokl_hip_internal.h): one more stream synchronisation and host copies, no other launch and no change to a kernel.

namespace fokl {

constexpr int CTL_POOL_CHUNK = 64;
constexpr int CTL_POOL_BLOCK = 256;            // threads of a chunk-sum workgroup

// Launch 1.  z [starts][D]; status [starts]; w [draws]; rows [starts][draws][2 + D + D D]
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void control_pooled_tangent_kernel(
    SimSystem sys, CtlProblem cp, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const int *__restrict__ norm_control, const int *__restrict__ seg_first,
    const double *__restrict__ ref, const double *__restrict__ coef, const double *__restrict__ forcing,
    const double *__restrict__ y0, const double *__restrict__ z, const int *__restrict__ status, const double *__restrict__ w,
    double *__restrict__ rows)
{
    const size_t b = blockIdx.x, s = b / (size_t)cp.n_draws, e = b % (size_t)cp.n_draws;
    if (status[s] >= 0 || w[e] == 0.0) return;
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    const CtlTables ct{norm_control, seg_first, ref};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, D = cp.D;
    const CtlLds l = ctl_lds(lds, sys, D, lane);
    double *Hl = l.H + lane;
    ctl_tangent_load(sys, l, Hl, D, lane, coef + e * sys.n_coef, z + s * D);
    double y0r[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0r[j] = y0[(size_t)j * cp.n_draws + e];
    double F, noise, g;
    ctl_tangent_pass<NS>(sys, cp, tab, ct, forcing, l, Hl, y0r, lane, F, noise, g);
    double *row = rows + b * (size_t)(2 + D + D * D);
    if (lane == 0) {
        row[0] = F;
        row[1] = noise;
    }
    if (lane < D) {
        row[2 + lane] = g;
        for (int d2 = 0; d2 < D; ++d2) row[2 + D + lane * D + d2] = Hl[d2 * SIM_LANES];
    }
}

// Launches 2 and 5: the weighted chunk sums of rows [starts][draws][n] -> sums [starts][chunks][n], one thread per entry
// (coalesced across the entries), the draws of the chunk in index order.  Workgroup (s n_chunks + chunk) blocks_per_row + k.
__global__ __launch_bounds__(CTL_POOL_BLOCK) void control_pooled_chunk_kernel(const double *__restrict__ rows,
                                                                             const double *__restrict__ w,
                                                                             const int *__restrict__ status,
                                                                             double *__restrict__ sums, int n_draws, int n,
                                                                             int n_chunks, int blocks_per_row)
{
    const size_t sc = blockIdx.x / (unsigned)blocks_per_row, s = sc / (size_t)n_chunks;
    const int chunk = (int)(sc % (size_t)n_chunks), i = (int)(blockIdx.x % (unsigned)blocks_per_row) * CTL_POOL_BLOCK + (int)threadIdx.x;
    if (status[s] >= 0 || i >= n) return;
    const int first = chunk * CTL_POOL_CHUNK, last = min(n_draws, first + CTL_POOL_CHUNK);
    double acc = 0.0;
    for (int e = first; e < last; ++e) {
        const double we = w[e];
        if (we == 0.0) continue;                                       // no multiply, no add: the row may hold anything
        acc = acc + we * rows[(s * n_draws + e) * (size_t)n + i];
    }
    sums[sc * (size_t)n + i] = acc;
}

// What control_pooled_step_kernel and control_cvar_step_kernel do for start s once its F, noise, g (lane d: g[d]) and H (lane
// d: row d, in the LDS layout below) are formed: iteration 0's record, the stop test, the Newton direction, the trial points.
// lds: exchange, z, g, direction [64] each, then H as [D][64]; z is there already.
__device__ __forceinline__ void ctl_pooled_step(const CtlProblem &cp, size_t s, int lane, int it, double F, double noise, double g,
                                                double zl, double *lds, int *__restrict__ status, int *__restrict__ iterations,
                                                double *__restrict__ cost, double *__restrict__ cost_start,
                                                double *__restrict__ trial, double *__restrict__ slope_out,
                                                int *__restrict__ moved_out, double *__restrict__ pooled,
                                                double *__restrict__ first)
{
    const int D = cp.D, n = 2 + D + D * D;
    double *ex = lds, *zs = ex + SIM_LANES, *gs = zs + SIM_LANES, *ds = gs + SIM_LANES, *H = ds + SIM_LANES;
    double *Hl = H + lane;                                             // Hl[d' * 64] = H[lane][d']
    if (it == 0) {
        if (lane == 0) cost_start[s] = F;
        if (first) {
            double *row = first + s * (size_t)n;
            if (lane == 0) {
                row[0] = F;
                row[1] = noise;
            }
            if (lane < D) {
                row[2 + lane] = g;
                for (int d2 = 0; d2 < D; ++d2) row[2 + D + lane * D + d2] = Hl[d2 * SIM_LANES];
            }
        }
    }
    if (lane == 0) cost[s] = F;
    __syncthreads();

    const int code = ctl_stop_code(cp, F, g, zl, lane, it);
    if (code >= 0) {
        if (lane == 0) {
            status[s] = code;
            iterations[s] = it;
        }
        return;
    }
    ctl_newton_direction(H, ex, gs, ds, D, lane, zl, g);
    double slope;
    bool moved;
    const bool valid = ctl_trial_points(zs, gs, ds, Hl, D, lane, slope, moved);
    for (int d = 0; d < D; ++d) trial[(s * D + d) * SIM_LANES + lane] = Hl[d * SIM_LANES];
    slope_out[s * SIM_LANES + lane] = slope;
    moved_out[s * SIM_LANES + lane] = (valid && moved) ? 1 : 0;
    if (lane == 0) {
        pooled[s * (2 + D)] = F;
        pooled[s * (2 + D) + 1] = noise;
    }
    if (lane < D) pooled[s * (2 + D) + 2 + lane] = g;
}

// Launch 3.  sums [starts][chunks][n]; trial [starts][D][64]; slope [starts][64]; moved [starts][64] (the lane is a trial
// AND moves z); pooled [starts][2 + D] = F, noise, g; first [starts][n] (or null): the pooled row of iteration 0
__global__ __launch_bounds__(SIM_LANES) void control_pooled_step_kernel(
    CtlProblem cp, const double *__restrict__ sums, int n_chunks, const double *__restrict__ z, int *__restrict__ status,
    int *__restrict__ iterations, double *__restrict__ cost, double *__restrict__ cost_start, int *__restrict__ work,
    double *__restrict__ trial, double *__restrict__ slope_out, int *__restrict__ moved_out, double *__restrict__ pooled,
    double *__restrict__ first, int it)
{
    const size_t s = blockIdx.x;
    if (status[s] >= 0) return;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, D = cp.D, n = 2 + D + D * D;
    double *zs = lds + SIM_LANES, *Hl = lds + 4 * SIM_LANES + lane;    // ctl_pooled_step's layout: Hl[d' * 64] = H[lane][d']
    if (lane == 0) work[it] = 1;
    const double zl = lane < D ? z[s * D + lane] : 0.0;
    zs[lane] = zl;
    // ---- the chunk sums in chunk order from the first ----
    const double *cs = sums + s * (size_t)n_chunks * n;
    double F = cs[0], noise = cs[1], g = lane < D ? cs[2 + lane] : 0.0;
    for (int c = 1; c < n_chunks; ++c) {
        F = F + cs[(size_t)c * n];
        noise = noise + cs[(size_t)c * n + 1];
        if (lane < D) g = g + cs[(size_t)c * n + 2 + lane];
    }
    for (int d2 = 0; d2 < D; ++d2) {
        double h = 0.0;
        if (lane < D) {
            h = cs[2 + D + lane * D + d2];
            for (int c = 1; c < n_chunks; ++c) h = h + cs[(size_t)c * n + 2 + D + lane * D + d2];
        }
        Hl[d2 * SIM_LANES] = h;
    }
    ctl_pooled_step(cp, s, lane, it, F, noise, g, zl, lds, status, iterations, cost, cost_start, trial, slope_out, moved_out, pooled,
                    first);
}

// Launch 4 (and, with w null, one start and every lane at the same point, the draws' own costs at the returned controls).
// trial [starts][D][64]; ft [starts][draws][64]
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void control_pooled_trial_kernel(
    SimSystem sys, CtlProblem cp, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const int *__restrict__ norm_control, const int *__restrict__ seg_first,
    const double *__restrict__ ref, const double *__restrict__ coef, const double *__restrict__ forcing,
    const double *__restrict__ y0, const double *__restrict__ trial, const int *__restrict__ status,
    const double *__restrict__ w, double *__restrict__ ft)
{
    const size_t b = blockIdx.x, s = b / (size_t)cp.n_draws, e = b % (size_t)cp.n_draws;
    if (status[s] >= 0 || (w && w[e] == 0.0)) return;
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    const CtlTables ct{norm_control, seg_first, ref};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, D = cp.D;
    const CtlLds l = ctl_lds(lds, sys, D, lane);
    double *Hl = l.H + lane;
    l.fac[0] = 1.0;
    for (int c = lane; c < sys.n_coef; c += SIM_LANES) l.cf[c] = coef[e * sys.n_coef + c];
    for (int d = 0; d < D; ++d) Hl[d * SIM_LANES] = trial[(s * D + d) * SIM_LANES + lane];
    __syncthreads();
    double y0r[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0r[j] = y0[(size_t)j * cp.n_draws + e];
    int unused = 0;
    ft[b * SIM_LANES + lane] = ctl_value_pass<NS>(sys, cp, tab, ct, forcing, l.xn, l.fac, l.cf, Hl, y0r, lane, nullptr, unused);
}

// Launch 6.  ft_sums [starts][chunks][64]
__global__ __launch_bounds__(SIM_LANES) void control_pooled_accept_kernel(
    int D, const double *__restrict__ ft_sums, int n_chunks, const double *__restrict__ trial, const double *__restrict__ slope,
    const int *__restrict__ moved, const double *__restrict__ pooled, double *__restrict__ z, int *__restrict__ status,
    int *__restrict__ iterations, int *__restrict__ descent, int it)
{
    const size_t s = blockIdx.x;
    if (status[s] >= 0) return;
    const int lane = threadIdx.x;
    const double *cs = ft_sums + s * (size_t)n_chunks * SIM_LANES;
    double Ft = cs[lane];
    for (int c = 1; c < n_chunks; ++c) Ft = Ft + cs[(size_t)c * SIM_LANES + lane];
    const double F = pooled[s * (2 + D)], noise = pooled[s * (2 + D) + 1];
    const int taken = ctl_first_passing(moved[s * SIM_LANES + lane] != 0, true, Ft, F, slope[s * SIM_LANES + lane], noise);
    if (taken < 0) {
        if (lane == 0) {
            status[s] = CTL_STALLED;
            iterations[s] = it;
        }
        return;
    }
    if (lane < D) z[s * D + lane] = trial[(s * D + lane) * SIM_LANES + taken];
    if (lane == 0 && taken >= 32) descent[s] = descent[s] + 1;
}

}  // namespace fokl

namespace {

enum { POOLED_TANGENT = 0, POOLED_CHUNK = 1, POOLED_STEP = 2, POOLED_TRIAL = 3, POOLED_ACCEPT = 4, POOLED_KINDS = 5 };

// The launches' own events while the context times its kernels: nanoseconds per kind of kernel into the report
struct PooledClock {
    fokl_ctx *ctx;
    struct Stamp {
        int kind;
        hipEvent_t start, stop;
    };
    std::vector<Stamp> stamps;
    explicit PooledClock(fokl_ctx *c) : ctx(c) {}
    ~PooledClock()
    {
        for (const Stamp &s : stamps) {
            ctx->event_pool.push_back(s.start);
            ctx->event_pool.push_back(s.stop);
        }
    }
    void before(int kind)
    {
        if (!ctx->timing) return;
        hipEvent_t a = take_event(ctx), b = take_event(ctx);
        if (!a || !b) return;
        (void)hipEventRecord(a, ctx->stream);
        stamps.push_back({kind, a, b});
    }
    void after()
    {
        if (!ctx->timing || stamps.empty()) return;
        (void)hipEventRecord(stamps.back().stop, ctx->stream);
    }
    void read(int64_t *ns) const                                       // after the stream was synchronised
    {
        for (const Stamp &s : stamps) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.start, s.stop) == hipSuccess) ns[s.kind] += (int64_t)((double)ms * 1e6);
        }
    }
};

hipError_t pooled_tangent(fokl_ctx *ctx, int n_states, int grid, size_t lds_bytes, const SimSystem &sys, const CtlProblem &cp,
                          const CtlDevice &d, const double *z, const int *status, const double *w, double *rows)
{
    return sim_dispatch(n_states, [&](auto ns) {
        const auto kernel = control_pooled_tangent_kernel<decltype(ns)::value>;
        if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, cp, d.tab.norm_src, d.tab.norm_lo,
                           d.tab.norm_span, d.tab.fac_norm, d.tab.fac_row, d.tab.fac_degree, d.tab.entries, d.tab.spline, d.tab.bern,
                           d.ct.norm_control, d.ct.seg_first, d.ct.ref, (const double *)d.coef, (const double *)d.forcing,
                           (const double *)d.y0, z, status, w, rows);
        return hipGetLastError();
    });
}

hipError_t pooled_trial(fokl_ctx *ctx, int n_states, int grid, size_t lds_bytes, const SimSystem &sys, const CtlProblem &cp,
                        const CtlDevice &d, const double *trial, const int *status, const double *w, double *ft)
{
    return sim_dispatch(n_states, [&](auto ns) {
        const auto kernel = control_pooled_trial_kernel<decltype(ns)::value>;
        if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, cp, d.tab.norm_src, d.tab.norm_lo,
                           d.tab.norm_span, d.tab.fac_norm, d.tab.fac_row, d.tab.fac_degree, d.tab.entries, d.tab.spline, d.tab.bern,
                           d.ct.norm_control, d.ct.seg_first, d.ct.ref, (const double *)d.coef, (const double *)d.forcing,
                           (const double *)d.y0, trial, status, w, ft);
        return hipGetLastError();
    });
}

// For the first_trial outputs: NaN into a buffer that iteration 0 may leave unwritten in places
hipError_t pooled_fill_nan(double *d, size_t count)
{
    const std::vector<double> h(count, NAN);
    return hipMemcpy(d, h.data(), count * sizeof(double), hipMemcpyHostToDevice);
}

hipError_t pooled_chunks(fokl_ctx *ctx, const double *rows, const double *w, const int *status, double *sums, int n_draws,
                         int n_starts, int n, int n_chunks)
{
    const int blocks_per_row = (n + CTL_POOL_BLOCK - 1) / CTL_POOL_BLOCK;
    hipLaunchKernelGGL(control_pooled_chunk_kernel, dim3((unsigned)((size_t)n_starts * n_chunks * blocks_per_row)),
                       dim3(CTL_POOL_BLOCK), 0, ctx->stream, rows, w, status, sums, n_draws, n, n_chunks, blocks_per_row);
    return hipGetLastError();
}

// The outputs fokl_control_pooled_solve and fokl_control_cvar_solve share
struct PooledOutputs {
    double *z, *cost, *cost_start;
    int32_t *status, *iterations, *descent_steps, *best_start;
    double *members;
    int32_t *first_saturation;
    double *cost_draws, *first_pooled, *first_rows;
    bool complete() const
    {
        return z && cost && cost_start && status && iterations && descent_steps && best_start && members && first_saturation &&
               cost_draws && (first_pooled == nullptr) == (first_rows == nullptr);
    }
};

int pooled_weights_check(fokl_ctx *ctx, const std::string &who, int n_draws, const double *draw_weights)
{
    double weight_sum = 0.0;
    for (int e = 0; e < n_draws; ++e) {
        if (!(draw_weights[e] >= 0) || !std::isfinite(draw_weights[e]))
            return fail(ctx, FOKL_ERR_ARG, who + "draw weights must be non-negative and finite");
        weight_sum += draw_weights[e];
    }
    if (!(weight_sum > 0)) return fail(ctx, FOKL_ERR_ARG, who + "the draw weights sum to zero: at least one draw must weigh something");
    return FOKL_OK;
}

// What both solves keep on the device (S starts, E draws, B = E S, n = 2 + D + D D): the state of the starts, the draws'
// rows and trial costs, the step kernel's outputs, and the buffers of the closing trajectory.  sums is [S][chunks][sums_width].
struct PooledWork {
    int D, n, n_chunks;
    size_t E, S, B;
    int *status = nullptr, *iterations = nullptr, *descent = nullptr, *work = nullptr, *first = nullptr, *moved = nullptr,
        *running = nullptr;
    double *w = nullptr, *z = nullptr, *cost = nullptr, *cost_start = nullptr, *rows = nullptr, *sums = nullptr, *ft = nullptr,
           *trial = nullptr, *slope = nullptr, *pooled = nullptr, *fpool = nullptr, *zbest = nullptr, *members = nullptr;
    std::vector<int32_t> h_work;

    PooledWork(const CtlProblem &cp)
        : D(cp.D), n(2 + cp.D + cp.D * cp.D), n_chunks((cp.n_draws + CTL_POOL_CHUNK - 1) / CTL_POOL_CHUNK), E((size_t)cp.n_draws),
          S((size_t)cp.n_starts), B(E * S), h_work((size_t)cp.max_iter + 1, 0)
    {
    }

    // want_first: rows and the pooled row of iteration 0 are read back (a draw of weight 0 writes no row: it reads NaN);
    // fill_trial: what iteration 0 does not write of the first_trial fields kept here reads NaN, moved 0
    int alloc(fokl_ctx *ctx, DeviceBuffers &buf, const fokl_system &s, const double *draw_weights, const double *z0,
              size_t sums_width, bool want_first, bool fill_trial)
    {
        const std::vector<int32_t> h_status(S, -1), h_none(S, 0);
        const std::vector<double> h_nan(S, NAN);
        HIP_TRY(ctx, buf.upload(&w, draw_weights, E));
        HIP_TRY(ctx, buf.upload(&z, z0, S * D));
        HIP_TRY(ctx, buf.upload(&status, h_status.data(), S));
        HIP_TRY(ctx, buf.upload(&iterations, h_status.data(), S));
        HIP_TRY(ctx, buf.upload(&descent, h_none.data(), S));
        HIP_TRY(ctx, buf.upload(&cost, h_nan.data(), S));
        HIP_TRY(ctx, buf.upload(&cost_start, h_nan.data(), S));
        HIP_TRY(ctx, buf.upload(&work, h_work.data(), h_work.size()));
        HIP_TRY(ctx, buf.upload(&running, h_status.data(), 1));
        HIP_TRY(ctx, buf.get(&rows, B * n));
        HIP_TRY(ctx, buf.get(&sums, S * n_chunks * sums_width));
        HIP_TRY(ctx, buf.get(&ft, B * SIM_LANES));
        HIP_TRY(ctx, buf.get(&trial, S * D * SIM_LANES));
        HIP_TRY(ctx, buf.get(&slope, S * SIM_LANES));
        HIP_TRY(ctx, buf.get(&moved, S * SIM_LANES));
        HIP_TRY(ctx, buf.get(&pooled, S * (2 + D)));
        if (want_first) {
            HIP_TRY(ctx, pooled_fill_nan(rows, B * n));
            HIP_TRY(ctx, buf.get(&fpool, S * n));
        }
        if (fill_trial) {
            HIP_TRY(ctx, pooled_fill_nan(trial, S * D * SIM_LANES));
            HIP_TRY(ctx, pooled_fill_nan(slope, S * SIM_LANES));
            HIP_TRY(ctx, pooled_fill_nan(pooled, S * (2 + D)));
            HIP_TRY(ctx, pooled_fill_nan(ft, B * SIM_LANES));
            HIP_TRY(ctx, hipMemset(moved, 0, S * SIM_LANES * sizeof(int)));
        }
        HIP_TRY(ctx, buf.get(&zbest, E * D));
        HIP_TRY(ctx, buf.get(&members, E * s.n_states * (s.n_steps + 1)));
        HIP_TRY(ctx, buf.get(&first, E));
        return FOKL_OK;
    }

    // Iteration 0's trial half, before a later one overwrites it: the fields both solves fill
    int first_trial_out(fokl_ctx *ctx, const fokl_control_first_trial &t) const
    {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(t.trial, trial, S * D * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(t.slope, slope, S * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(t.moved, moved, S * SIM_LANES * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(t.pooled, pooled, S * (2 + D) * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(t.ft, ft, B * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(t.z, z, S * D * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(t.status, status, S * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(t.descent, descent, S * sizeof(int32_t), hipMemcpyDeviceToHost));
        return FOKL_OK;
    }

    // After the last iteration: the starts' results, the best start, every draw's trajectory and own cost under its controls
    // (one start -- `running` holds -1 -- and no weights: every draw's value pass at the returned point, lane 0 is read).
    // worked: the iterations that found a running start.
    int finish(fokl_ctx *ctx, const std::string &who, const fokl_system &s, const SimSystem &sys, const CtlProblem &cp,
               size_t lds_bytes, const CtlDevice &dev, double pass_flops, const PooledOutputs &out, int64_t &worked)
    {
        const int64_t n_points = s.n_steps + 1;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(out.z, z, S * D * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.cost, cost, S * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.cost_start, cost_start, S * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.status, status, S * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.iterations, iterations, S * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.descent_steps, descent, S * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(h_work.data(), work, h_work.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (out.first_pooled) {
            HIP_TRY(ctx, hipMemcpy(out.first_pooled, fpool, S * n * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(out.first_rows, rows, B * n * sizeof(double), hipMemcpyDeviceToHost));
        }
        for (size_t k = 0; k < S; ++k)
            if (out.status[k] < 0) return fail(ctx, FOKL_ERR_HIP, who + "a solve was left running");
        worked = 0;
        for (int32_t found : h_work) worked += found;

        const int best = ctl_best_start(out.cost, out.status, (int)S);
        *out.best_start = best;
        std::vector<double> z_best(E * D), point((size_t)D * SIM_LANES);
        for (size_t e = 0; e < E; ++e) std::memcpy(z_best.data() + e * D, out.z + (size_t)best * D, D * sizeof(double));
        for (int d = 0; d < D; ++d)
            for (int lane = 0; lane < SIM_LANES; ++lane) point[(size_t)d * SIM_LANES + lane] = out.z[(size_t)best * D + d];
        HIP_TRY(ctx, hipMemcpy(zbest, z_best.data(), E * D * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(trial, point.data(), point.size() * sizeof(double), hipMemcpyHostToDevice));
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)E * s.n_states * n_points, 2.0 * pass_flops / (double)S);
            HIP_TRY(ctx, ctl_trajectory(ctx, s.n_states, (int)E, lds_bytes, sys, cp, dev, zbest, members, first));
            HIP_TRY(ctx, pooled_trial(ctx, s.n_states, (int)E, lds_bytes, sys, cp, dev, trial, running, nullptr, ft));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(out.members, members, E * s.n_states * n_points * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.first_saturation, first, E * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<double> h_ft(E * SIM_LANES);
        HIP_TRY(ctx, hipMemcpy(h_ft.data(), ft, h_ft.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < E; ++e) out.cost_draws[e] = h_ft[e * SIM_LANES];
        return FOKL_OK;
    }

    // out[0 .. 6] of both reports
    void report_head(int64_t *rep, int n_states, size_t lds_bytes, size_t step_lds) const
    {
        rep[0] = n_states;
        rep[1] = (int64_t)E;
        rep[2] = (int64_t)S;
        rep[3] = D;
        rep[4] = n_chunks;
        rep[5] = (int64_t)lds_bytes;
        rep[6] = (int64_t)step_lds;
    }
};

// The workspace against the device's free memory, of which the environment variable `cap_env` caps what counts;
// `what` spells the workspace out for the refusal
int pooled_workspace_fits(fokl_ctx *ctx, const std::string &who, size_t workspace, const char *cap_env, const std::string &what)
{
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes(cap_env, &free_bytes));
    if (workspace > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + "the workspace needs " + std::to_string(workspace) + " bytes (" + what + "), the device has " +
                                           std::to_string(free_bytes) + " free (" + cap_env +
                                           " caps what counts; solve over fewer draws or starts)");
    return FOKL_OK;
}

}  // namespace

extern "C" int fokl_control_pooled_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_control_pooled_report: null argument");
    std::memcpy(out, ctx->control_pooled_report, sizeof ctx->control_pooled_report);
    return FOKL_OK;
}

extern "C" int fokl_control_pooled_solve(fokl_ctx *ctx, const fokl_system *system, const fokl_control_problem *problem,
                                         const double *draw_weights, double *z, double *cost, double *cost_start,
                                         int32_t *status, int32_t *iterations, int32_t *descent_steps, int32_t *best_start,
                                         double *members, int32_t *first_saturation, double *cost_draws, double *first_pooled,
                                         double *first_rows, const fokl_control_first_trial *first_trial)
{
    const std::string who = "fokl_control_pooled_solve: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->control_pooled_report, 0, sizeof ctx->control_pooled_report);
    const PooledOutputs out{z, cost, cost_start, status, iterations, descent_steps, best_start, members, first_saturation,
                            cost_draws, first_pooled, first_rows};
    const bool outputs_ok =
        draw_weights && out.complete() &&
        (!first_trial || (first_trial->trial && first_trial->slope && first_trial->moved && first_trial->pooled && first_trial->ft &&
                          first_trial->ft_sums && first_trial->z && first_trial->status && first_trial->descent));
    SimSystem sys{};
    CtlProblem cp{};
    size_t lds_bytes = 0;
    int n_bern_factors = 0;
    if (const int refused = ctl_plan(ctx, who, system, problem, outputs_ok, sys, cp, lds_bytes, n_bern_factors)) return refused;
    const fokl_system &s = *system;
    const int n_draws = s.n_members, n_states = s.n_states, n_starts = cp.n_starts, max_iter = cp.max_iter;
    if (const int refused = pooled_weights_check(ctx, who, n_draws, draw_weights)) return refused;

    PooledWork k(cp);
    const int D = k.D, n = k.n, n_chunks = k.n_chunks;
    const size_t S = k.S, B = k.B;
    const size_t step_lds = (size_t)(4 + D) * SIM_LANES * sizeof(double);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t workspace = (B * (size_t)(n + SIM_LANES) + S * n_chunks * (size_t)(n + SIM_LANES)) * sizeof(double);
    if (const int refused = pooled_workspace_fits(
            ctx, who, workspace, "FOKL_CONTROL_POOLED_FREE_BYTES",
            std::to_string(n_draws) + " draws x " + std::to_string(n_starts) + " starts x (2 + D + D x D + 64 = " +
                std::to_string(n + SIM_LANES) + ") x 8, and as much per chunk of 64 draws: " + std::to_string(n_chunks) + " chunks"))
        return refused;

    DeviceBuffers buf;
    CtlDevice dev{};
    HIP_TRY(ctx, ctl_upload(buf, s, *problem, dev));
    if (const int failed = k.alloc(ctx, buf, s, draw_weights, problem->z0, (size_t)n, first_pooled != nullptr, first_trial != nullptr))
        return failed;
    double *d_ft_sums = nullptr;
    HIP_TRY(ctx, buf.get(&d_ft_sums, S * n_chunks * SIM_LANES));
    if (first_trial) HIP_TRY(ctx, pooled_fill_nan(d_ft_sums, S * n_chunks * SIM_LANES));

    const double pass_flops = (double)B * SIM_LANES * (double)s.n_steps * 4.0 * (8.0 * sim_terms_per_stage(sys, n_states) + 20.0 * s.n_factors);
    PooledClock clock(ctx);
    CtlPoll poll;
    int64_t queued = 0;
    hipError_t launched = hipSuccess;
    for (int it = 0; it <= max_iter; ++it) {
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (2.0 * (double)B * (n + SIM_LANES)), 3.0 * pass_flops);
            clock.before(POOLED_TANGENT);
            launched = pooled_tangent(ctx, n_states, (int)B, lds_bytes, sys, cp, dev, k.z, k.status, k.w, k.rows);
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_CHUNK);
            launched = pooled_chunks(ctx, k.rows, k.w, k.status, k.sums, n_draws, n_starts, n, n_chunks);
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_STEP);
            hipLaunchKernelGGL(control_pooled_step_kernel, dim3((unsigned)S), dim3(SIM_LANES), step_lds, ctx->stream, cp, k.sums,
                               n_chunks, k.z, k.status, k.iterations, k.cost, k.cost_start, k.work, k.trial, k.slope, k.moved,
                               k.pooled, k.fpool, it);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_TRIAL);
            launched = pooled_trial(ctx, n_states, (int)B, lds_bytes, sys, cp, dev, k.trial, k.status, k.w, k.ft);
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_CHUNK);
            launched = pooled_chunks(ctx, k.ft, k.w, k.status, d_ft_sums, n_draws, n_starts, SIM_LANES, n_chunks);
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_ACCEPT);
            hipLaunchKernelGGL(control_pooled_accept_kernel, dim3((unsigned)S), dim3(SIM_LANES), 0, ctx->stream, D, d_ft_sums,
                               n_chunks, k.trial, k.slope, k.moved, k.pooled, k.z, k.status, k.iterations, k.descent, it);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            ++queued;
        }
        if (it == 0 && first_trial) {
            if (const int failed = k.first_trial_out(ctx, *first_trial)) return failed;
            HIP_TRY(ctx, hipMemcpy(first_trial->ft_sums, d_ft_sums, S * n_chunks * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
        }
        bool stopped = false;
        if (const int failed = poll(ctx, it, max_iter, k.status, S, stopped)) return failed;
        if (stopped) break;
    }
    int64_t worked = 0;
    if (const int failed = k.finish(ctx, who, s, sys, cp, lds_bytes, dev, pass_flops, out, worked)) return failed;
    int64_t *rep = ctx->control_pooled_report;
    k.report_head(rep, n_states, lds_bytes, step_lds);
    rep[7] = queued;
    rep[8] = worked;
    rep[9] = 6;
    clock.read(rep + 10);
    return FOKL_OK;
}

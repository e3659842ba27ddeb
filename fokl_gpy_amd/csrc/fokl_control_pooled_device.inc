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
    double *ex = lds, *zs = ex + SIM_LANES, *gs = zs + SIM_LANES, *ds = gs + SIM_LANES, *H = ds + SIM_LANES;
    double *Hl = H + lane;                                             // Hl[d' * 64] = H[lane][d']
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

template <typename Kernel>
hipError_t pooled_lds(Kernel kernel, size_t lds_bytes)
{
    if (lds_bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SIM_LDS_BUDGET);
}

template <int NS>
hipError_t pooled_tangent(fokl_ctx *ctx, int grid, size_t lds_bytes, const SimSystem &sys, const CtlProblem &cp, const CtlDevice &d,
                          const double *z, const int *status, const double *w, double *rows)
{
    if (hipError_t e = pooled_lds(control_pooled_tangent_kernel<NS>, lds_bytes)) return e;
    hipLaunchKernelGGL(control_pooled_tangent_kernel<NS>, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, cp,
                       d.tab.norm_src, d.tab.norm_lo, d.tab.norm_span, d.tab.fac_norm, d.tab.fac_row, d.tab.fac_degree, d.tab.entries,
                       d.tab.spline, d.tab.bern, d.ct.norm_control, d.ct.seg_first, d.ct.ref, d.coef, d.forcing, d.y0, z, status, w,
                       rows);
    return hipGetLastError();
}

template <int NS>
hipError_t pooled_trial(fokl_ctx *ctx, int grid, size_t lds_bytes, const SimSystem &sys, const CtlProblem &cp, const CtlDevice &d,
                        const double *trial, const int *status, const double *w, double *ft)
{
    if (hipError_t e = pooled_lds(control_pooled_trial_kernel<NS>, lds_bytes)) return e;
    hipLaunchKernelGGL(control_pooled_trial_kernel<NS>, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, cp,
                       d.tab.norm_src, d.tab.norm_lo, d.tab.norm_span, d.tab.fac_norm, d.tab.fac_row, d.tab.fac_degree, d.tab.entries,
                       d.tab.spline, d.tab.bern, d.ct.norm_control, d.ct.seg_first, d.ct.ref, d.coef, d.forcing, d.y0, trial, status, w,
                       ft);
    return hipGetLastError();
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

#define POOLED_NS_SWITCH(call, ...)                                                                                           \
    switch (n_states) {                                                                                                       \
        case 1: launched = call<1>(__VA_ARGS__); break;                                                                       \
        case 2: launched = call<2>(__VA_ARGS__); break;                                                                       \
        case 3: launched = call<3>(__VA_ARGS__); break;                                                                       \
        case 4: launched = call<4>(__VA_ARGS__); break;                                                                       \
        case 5: launched = call<5>(__VA_ARGS__); break;                                                                       \
        case 6: launched = call<6>(__VA_ARGS__); break;                                                                       \
        case 7: launched = call<7>(__VA_ARGS__); break;                                                                       \
        case 8: launched = call<8>(__VA_ARGS__); break;                                                                       \
    }

}  // namespace

extern "C" int fokl_control_pooled_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_control_pooled_report: null argument");
    std::memcpy(out, ctx->control_pooled_report, sizeof ctx->control_pooled_report);
    return FOKL_OK;
}

extern "C" int fokl_control_pooled_solve(
    fokl_ctx *ctx, int n_draws, int n_states, int64_t n_steps, double h, int n_forcing_cols, const double *forcing,
    int n_norm_forcing, int n_norm, const int32_t *norm_src, const double *norm_lo, const double *norm_span, int n_forcing_factors,
    int n_factors, const int32_t *fac_norm, const int32_t *fac_kind, const int32_t *fac_row, const int32_t *fac_degree,
    int n_spline_rows, const double *spline_table, int n_bern_rows, const double *bern_table, int n_entries, const int32_t *entries,
    const int32_t *entry_begin, const int32_t *entry_count, const int32_t *constant, int n_coef, const double *coef, const double *y0,
    const double *box, int n_controls, int n_segments, const int32_t *seg_first, const int32_t *norm_control, const double *ctl_lo,
    const double *ctl_width, const double *ref, const double *track_weight, const double *terminal_weight, const double *limit_lo,
    const double *limit_hi, double limit_weight, const double *move_weight, const double *previous, int has_previous, int n_starts,
    const double *z0, int max_iter, double tol, const double *draw_weights, double *z, double *cost, double *cost_start,
    int32_t *status, int32_t *iterations, int32_t *descent_steps, int32_t *best_start, double *members, int32_t *first_saturation,
    double *cost_draws, double *first_pooled, double *first_rows, const fokl_control_first_trial *first_trial)
{
    const std::string who = "fokl_control_pooled_solve: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->control_pooled_report, 0, sizeof ctx->control_pooled_report);
    if (!draw_weights || !z || !cost || !cost_start || !status || !iterations || !descent_steps || !best_start || !members ||
        !first_saturation || !cost_draws || (first_pooled == nullptr) != (first_rows == nullptr) ||
        (first_trial && (!first_trial->trial || !first_trial->slope || !first_trial->moved || !first_trial->pooled || !first_trial->ft ||
                         !first_trial->ft_sums || !first_trial->z || !first_trial->status || !first_trial->descent)))
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer, negative size or empty system");
    const CtlArgs args{n_draws, n_states, n_steps, h, n_forcing_cols, forcing, n_norm_forcing, n_norm, norm_src, norm_lo, norm_span,
                       n_forcing_factors, n_factors, fac_norm, fac_kind, fac_row, fac_degree, n_spline_rows, spline_table,
                       n_bern_rows, bern_table, n_entries, entries, entry_begin, entry_count, constant, n_coef, coef, y0, box,
                       n_controls, n_segments, seg_first, norm_control, ctl_lo, ctl_width, ref, track_weight, terminal_weight,
                       limit_lo, limit_hi, limit_weight, move_weight, previous, has_previous, n_starts, z0, max_iter, tol};
    SimSystem sys{};
    CtlProblem cp{};
    size_t lds_bytes = 0;
    int n_bern_factors = 0;
    if (const int refused = ctl_plan(ctx, who, args, sys, cp, lds_bytes, n_bern_factors)) return refused;
    double weight_sum = 0.0;
    for (int e = 0; e < n_draws; ++e) {
        if (!(draw_weights[e] >= 0) || !std::isfinite(draw_weights[e]))
            return fail(ctx, FOKL_ERR_ARG, who + "draw weights must be non-negative and finite");
        weight_sum += draw_weights[e];
    }
    if (!(weight_sum > 0)) return fail(ctx, FOKL_ERR_ARG, who + "the draw weights sum to zero: at least one draw must weigh something");

    const int D = cp.D, n = 2 + D + D * D, n_chunks = (n_draws + CTL_POOL_CHUNK - 1) / CTL_POOL_CHUNK;
    const int64_t n_points = n_steps + 1;
    const size_t E = (size_t)n_draws, S = (size_t)n_starts, B = E * S;
    const size_t step_lds = (size_t)(4 + D) * SIM_LANES * sizeof(double);
    const int poll = std::max(0, env_int("FOKL_CONTROL_POLL", 8));    // read the statuses every `poll` iterations; 0: never

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // ---- the workspace against the device's free memory (FOKL_CONTROL_POOLED_FREE_BYTES caps what counts as free) ----
    const size_t workspace = (B * (size_t)(n + SIM_LANES) + S * n_chunks * (size_t)(n + SIM_LANES)) * sizeof(double);
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    if (const char *cap = std::getenv("FOKL_CONTROL_POOLED_FREE_BYTES"))
        free_bytes = std::min<size_t>(free_bytes, std::strtoull(cap, nullptr, 10));
    if (workspace > free_bytes)
        return fail(ctx, FOKL_ERR_ARG,
                    who + "the workspace needs " + std::to_string(workspace) + " bytes (" + std::to_string(n_draws) + " draws x " +
                        std::to_string(n_starts) + " starts x (2 + D + D x D + 64 = " + std::to_string(n + SIM_LANES) +
                        ") x 8, and as much per chunk of 64 draws: " + std::to_string(n_chunks) + " chunks), the device has " +
                        std::to_string(free_bytes) + " free (FOKL_CONTROL_POOLED_FREE_BYTES caps what counts; solve over fewer draws or starts)");

    DeviceBuffers buf;
    CtlDevice dev{};
    HIP_TRY(ctx, ctl_upload(buf, args, dev));
    int *d_status = nullptr, *d_iterations = nullptr, *d_descent = nullptr, *d_work = nullptr, *d_first = nullptr, *d_moved = nullptr,
        *d_running = nullptr;
    double *d_w = nullptr, *d_z = nullptr, *d_cost = nullptr, *d_cost_start = nullptr, *d_rows = nullptr, *d_sums = nullptr,
           *d_ft = nullptr, *d_ft_sums = nullptr, *d_trial = nullptr, *d_slope = nullptr, *d_pooled = nullptr, *d_fpool = nullptr,
           *d_zbest = nullptr, *d_members = nullptr;
    std::vector<int32_t> h_status(S, -1), h_none(S, 0), h_zero((size_t)max_iter + 1, 0);
    std::vector<double> h_nan(S, NAN);
    HIP_TRY(ctx, buf.upload(&d_w, draw_weights, E));
    HIP_TRY(ctx, buf.upload(&d_z, z0, S * D));
    HIP_TRY(ctx, buf.upload(&d_status, h_status.data(), S));
    HIP_TRY(ctx, buf.upload(&d_iterations, h_status.data(), S));
    HIP_TRY(ctx, buf.upload(&d_descent, h_none.data(), S));
    HIP_TRY(ctx, buf.upload(&d_cost, h_nan.data(), S));
    HIP_TRY(ctx, buf.upload(&d_cost_start, h_nan.data(), S));
    HIP_TRY(ctx, buf.upload(&d_work, h_zero.data(), h_zero.size()));
    HIP_TRY(ctx, buf.upload(&d_running, h_status.data(), 1));
    HIP_TRY(ctx, buf.get(&d_rows, B * n));
    HIP_TRY(ctx, buf.get(&d_sums, S * n_chunks * n));
    HIP_TRY(ctx, buf.get(&d_ft, B * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_ft_sums, S * n_chunks * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_trial, S * D * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_slope, S * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_moved, S * SIM_LANES));
    HIP_TRY(ctx, buf.get(&d_pooled, S * (2 + D)));
    if (first_pooled) {                                               // a draw of weight 0 writes no row: its row reads NaN
        std::vector<double> h_rows(B * n, NAN);
        HIP_TRY(ctx, hipMemcpy(d_rows, h_rows.data(), h_rows.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(ctx, buf.get(&d_fpool, S * n));
    }
    if (first_trial) {                                                // what iteration 0 does not write reads NaN, moved 0
        HIP_TRY(ctx, pooled_fill_nan(d_trial, S * D * SIM_LANES));
        HIP_TRY(ctx, pooled_fill_nan(d_slope, S * SIM_LANES));
        HIP_TRY(ctx, pooled_fill_nan(d_pooled, S * (2 + D)));
        HIP_TRY(ctx, pooled_fill_nan(d_ft, B * SIM_LANES));
        HIP_TRY(ctx, pooled_fill_nan(d_ft_sums, S * n_chunks * SIM_LANES));
        HIP_TRY(ctx, hipMemset(d_moved, 0, S * SIM_LANES * sizeof(int)));
    }
    HIP_TRY(ctx, buf.get(&d_zbest, E * D));
    HIP_TRY(ctx, buf.get(&d_members, E * n_states * n_points));
    HIP_TRY(ctx, buf.get(&d_first, E));

    double terms_per_stage = 0.0;
    for (int k = 0; k < n_states; ++k) terms_per_stage += sys.entry_count[k];
    const double pass_flops = (double)B * SIM_LANES * (double)n_steps * 4.0 * (8.0 * terms_per_stage + 20.0 * n_factors);
    PooledClock clock(ctx);
    int64_t queued = 0;
    hipError_t launched = hipSuccess;
    for (int it = 0; it <= max_iter; ++it) {
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (2.0 * (double)B * (n + SIM_LANES)), 3.0 * pass_flops);
            clock.before(POOLED_TANGENT);
            POOLED_NS_SWITCH(pooled_tangent, ctx, (int)B, lds_bytes, sys, cp, dev, d_z, d_status, d_w, d_rows)
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_CHUNK);
            launched = pooled_chunks(ctx, d_rows, d_w, d_status, d_sums, n_draws, n_starts, n, n_chunks);
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_STEP);
            hipLaunchKernelGGL(control_pooled_step_kernel, dim3((unsigned)S), dim3(SIM_LANES), step_lds, ctx->stream, cp, d_sums,
                               n_chunks, d_z, d_status, d_iterations, d_cost, d_cost_start, d_work, d_trial, d_slope, d_moved,
                               d_pooled, d_fpool, it);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_TRIAL);
            POOLED_NS_SWITCH(pooled_trial, ctx, (int)B, lds_bytes, sys, cp, dev, d_trial, d_status, d_w, d_ft)
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_CHUNK);
            launched = pooled_chunks(ctx, d_ft, d_w, d_status, d_ft_sums, n_draws, n_starts, SIM_LANES, n_chunks);
            clock.after();
            HIP_TRY(ctx, launched);
            clock.before(POOLED_ACCEPT);
            hipLaunchKernelGGL(control_pooled_accept_kernel, dim3((unsigned)S), dim3(SIM_LANES), 0, ctx->stream, D, d_ft_sums,
                               n_chunks, d_trial, d_slope, d_moved, d_pooled, d_z, d_status, d_iterations, d_descent, it);
            launched = hipGetLastError();
            clock.after();
            HIP_TRY(ctx, launched);
            ++queued;
        }
        if (it == 0 && first_trial) {                                 // iteration 0's trial half, before a later one overwrites it
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy(first_trial->trial, d_trial, S * D * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->slope, d_slope, S * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->moved, d_moved, S * SIM_LANES * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->pooled, d_pooled, S * (2 + D) * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->ft, d_ft, B * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->ft_sums, d_ft_sums, S * n_chunks * SIM_LANES * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->z, d_z, S * D * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->status, d_status, S * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(first_trial->descent, d_descent, S * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        if (poll > 0 && (it + 1) % poll == 0 && it < max_iter) {      // may stop queuing early: an iteration without work changes nothing
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy(h_status.data(), d_status, S * sizeof(int32_t), hipMemcpyDeviceToHost));
            bool running = false;
            for (size_t s = 0; s < S && !running; ++s) running = h_status[s] < 0;
            if (!running) break;
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(z, d_z, S * D * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cost, d_cost, S * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cost_start, d_cost_start, S * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(status, d_status, S * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(iterations, d_iterations, S * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(descent_steps, d_descent, S * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(h_zero.data(), d_work, h_zero.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (first_pooled) {
        HIP_TRY(ctx, hipMemcpy(first_pooled, d_fpool, S * n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(first_rows, d_rows, B * n * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (size_t s = 0; s < S; ++s)
        if (status[s] < 0) return fail(ctx, FOKL_ERR_HIP, who + "a solve was left running");
    int64_t worked = 0;
    for (int32_t found : h_zero) worked += found;

    // ---- the best start (a non-finite solve is never the best); every draw's trajectory and own cost under its controls ----
    int best = 0;
    double best_key = INFINITY;
    for (int s = 0; s < n_starts; ++s) {
        const double key = (std::isfinite(cost[s]) && status[s] != CTL_NON_FINITE) ? cost[s] : INFINITY;
        if (key < best_key) {
            best_key = key;
            best = s;
        }
    }
    *best_start = best;
    std::vector<double> z_best(E * D), point((size_t)D * SIM_LANES);
    for (size_t e = 0; e < E; ++e) std::memcpy(z_best.data() + e * D, z + (size_t)best * D, D * sizeof(double));
    for (int d = 0; d < D; ++d)
        for (int lane = 0; lane < SIM_LANES; ++lane) point[(size_t)d * SIM_LANES + lane] = z[(size_t)best * D + d];
    HIP_TRY(ctx, hipMemcpy(d_zbest, z_best.data(), E * D * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_trial, point.data(), point.size() * sizeof(double), hipMemcpyHostToDevice));
    {
        TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)E * n_states * n_points, 2.0 * pass_flops / (double)S);
#define CTL_CASE(NS)                                                                                                         \
    case NS:                                                                                                                 \
        launched = ctl_trajectory<NS>(ctx, n_draws, lds_bytes, sys, cp, dev.tab, dev.ct, dev.coef, dev.forcing, dev.y0, d_zbest,  \
                                      d_members, d_first);                                                                   \
        break;
        switch (n_states) {
            CTL_CASE(1) CTL_CASE(2) CTL_CASE(3) CTL_CASE(4) CTL_CASE(5) CTL_CASE(6) CTL_CASE(7) CTL_CASE(8)
        }
#undef CTL_CASE
        HIP_TRY(ctx, launched);
        // one start (d_running holds -1), no weights: every draw's value pass at the returned point, lane 0 is read
        POOLED_NS_SWITCH(pooled_trial, ctx, n_draws, lds_bytes, sys, cp, dev, d_trial, d_running, nullptr, d_ft)
        HIP_TRY(ctx, launched);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(members, d_members, E * n_states * n_points * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(first_saturation, d_first, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<double> h_ft(E * SIM_LANES);
    HIP_TRY(ctx, hipMemcpy(h_ft.data(), d_ft, h_ft.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < E; ++e) cost_draws[e] = h_ft[e * SIM_LANES];
    int64_t *rep = ctx->control_pooled_report;
    rep[0] = n_states;
    rep[1] = n_draws;
    rep[2] = n_starts;
    rep[3] = D;
    rep[4] = n_chunks;
    rep[5] = (int64_t)lds_bytes;
    rep[6] = (int64_t)step_lds;
    rep[7] = queued;
    rep[8] = worked;
    rep[9] = 6;
    clock.read(rep + 10);
    return FOKL_OK;
}

#undef POOLED_NS_SWITCH

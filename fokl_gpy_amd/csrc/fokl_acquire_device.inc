// acquire(): which rows of a candidate pool should be measured next to find a better optimum -- expected improvement (EI) and
// probability of improvement (PI) over the posterior draws, greedy batch selection (textually included by fokl_hip.hip after
// fokl_draw_tile.inc).  The statement is fokl_gpy_amd/acquire.py: select_host.
//
// With f_sd = x_s . beta_d the fitted function of draw d at pool row s and b_d the incumbent of draw d, the gain of a row is
//   'ei'   (sum_d max(f_sd - b_d, 0)) / E          and a pick s* sets  b_d <- max(b_d, f_s*d)
//   'pi'   (sum_d [f_sd > b_d]) / E                and a pick s* sets  b_d <- +inf where f_s*d > b_d
// A pick is the arg-max over the rows not yet picked, the lowest index on equal values; NaN never wins.  The product is the
// draw tile's (fokl_draw_tile.inc: the coefficient table and the lane map): one wavefront per tile of 16 rows, the tile's
// basis values in LDS [ncp][16], blocks of AQ_DT x 16 draws; f is never stored.  b is a device vector [dp] of its own, not a
// row of the coefficient table: the picks change it between the launches, the table is written once.
//   acquire_pass_kernel    the gain g of every row of the tiles it evaluates, and one (value, index) per workgroup behind the
//                          mask of picked rows.  Each lane sums its quarter of the draws in draw order, the four quarters of a
//                          row merge in their order, the division by E comes last.  Under LAZY a tile first reads its 16 stale
//                          gains and tau and leaves without touching LDS or the product if every row not yet picked has a
//                          stale gain strictly below tau (a NaN is not below: such a tile is evaluated); the candidate's tile,
//                          fresh from the pivot, is not evaluated again.  Skipped rows enter the arg-max with their stale gain.
//   acquire_bound_kernel   the arg-max of the stale g behind the mask: a stream over 8 + 1 bytes per row.
//   acquire_pivot_kernel   one wavefront.  AQ_CANDIDATE: the bound partials in index order, the candidate's tile evaluated fresh
//                          (g written), tau = the largest fresh gain among its rows not yet picked, the tile's number.
//                          AQ_PICK: the pass partials in index order, the evaluated tiles summed, index and gain recorded, the
//                          mask set, and b updated from draw_product on the PICKED ROW'S TILE: f* has the bits the pass saw,
//                          so the picked row's 'ei' is exactly 0.0 in every later pass.  A pick that finds no row (all
//                          picked, or every gain NaN) writes index -1, gain -inf and leaves b alone.
// Why skipping changes no bit: b only rises, and f - b, the comparison with 0, the sum of non-negative terms in a fixed order
// and the division by E are monotone under correct rounding; f is recomputed by the same instructions every time.  So a
// row's gain of an earlier pick bounds its gain now, a skipped tile's rows are all strictly below a gain that exists, and
// the arg-max and its value are those of evaluating everything.  The set of evaluated tiles follows from the values alone.
// The best of two candidates is the larger value, on equal values the lower index (ds_better): associative and commutative,
// so neither the grid nor the order of a reduction changes a bit.  Nothing is accumulated with atomics.

namespace fokl {

constexpr int AQ_DT = 4;                         // 16-draw tiles per block: independent MFMA chains
constexpr int AQ_BOUND_THREADS = 256;
enum { AQ_EI = FOKL_ACQUIRE_EI, AQ_PI = FOKL_ACQUIRE_PI };
enum { AQ_CANDIDATE = 0, AQ_PICK = 1 };

// one draw's term of a row's gain; an f that is not finite makes the row's gain NaN under both criteria
template <int CRIT>
__device__ __forceinline__ double aq_term(double f, double b)
{
    if constexpr (CRIT == AQ_EI) {
        const double t = f - b;
        return t <= 0.0 ? 0.0 : t;                   // NaN is not <= 0: it stays
    } else {
        return f > b ? 1.0 : f - f;                  // 0.0, or NaN
    }
}

// The gain of row `col` of the tile in xs, in all four lanes of the row.  Padding draws and the clamped tiles past dp are
// skipped; their b is read (inside [dp]) and never used.
template <int CRIT>
__device__ __forceinline__ double aq_tile_gain(const double *xs, const double *__restrict__ betas_t, const double *b, int ncp,
                                               int draws, int dp, int quad, int col)
{
    double s = 0.0;
    for (int d0 = 0; d0 < dp; d0 += 16 * AQ_DT) {
        d4 acc[AQ_DT];
        draw_product<AQ_DT>(xs, betas_t, ncp, dp, d0, quad, col, acc);
#pragma unroll
        for (int t = 0; t < AQ_DT; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int d = d0 + 16 * t + quad + 4 * v;
                const double bv = b[min(d, dp - 1)];
                if (d < draws) s += aq_term<CRIT>(acc[t][v], bv);
            }
    }
    double G = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) G += __shfl(s, col + 16 * q, WAVE);     // the row's four quarters, in their order
    return G / (double)draws;
}

// (value, index) of the wavefront's best under ds_better, in every lane
__device__ __forceinline__ void aq_wave_best(double &best, int64_t &best_i)
{
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const double ov = __shfl_xor(best, off, WAVE);
        const int64_t oi = __shfl_xor(best_i, off, WAVE);
        if (ds_better(ov, oi, best, best_i)) {
            best = ov;
            best_i = oi;
        }
    }
}

// tau_p, cand_p: what the candidate pivot left (LAZY only).  trace_g [n], trace_eval [tiles]: null, or where this pass
// leaves g as it stands after it and, under LAZY, whether a tile was evaluated for this pick (by this pass or the pivot).
template <int CRIT, bool LAZY>
__global__ __launch_bounds__(WAVE) void acquire_pass_kernel(double *const *__restrict__ slot_ptr, const int *__restrict__ slots,
                                                             int nc, int ncp, const double *__restrict__ betas_t,
                                                             const double *b, int draws, int dp, int64_t n, double *g,
                                                             const unsigned char *__restrict__ mask, const double *tau_p,
                                                             const int64_t *cand_p, double *__restrict__ part_val,
                                                             int64_t *__restrict__ part_idx, int *__restrict__ evals,
                                                             double *__restrict__ trace_g, unsigned char *__restrict__ trace_eval)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [ncp][16]
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int64_t n_tiles = (n + 15) / 16;
    double tau = -INFINITY;
    int64_t cand = -1;
    if constexpr (LAZY) {
        tau = tau_p[0];
        cand = cand_p[0];
    }
    double best = -INFINITY;
    int64_t best_i = DS_NO_ROW;
    int evaluated = 0;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * 16 + col;
        const bool in = r < n;
        const bool open = in && !mask[r];
        double G = 0.0;
        bool fresh = true;
        if constexpr (LAZY) {
            G = in ? g[r] : 0.0;
            fresh = tile != cand && __any(open && !(G < tau));           // wave uniform
        }
        if (fresh) {
            draw_tile_load(xs, slot_ptr, slots, nc, ncp, r, in, quad, col);
            __syncthreads();                             // one wavefront per workgroup: orders the LDS traffic
            G = aq_tile_gain<CRIT>(xs, betas_t, b, ncp, draws, dp, quad, col);
            if (quad == 0 && in) g[r] = G;
            ++evaluated;
            __syncthreads();                             // the tile's LDS has been read: the next one may be stored
        }
        if (trace_g && quad == 0 && in) trace_g[r] = G;
        if (LAZY && trace_eval && lane == 0) trace_eval[tile] = (fresh || tile == cand) ? 1 : 0;
        const double crit = open ? G : -INFINITY;
        if (quad == 0 && in && ds_better(crit, r, best, best_i)) {
            best = crit;
            best_i = r;
        }
    }
    aq_wave_best(best, best_i);
    if (lane == 0) {
        part_val[blockIdx.x] = best;
        part_idx[blockIdx.x] = best_i;
        evals[blockIdx.x] = evaluated;
    }
}

__global__ __launch_bounds__(AQ_BOUND_THREADS) void acquire_bound_kernel(const double *__restrict__ g,
                                                                          const unsigned char *__restrict__ mask, int64_t n,
                                                                          double *__restrict__ part_val,
                                                                          int64_t *__restrict__ part_idx)
{
    __shared__ double red_v[AQ_BOUND_THREADS / WAVE];
    __shared__ int64_t red_i[AQ_BOUND_THREADS / WAVE];
    const int tid = threadIdx.x;
    double best = -INFINITY;
    int64_t best_i = DS_NO_ROW;
    for (int64_t s = (int64_t)blockIdx.x * AQ_BOUND_THREADS + tid; s < n; s += (int64_t)gridDim.x * AQ_BOUND_THREADS) {
        const double crit = mask[s] ? -INFINITY : g[s];
        if (ds_better(crit, s, best, best_i)) {
            best = crit;
            best_i = s;
        }
    }
    aq_wave_best(best, best_i);
    if (tid % WAVE == 0) {
        red_v[tid / WAVE] = best;
        red_i[tid / WAVE] = best_i;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < AQ_BOUND_THREADS / WAVE; ++k)
            if (ds_better(red_v[k], red_i[k], best, best_i)) {
                best = red_v[k];
                best_i = red_i[k];
            }
        part_val[blockIdx.x] = best;
        part_idx[blockIdx.x] = best_i;
    }
}

// mode AQ_CANDIDATE: parts partials of acquire_bound_kernel -> g of the candidate's tile, tau_p, cand_p.
// mode AQ_PICK: parts partials and evals of acquire_pass_kernel -> index_out, gain_out, tiles_out [pick_no], mask, b.
template <int CRIT>
__global__ __launch_bounds__(WAVE) void acquire_pivot_kernel(double *const *__restrict__ slot_ptr, const int *__restrict__ slots,
                                                              int nc, int ncp, const double *__restrict__ betas_t, double *b,
                                                              int draws, int dp, int64_t n, const double *__restrict__ part_val,
                                                              const int64_t *__restrict__ part_idx, int parts,
                                                              const int *__restrict__ evals, int mode, int pick_no, double *g,
                                                              unsigned char *mask, double *tau_p, int64_t *cand_p,
                                                              int64_t *__restrict__ index_out, double *__restrict__ gain_out,
                                                              int64_t *__restrict__ tiles_out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [ncp][16]
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;

    // the partials, in index order per lane, then the butterfly: the comparison is associative and commutative
    double best = -INFINITY;
    int64_t best_i = DS_NO_ROW;
    for (int k = lane; k < parts; k += WAVE)
        if (ds_better(part_val[k], part_idx[k], best, best_i)) {
            best = part_val[k];
            best_i = part_idx[k];
        }
    aq_wave_best(best, best_i);
    const bool none = best_i == DS_NO_ROW || !(best > -INFINITY);     // nothing left to take (or every gain NaN)
    const int64_t tile = none ? 0 : best_i / 16;
    const int64_t r = tile * 16 + col;
    const bool in = r < n;

    if (mode == AQ_CANDIDATE) {
        if (none) {
            if (lane == 0) {
                tau_p[0] = -INFINITY;
                cand_p[0] = -1;
            }
            return;
        }
        draw_tile_load(xs, slot_ptr, slots, nc, ncp, r, in, quad, col);
        __syncthreads();
        const double G = aq_tile_gain<CRIT>(xs, betas_t, b, ncp, draws, dp, quad, col);
        if (quad == 0 && in) g[r] = G;
        double t = (in && !mask[r] && G > -INFINITY) ? G : -INFINITY;    // NaN is not above: it is left out
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const double o = __shfl_xor(t, off, WAVE);
            t = o > t ? o : t;
        }
        if (lane == 0) {
            tau_p[0] = t;
            cand_p[0] = tile;
        }
        return;
    }

    int64_t ev = 0;
    for (int k = lane; k < parts; k += WAVE) ev += evals[k];
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) ev += __shfl_xor(ev, off, WAVE);
    if (lane == 0) {
        tiles_out[pick_no] = ev + (cand_p[0] >= 0 ? 1 : 0);          // the candidate's tile was the pivot's
        index_out[pick_no] = none ? -1 : best_i;
        gain_out[pick_no] = none ? -INFINITY : best;
    }
    if (none) return;
    const int cstar = (int)(best_i - tile * 16);
    draw_tile_load(xs, slot_ptr, slots, nc, ncp, r, in, quad, col);
    __syncthreads();
    for (int d0 = 0; d0 < dp; d0 += 16 * AQ_DT) {
        d4 acc[AQ_DT];
        draw_product<AQ_DT>(xs, betas_t, ncp, dp, d0, quad, col, acc);
#pragma unroll
        for (int t = 0; t < AQ_DT; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int d = d0 + 16 * t + quad + 4 * v;               // draw d belongs to one lane of the picked row
                if (col == cstar && d < draws) {
                    const double f = acc[t][v];
                    if (f > b[d]) b[d] = CRIT == AQ_EI ? f : INFINITY;
                }
            }
    }
    if (lane == 0) mask[best_i] = 1;
}

}  // namespace fokl

extern "C" int fokl_acquire_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_acquire_report: null argument");
    std::memcpy(out, ctx->acquire_report, sizeof ctx->acquire_report);
    return FOKL_OK;
}

extern "C" int fokl_acquire_select(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, int draws,
                                   const double *incumbent, int criterion, int lazy, int picks, int grid_cap, int trace_pick,
                                   int64_t *index_out, double *gain_out, double *incumbent_out, int64_t *tiles_out,
                                   double *trace_g_out, unsigned char *trace_eval_out)
{
    using namespace fokl;
    const std::string who = "fokl_acquire_select";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + ": null context");
    std::memset(ctx->acquire_report, 0, sizeof ctx->acquire_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, who + ": call fokl_upload first");
    if (nc <= 0 || draws <= 0 || !betas || !incumbent || !index_out || !gain_out || !incumbent_out || !tiles_out || grid_cap < 0)
        return fail(ctx, FOKL_ERR_ARG, who + ": bad argument");
    if (draws > (1 << 22) || nc > (1 << 20)) return fail(ctx, FOKL_ERR_ARG, who + ": too many draws or columns");
    if (criterion != FOKL_ACQUIRE_EI && criterion != FOKL_ACQUIRE_PI)
        return fail(ctx, FOKL_ERR_ARG, who + ": criterion must be FOKL_ACQUIRE_EI (1) or FOKL_ACQUIRE_PI (2)");
    const int64_t n = ctx->n;
    if (n <= 0) return fail(ctx, FOKL_ERR_STATE, who + ": the dataset has no rows");
    if (picks < 1) return fail(ctx, FOKL_ERR_ARG, who + ": picks must be at least 1");
    if ((int64_t)picks > n)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(picks) + " picks from a pool of " + std::to_string(n) +
                    " rows: a row is taken once (the function is noiseless, a second visit gains nothing)");
    if (trace_pick < -1 || trace_pick >= picks)
        return fail(ctx, FOKL_ERR_ARG, who + ": trace_pick must be -1 (off) or a pick, 0 .. picks - 1");
    if (trace_pick >= 0 && (!trace_g_out || (lazy && !trace_eval_out)))
        return fail(ctx, FOKL_ERR_ARG, who + ": trace_pick needs trace_g_out and, under lazy, trace_eval_out");
    for (size_t i = 0; i < (size_t)draws * nc; ++i)
        if (!std::isfinite(betas[i])) return fail(ctx, FOKL_ERR_ARG, who + ": every coefficient must be finite");
    for (int d = 0; d < draws; ++d)
        if (std::isnan(incumbent[d]) || incumbent[d] == INFINITY)
            return fail(ctx, FOKL_ERR_ARG, who + ": every incumbent must be finite or -inf (draw " + std::to_string(d) + " is not)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_slots(ctx, slots, nc, who.c_str());
    if (rc) return rc;

    const int ncp = (nc + 3) & ~3, dp = (draws + 15) & ~15;
    const size_t lds_bytes = (size_t)ncp * 16 * sizeof(double);
    if (lds_bytes > 160 * 1024)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(nc) + " columns want " + std::to_string(lds_bytes) +
                    " bytes of LDS per 16-row tile, a compute unit has 163840 (at most 1280 columns)");
    const int64_t tiles = (n + 15) / 16;
    const bool trace = trace_pick >= 0;
    const size_t table_bytes = ((size_t)ncp + 1) * dp * sizeof(double);
    const size_t row_bytes = (size_t)n * (sizeof(double) * (trace ? 2 : 1) + 1) + (trace && lazy ? (size_t)tiles : 0);
    const size_t pick_bytes = (size_t)picks * 3 * sizeof(double);
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_ACQUIRE_FREE_BYTES", &free_bytes));
    if (table_bytes + row_bytes + pick_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + ": the call wants " + std::to_string(table_bytes + row_bytes + pick_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(table_bytes) +
                    " bytes of coefficients = (columns + 1) x draws x 8, " + std::to_string(row_bytes) + " per-row bytes = rows x " +
                    std::to_string(trace ? 17 : 9) + ", " + std::to_string(pick_bytes) + " of picks), the device has " +
                    std::to_string(free_bytes) + " free (FOKL_ACQUIRE_FREE_BYTES caps what counts" +
                    (table_bytes > row_bytes ? "; thin the draws)" : "; select from the pool in parts)"));

    // coefficients transposed and zero padded [ncp][dp]; b [dp] apart from them (padding draws: 0, never used)
    std::vector<double> table((size_t)ncp * dp, 0.0), b0((size_t)dp, 0.0);
    fill_draw_table(table.data(), betas, draws, nc, ncp, dp);
    std::memcpy(b0.data(), incumbent, (size_t)draws * sizeof(double));

    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, 160 * 1024 / lds_bytes));
    int grid = (int)std::min<int64_t>(tiles, (int64_t)cu_count(ctx) * per_cu);
    int grid_b = (int)std::min<int64_t>((n + AQ_BOUND_THREADS - 1) / AQ_BOUND_THREADS, (int64_t)cu_count(ctx) * 8);
    if (grid_cap > 0) {
        grid = std::min(grid, grid_cap);
        grid_b = std::min(grid_b, grid_cap);
    }
    const int parts_max = std::max(grid, grid_b);

    DeviceBuffers buf;
    double *d_table = nullptr, *d_b = nullptr, *d_g = nullptr, *d_part = nullptr, *d_gain = nullptr, *d_tau = nullptr,
           *d_trace_g = nullptr;
    int64_t *d_part_i = nullptr, *d_index = nullptr, *d_tiles = nullptr, *d_cand = nullptr;
    unsigned char *d_mask = nullptr, *d_trace_eval = nullptr;
    int *d_slots = nullptr, *d_evals = nullptr;
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_b, b0.data(), b0.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc));
    HIP_TRY(ctx, buf.get(&d_g, (size_t)n));
    HIP_TRY(ctx, buf.get(&d_mask, (size_t)n));
    HIP_TRY(ctx, buf.get(&d_part, (size_t)parts_max));
    HIP_TRY(ctx, buf.get(&d_part_i, (size_t)parts_max));
    HIP_TRY(ctx, buf.get(&d_evals, (size_t)grid));
    HIP_TRY(ctx, buf.get(&d_index, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_tiles, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_gain, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_tau, (size_t)1));
    HIP_TRY(ctx, buf.get(&d_cand, (size_t)1));
    if (trace) HIP_TRY(ctx, buf.get(&d_trace_g, (size_t)n));
    if (trace && lazy) HIP_TRY(ctx, buf.get(&d_trace_eval, (size_t)tiles));
    HIP_TRY(ctx, hipMemsetAsync(d_mask, 0, (size_t)n, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_tau, 0, sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_cand, 0xff, sizeof(int64_t), ctx->stream));          // -1: no candidate's tile yet

    const bool ei = criterion == FOKL_ACQUIRE_EI;
    auto pass_full = ei ? acquire_pass_kernel<AQ_EI, false> : acquire_pass_kernel<AQ_PI, false>;
    auto pass_lazy = ei ? acquire_pass_kernel<AQ_EI, true> : acquire_pass_kernel<AQ_PI, true>;
    auto pivot = ei ? acquire_pivot_kernel<AQ_EI> : acquire_pivot_kernel<AQ_PI>;
    HIP_TRY(ctx, lds_opt_in(pass_full, lds_bytes, 160 * 1024));
    HIP_TRY(ctx, lds_opt_in(pass_lazy, lds_bytes, 160 * 1024));
    HIP_TRY(ctx, lds_opt_in(pivot, lds_bytes, 160 * 1024));

    // marks: the whole queue always; with timing on also every launch, by kernel
    hipError_t e = hipSuccess;
    StreamStopwatch watch(ctx, e);
    std::vector<std::pair<int, int>> pass_marks, bound_marks, pivot_marks;
    const bool split = ctx->timing;
    int64_t launches = 0;
    const int total0 = watch.mark();
    {
        TimedRegion timed(ctx, FOKL_K_ACQUIRE, 0.0, 0.0);                // bytes and flops: below, of the tiles evaluated
        auto launch_pivot = [&](int mode, int parts, int k) {
            const int m0 = split ? watch.mark() : 0;
            hipLaunchKernelGGL(pivot, dim3(1), dim3(WAVE), lds_bytes, ctx->stream, ctx->d_slot_ptr, d_slots, nc, ncp, d_table, d_b,
                               draws, dp, n, d_part, d_part_i, parts, d_evals, mode, k, d_g, d_mask, d_tau, d_cand, d_index, d_gain,
                               d_tiles);
            if (e == hipSuccess) e = hipGetLastError();
            if (split) pivot_marks.push_back({m0, watch.mark()});
            ++launches;
        };
        for (int k = 0; k < picks && e == hipSuccess; ++k) {
            const bool skipping = lazy && k > 0;
            if (skipping) {
                const int m0 = split ? watch.mark() : 0;
                hipLaunchKernelGGL(acquire_bound_kernel, dim3(grid_b), dim3(AQ_BOUND_THREADS), 0, ctx->stream, d_g, d_mask, n,
                                   d_part, d_part_i);
                if (e == hipSuccess) e = hipGetLastError();
                if (split) bound_marks.push_back({m0, watch.mark()});
                ++launches;
                launch_pivot(AQ_CANDIDATE, grid_b, k);
            }
            const bool traced = k == trace_pick;
            const int m1 = split ? watch.mark() : 0;
            hipLaunchKernelGGL(skipping ? pass_lazy : pass_full, dim3(grid), dim3(WAVE), lds_bytes, ctx->stream, ctx->d_slot_ptr,
                               d_slots, nc, ncp, d_table, d_b, draws, dp, n, d_g, d_mask, d_tau, d_cand, d_part, d_part_i, d_evals,
                               traced ? d_trace_g : (double *)nullptr, traced ? d_trace_eval : (unsigned char *)nullptr);
            if (e == hipSuccess) e = hipGetLastError();
            if (split) pass_marks.push_back({m1, watch.mark()});
            ++launches;
            launch_pivot(AQ_PICK, grid, k);
        }
    }
    const int total1 = watch.mark();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    auto span = [&](const std::vector<std::pair<int, int>> &marks) -> int64_t {
        double sum = 0.0;
        for (const auto &m : marks) sum += watch.us(m.first, m.second);
        return (int64_t)std::llround(sum);
    };
    const int64_t us_total = span({{total0, total1}}), us_pass = span(pass_marks), us_bound = span(bound_marks),
                  us_pivot = span(pivot_marks);
    if (e == hipSuccess) e = hipMemcpy(index_out, d_index, (size_t)picks * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(gain_out, d_gain, (size_t)picks * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(tiles_out, d_tiles, (size_t)picks * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(incumbent_out, d_b, (size_t)draws * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && trace) e = hipMemcpy(trace_g_out, d_trace_g, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && trace && lazy) {
        if (trace_pick == 0) std::memset(trace_eval_out, 1, (size_t)tiles);         // the first pass evaluates everything
        else e = hipMemcpy(trace_eval_out, d_trace_eval, (size_t)tiles, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, who + ": " + hipGetErrorString(e));

    int64_t sum = 0, most_lazy = 0;
    for (int k = 0; k < picks; ++k) {
        sum += tiles_out[k];
        if (lazy && k > 0) most_lazy = std::max(most_lazy, tiles_out[k]);
    }
    if (ctx->timing) {
        const double bytes = 8.0 * 16.0 * (double)sum * nc + 9.0 * (double)n * (double)(lazy ? 2 * picks - 1 : picks);
        const double flops = 2.0 * 16.0 * (double)ncp * (double)draws * (double)(sum + picks);
        ctx->tslot[FOKL_K_ACQUIRE].bytes += bytes;
        ctx->tslot[FOKL_K_ACQUIRE].flops += flops;
        ctx->tslot[FOKL_K_ACQUIRE].ideal_ms += 1e3 * std::max(bytes / FOKL_PEAK_HBM_BYTES_PER_S, flops / FOKL_PEAK_F64_FLOPS);
    }
    int64_t *rep = ctx->acquire_report;
    rep[0] = criterion;
    rep[1] = lazy ? 1 : 0;
    rep[2] = grid;
    rep[3] = grid_b;
    rep[4] = tiles;
    rep[5] = (int64_t)lds_bytes;
    rep[6] = AQ_DT;
    rep[7] = picks;
    rep[8] = launches;
    rep[9] = sum;
    rep[10] = most_lazy;
    rep[11] = us_total;
    rep[12] = us_pass;
    rep[13] = us_bound;
    rep[14] = us_pivot;
    return FOKL_OK;
}

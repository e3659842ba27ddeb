// acquire_system(): EI and PI over a candidate pool under limits on OTHER models' outputs, greedy batch selection (textually
// included by fokl_hip.hip after fokl_acquire_device.inc, whose aq_term, aq_wave_best and acquire_bound_kernel it uses).  The
// statement is fokl_gpy_amd/acquire.py: select_system_host and incumbent_system_host.
//
// Model 0 is the objective, models 1..K the constraint models with limits lo_k <= hi_k (either may be infinite).  Draw d is
// row d of every model's coefficients.  With f_sd = x0_s . beta0_d and g_ksd = xk_s . betak_d,
//   ok_sd   every k has g_ksd >= lo_k and g_ksd <= hi_k (a NaN g is therefore infeasible)
//   'ei'    (sum_d ok_sd ? max(f_sd - b_d, 0) : 0.0) / E     and a pick s* sets  b_d <- max(b_d, f_s*d) where ok_s*d
//   'pi'    (sum_d ok_sd ? [f_sd > b_d] : 0.0) / E           and a pick s* sets  b_d <- +inf where ok_s*d and f_s*d > b_d
// An infeasible draw adds nothing to a lane's sum (s + 0.0 is s: the sums are never -0.0), whatever f is.  ok does not depend
// on b, so a gain still only falls as b rises and the lazy rule of fokl_acquire_device.inc holds word for word.
//
// The tile's LDS is [sum ncp_k][16]: model k's basis values at row offset off_k = sum_{j<k} ncp_j, each model padded to 4 on
// its own, and the coefficient tables lie likewise one behind the other, [ncp_k][dp] each.  One draw_tile_load and one
// draw_product<AQ_DT> per model on its own sub-table.  Per block of 64 draws the constraint products run first, one model
// after the other, and are folded into a 16-bit mask per lane (bit 4 t + v: draw d0 + 16 t + quad + 4 v); then the
// objective's product forms the terms: one accumulator set is live at a time.  With infinite limits the objective sees the
// instructions of acquire_pass_kernel.
//   acquire_system_pass_kernel       acquire_pass_kernel with that gain
//   acquire_system_pivot_kernel      acquire_pivot_kernel with that gain; AQ_PICK recomputes ALL products on the picked row's
//                                    tile, updates b in the feasible draws only and writes the picked row's feasible-draw
//                                    count (the row's four lanes, added in their order)
//   acquire_system_incumbent_kernel  per draw the largest f over the uploaded rows that are feasible in that draw and their
//                                    number: a tile's 16 rows are merged across the 16 lanes of a quarter, lane col 0 keeps
//                                    the workgroup's [dp] partial in global memory (it alone touches its draws)
//   acquire_system_merge_kernel      the workgroups' partials in index order
// The maximum that keeps a NaN (aqs_nan_max) and the integer sum are associative and commutative: no atomics, and the same
// arguments give the same bits whatever the grid.

namespace fokl {

constexpr int AQS_MAX_MODELS = FOKL_ACQUIRE_SYSTEM_MAX_MODELS;
constexpr int AQS_MERGE_THREADS = 256;
constexpr int AQS_INCUMBENT = FOKL_ACQUIRE_SYSTEM_INCUMBENT;

// what the kernels know of the models (device memory, read uniformly); [0] is the objective, lo / hi [0] are not used
struct AqsModels {
    int count;                                   // K + 1
    int nc[AQS_MAX_MODELS];                      // columns
    int ncp[AQS_MAX_MODELS];                     // ... rounded up to 4
    int off[AQS_MAX_MODELS];                     // sum of ncp before it: the row of its basis values in LDS and of its table
    int slot0[AQS_MAX_MODELS];                   // where its slots begin in the slot list
    double lo[AQS_MAX_MODELS], hi[AQS_MAX_MODELS];
};

__device__ __forceinline__ void aqs_tile_load(double *xs, double *const *__restrict__ slot_ptr, const int *__restrict__ slots,
                                              const AqsModels *__restrict__ m, int64_t r, bool in, int quad, int col)
{
    const int count = m->count;
    for (int k = 0; k < count; ++k)
        draw_tile_load(xs + (size_t)m->off[k] * 16, slot_ptr, slots + m->slot0[k], m->nc[k], m->ncp[k], r, in, quad, col);
}

// bit 4 t + v: draw d0 + 16 t + quad + 4 v of row col satisfies every constraint model
__device__ __forceinline__ unsigned aqs_block_mask(const double *xs, const double *__restrict__ betas_t,
                                                   const AqsModels *__restrict__ m, int dp, int d0, int quad, int col)
{
    unsigned ok = 0xffffu;
    const int count = m->count;
    for (int k = 1; k < count; ++k) {
        const int off = m->off[k];
        const double lo = m->lo[k], hi = m->hi[k];
        d4 acc[AQ_DT];
        draw_product<AQ_DT>(xs + (size_t)off * 16, betas_t + (size_t)off * dp, m->ncp[k], dp, d0, quad, col, acc);
#pragma unroll
        for (int t = 0; t < AQ_DT; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (!(acc[t][v] >= lo && acc[t][v] <= hi)) ok &= ~(1u << (4 * t + v));      // NaN: neither holds
    }
    return ok;
}

// aq_tile_gain under the mask
template <int CRIT>
__device__ __forceinline__ double aqs_tile_gain(const double *xs, const double *__restrict__ betas_t, const double *b,
                                                const AqsModels *__restrict__ m, int draws, int dp, int quad, int col)
{
    const int ncp0 = m->ncp[0];
    double s = 0.0;
    for (int d0 = 0; d0 < dp; d0 += 16 * AQ_DT) {
        const unsigned ok = aqs_block_mask(xs, betas_t, m, dp, d0, quad, col);
        d4 acc[AQ_DT];
        draw_product<AQ_DT>(xs, betas_t, ncp0, dp, d0, quad, col, acc);
#pragma unroll
        for (int t = 0; t < AQ_DT; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int d = d0 + 16 * t + quad + 4 * v;
                const double bv = b[min(d, dp - 1)];
                if (d < draws && ((ok >> (4 * t + v)) & 1u)) s += aq_term<CRIT>(acc[t][v], bv);
            }
    }
    double G = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) G += __shfl(s, col + 16 * q, WAVE);     // the row's four quarters, in their order
    return G / (double)draws;
}

template <int CRIT, bool LAZY>
__global__ __launch_bounds__(WAVE) void acquire_system_pass_kernel(double *const *__restrict__ slot_ptr,
                                                                    const int *__restrict__ slots,
                                                                    const AqsModels *__restrict__ m,
                                                                    const double *__restrict__ betas_t, const double *b, int draws,
                                                                    int dp, int64_t n, double *g,
                                                                    const unsigned char *__restrict__ mask, const double *tau_p,
                                                                    const int64_t *cand_p, double *__restrict__ part_val,
                                                                    int64_t *__restrict__ part_idx, int *__restrict__ evals,
                                                                    double *__restrict__ trace_g,
                                                                    unsigned char *__restrict__ trace_eval)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [sum ncp][16]
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
            aqs_tile_load(xs, slot_ptr, slots, m, r, in, quad, col);
            __syncthreads();                             // one wavefront per workgroup: orders the LDS traffic
            G = aqs_tile_gain<CRIT>(xs, betas_t, b, m, draws, dp, quad, col);
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

// mode AQ_CANDIDATE: parts partials of acquire_bound_kernel -> g of the candidate's tile, tau_p, cand_p.
// mode AQ_PICK: parts partials and evals of the pass -> index_out, gain_out, tiles_out, feasible_out [pick_no], mask, b.
template <int CRIT>
__global__ __launch_bounds__(WAVE) void acquire_system_pivot_kernel(double *const *__restrict__ slot_ptr,
                                                                     const int *__restrict__ slots,
                                                                     const AqsModels *__restrict__ m,
                                                                     const double *__restrict__ betas_t, double *b, int draws,
                                                                     int dp, int64_t n, const double *__restrict__ part_val,
                                                                     const int64_t *__restrict__ part_idx, int parts,
                                                                     const int *__restrict__ evals, int mode, int pick_no,
                                                                     double *g, unsigned char *mask, double *tau_p,
                                                                     int64_t *cand_p, int64_t *__restrict__ index_out,
                                                                     double *__restrict__ gain_out,
                                                                     int64_t *__restrict__ tiles_out,
                                                                     int64_t *__restrict__ feasible_out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [sum ncp][16]
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;

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
        aqs_tile_load(xs, slot_ptr, slots, m, r, in, quad, col);
        __syncthreads();
        const double G = aqs_tile_gain<CRIT>(xs, betas_t, b, m, draws, dp, quad, col);
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
        if (none) feasible_out[pick_no] = 0;
    }
    if (none) return;
    const int cstar = (int)(best_i - tile * 16);
    const int ncp0 = m->ncp[0];
    aqs_tile_load(xs, slot_ptr, slots, m, r, in, quad, col);
    __syncthreads();
    int feasible = 0;                                // of this lane's row, in this lane's quarter of the draws
    for (int d0 = 0; d0 < dp; d0 += 16 * AQ_DT) {
        const unsigned ok = aqs_block_mask(xs, betas_t, m, dp, d0, quad, col);
        d4 acc[AQ_DT];
        draw_product<AQ_DT>(xs, betas_t, ncp0, dp, d0, quad, col, acc);
#pragma unroll
        for (int t = 0; t < AQ_DT; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int d = d0 + 16 * t + quad + 4 * v;               // draw d belongs to one lane of the picked row
                if (d < draws && ((ok >> (4 * t + v)) & 1u)) {
                    ++feasible;
                    if (col == cstar) {
                        const double f = acc[t][v];
                        if (f > b[d]) b[d] = CRIT == AQ_EI ? f : INFINITY;
                    }
                }
            }
    }
    int total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) total += __shfl(feasible, cstar + 16 * q, WAVE);     // the picked row's four lanes, in their order
    if (lane == 0) {
        feasible_out[pick_no] = total;
        mask[best_i] = 1;
    }
}

// the larger of two values; NaN if either is
__device__ __forceinline__ double aqs_nan_max(double a, double c) { return (a != a || c != c) ? (double)NAN : (a > c ? a : c); }

// part_best, part_cnt [gridDim.x][dp]: workgroup w's maximum of f over ITS rows that are feasible in draw d (-inf: none; NaN:
// one of them has an f that is not finite) and their number.  Entries d >= draws hold -inf and 0.
__global__ __launch_bounds__(WAVE) void acquire_system_incumbent_kernel(double *const *__restrict__ slot_ptr,
                                                                         const int *__restrict__ slots,
                                                                         const AqsModels *__restrict__ m,
                                                                         const double *__restrict__ betas_t, int draws, int dp,
                                                                         int64_t n, double *__restrict__ part_best,
                                                                         int64_t *__restrict__ part_cnt)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [sum ncp][16]
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int64_t n_tiles = (n + 15) / 16;
    const int ncp0 = m->ncp[0];
    double *mine_best = part_best + (size_t)blockIdx.x * dp;
    int64_t *mine_cnt = part_cnt + (size_t)blockIdx.x * dp;
    bool first = true;                               // the grid is at most the tiles: every workgroup has a first tile

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * 16 + col;
        const bool in = r < n;
        aqs_tile_load(xs, slot_ptr, slots, m, r, in, quad, col);
        __syncthreads();
        for (int d0 = 0; d0 < dp; d0 += 16 * AQ_DT) {
            const unsigned ok = aqs_block_mask(xs, betas_t, m, dp, d0, quad, col);
            d4 acc[AQ_DT];
            draw_product<AQ_DT>(xs, betas_t, ncp0, dp, d0, quad, col, acc);
#pragma unroll
            for (int t = 0; t < AQ_DT; ++t)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int d = d0 + 16 * t + quad + 4 * v;
                    const bool use = in && d < draws && ((ok >> (4 * t + v)) & 1u);     // a row past n is no row
                    const double f = acc[t][v];
                    double val = use ? (f - f == 0.0 ? f : (double)NAN) : -INFINITY;
                    int cnt = use ? 1 : 0;
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) {                           // the 16 rows: the lanes of one quarter
                        val = aqs_nan_max(val, __shfl_xor(val, off, WAVE));
                        cnt += __shfl_xor(cnt, off, WAVE);
                    }
                    if (col == 0 && d < dp) {                                          // a 16-draw tile past dp: skipped
                        mine_best[d] = first ? val : aqs_nan_max(mine_best[d], val);
                        mine_cnt[d] = first ? (int64_t)cnt : mine_cnt[d] + cnt;
                    }
                }
        }
        first = false;
        __syncthreads();                                 // the tile's LDS has been read: the next one may be stored
    }
}

__global__ __launch_bounds__(AQS_MERGE_THREADS) void acquire_system_merge_kernel(const double *__restrict__ part_best,
                                                                                  const int64_t *__restrict__ part_cnt, int parts,
                                                                                  int draws, int dp, double *__restrict__ best_out,
                                                                                  int64_t *__restrict__ count_out)
{
    const int d = blockIdx.x * AQS_MERGE_THREADS + threadIdx.x;
    if (d >= draws) return;
    double best = -INFINITY;
    int64_t cnt = 0;
    for (int k = 0; k < parts; ++k) {                    // in index order
        best = aqs_nan_max(best, part_best[(size_t)k * dp + d]);
        cnt += part_cnt[(size_t)k * dp + d];
    }
    best_out[d] = best;
    count_out[d] = cnt;
}

// The checks both entry points share, and the models as the kernels want them.  -> FOKL_OK, or the refusal.
static int aqs_models(fokl_ctx *ctx, const std::string &who, const int32_t *slots, const int32_t *widths, int n_constraints,
                      const double *betas, int draws, const double *lo, const double *hi, AqsModels *m, int *total_nc,
                      int *total_ncp)
{
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, who + ": call fokl_upload first");
    if (!slots || !widths || !betas || !lo || !hi || draws <= 0) return fail(ctx, FOKL_ERR_ARG, who + ": bad argument");
    if (n_constraints < 1 || n_constraints > AQS_MAX_MODELS - 1)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(n_constraints) + " constraint models: it takes 1 to " +
                    std::to_string(AQS_MAX_MODELS - 1) + " of them (" + std::to_string(AQS_MAX_MODELS) +
                    " models with the objective); without one use fokl_acquire_select");
    if (draws > (1 << 22)) return fail(ctx, FOKL_ERR_ARG, who + ": too many draws");
    std::memset(m, 0, sizeof *m);
    m->count = n_constraints + 1;
    int nc_sum = 0, ncp_sum = 0;
    for (int k = 0; k < m->count; ++k) {
        if (widths[k] < 1 || widths[k] > (1 << 20))
            return fail(ctx, FOKL_ERR_ARG, who + ": model " + std::to_string(k) + " has " + std::to_string(widths[k]) +
                        " columns: every model needs at least 1 (the constant)");
        m->nc[k] = widths[k];
        m->ncp[k] = (widths[k] + 3) & ~3;
        m->off[k] = ncp_sum;
        m->slot0[k] = nc_sum;
        nc_sum += m->nc[k];
        ncp_sum += m->ncp[k];
        m->lo[k] = k ? lo[k - 1] : -INFINITY;
        m->hi[k] = k ? hi[k - 1] : INFINITY;
    }
    for (int k = 0; k < n_constraints; ++k)
        if (std::isnan(lo[k]) || std::isnan(hi[k]))
            return fail(ctx, FOKL_ERR_ARG, who + ": the limits of constraint model " + std::to_string(k + 1) +
                        " hold a NaN: a limit is a number or infinite");
    const size_t lds_bytes = (size_t)ncp_sum * 16 * sizeof(double);
    if (lds_bytes > 160 * 1024)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(nc_sum) + " columns over " + std::to_string(m->count) +
                    " models, each padded to a multiple of 4, want " + std::to_string(lds_bytes) +
                    " bytes of LDS per 16-row tile, a compute unit has 163840 (at most 1280 padded columns in all)");
    for (size_t i = 0; i < (size_t)draws * nc_sum; ++i)
        if (!std::isfinite(betas[i])) return fail(ctx, FOKL_ERR_ARG, who + ": every coefficient must be finite");
    *total_nc = nc_sum;
    *total_ncp = ncp_sum;
    return FOKL_OK;
}

// the models' coefficient tables one behind the other, [ncp_k][dp] each (fokl_draw_tile.inc's format)
static void aqs_fill_tables(double *table, const AqsModels &m, const double *betas, int draws, int dp)
{
    size_t at = 0;
    for (int k = 0; k < m.count; ++k) {
        fill_draw_table(table + (size_t)m.off[k] * dp, betas + at, draws, m.nc[k], m.ncp[k], dp);
        at += (size_t)draws * m.nc[k];
    }
}

}  // namespace fokl

extern "C" int fokl_acquire_system_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_acquire_system_report: null argument");
    std::memcpy(out, ctx->acquire_system_report, sizeof ctx->acquire_system_report);
    return FOKL_OK;
}

extern "C" int fokl_acquire_system_select(fokl_ctx *ctx, const int32_t *slots, const int32_t *widths, int n_constraints,
                                          const double *betas, int draws, const double *incumbent, const double *lo,
                                          const double *hi, int criterion, int lazy, int picks, int grid_cap, int trace_pick,
                                          int64_t *index_out, double *gain_out, double *incumbent_out, int64_t *tiles_out,
                                          int64_t *feasible_out, double *trace_g_out, unsigned char *trace_eval_out)
{
    using namespace fokl;
    const std::string who = "fokl_acquire_system_select";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + ": null context");
    std::memset(ctx->acquire_system_report, 0, sizeof ctx->acquire_system_report);
    if (!incumbent || !index_out || !gain_out || !incumbent_out || !tiles_out || !feasible_out || grid_cap < 0)
        return fail(ctx, FOKL_ERR_ARG, who + ": bad argument");
    if (criterion != FOKL_ACQUIRE_EI && criterion != FOKL_ACQUIRE_PI)
        return fail(ctx, FOKL_ERR_ARG, who + ": criterion must be FOKL_ACQUIRE_EI (1) or FOKL_ACQUIRE_PI (2)");
    AqsModels models;
    int nc_sum = 0, ncp_sum = 0;
    int rc = aqs_models(ctx, who, slots, widths, n_constraints, betas, draws, lo, hi, &models, &nc_sum, &ncp_sum);
    if (rc) return rc;
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
    for (int d = 0; d < draws; ++d)
        if (std::isnan(incumbent[d]) || incumbent[d] == INFINITY)
            return fail(ctx, FOKL_ERR_ARG, who + ": every incumbent must be finite or -inf (draw " + std::to_string(d) + " is not)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = check_slots(ctx, slots, nc_sum, who.c_str());
    if (rc) return rc;

    const int dp = (draws + 15) & ~15;
    const size_t lds_bytes = (size_t)ncp_sum * 16 * sizeof(double);
    const int64_t tiles = (n + 15) / 16;
    const bool trace = trace_pick >= 0;
    const size_t table_bytes = ((size_t)ncp_sum + 1) * dp * sizeof(double);
    const size_t row_bytes = (size_t)n * (sizeof(double) * (trace ? 2 : 1) + 1) + (trace && lazy ? (size_t)tiles : 0);
    const size_t pick_bytes = (size_t)picks * 4 * sizeof(double);
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_ACQUIRE_FREE_BYTES", &free_bytes));
    if (table_bytes + row_bytes + pick_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + ": the call wants " + std::to_string(table_bytes + row_bytes + pick_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(table_bytes) +
                    " bytes of coefficients = (padded columns of all models + 1) x draws x 8, " + std::to_string(row_bytes) +
                    " per-row bytes = rows x " + std::to_string(trace ? 17 : 9) + ", " + std::to_string(pick_bytes) +
                    " of picks), the device has " + std::to_string(free_bytes) + " free (FOKL_ACQUIRE_FREE_BYTES caps what counts" +
                    (table_bytes > row_bytes ? "; thin the draws)" : "; select from the pool in parts)"));

    std::vector<double> table((size_t)ncp_sum * dp, 0.0), b0((size_t)dp, 0.0);
    aqs_fill_tables(table.data(), models, betas, draws, dp);
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
    int64_t *d_part_i = nullptr, *d_index = nullptr, *d_tiles = nullptr, *d_cand = nullptr, *d_feasible = nullptr;
    unsigned char *d_mask = nullptr, *d_trace_eval = nullptr;
    int *d_slots = nullptr, *d_evals = nullptr;
    AqsModels *d_models = nullptr;
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_b, b0.data(), b0.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc_sum));
    HIP_TRY(ctx, buf.upload(&d_models, &models, (size_t)1));
    HIP_TRY(ctx, buf.get(&d_g, (size_t)n));
    HIP_TRY(ctx, buf.get(&d_mask, (size_t)n));
    HIP_TRY(ctx, buf.get(&d_part, (size_t)parts_max));
    HIP_TRY(ctx, buf.get(&d_part_i, (size_t)parts_max));
    HIP_TRY(ctx, buf.get(&d_evals, (size_t)grid));
    HIP_TRY(ctx, buf.get(&d_index, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_tiles, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_feasible, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_gain, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_tau, (size_t)1));
    HIP_TRY(ctx, buf.get(&d_cand, (size_t)1));
    if (trace) HIP_TRY(ctx, buf.get(&d_trace_g, (size_t)n));
    if (trace && lazy) HIP_TRY(ctx, buf.get(&d_trace_eval, (size_t)tiles));
    HIP_TRY(ctx, hipMemsetAsync(d_mask, 0, (size_t)n, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_tau, 0, sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_cand, 0xff, sizeof(int64_t), ctx->stream));          // -1: no candidate's tile yet

    const bool ei = criterion == FOKL_ACQUIRE_EI;
    auto pass_full = ei ? acquire_system_pass_kernel<AQ_EI, false> : acquire_system_pass_kernel<AQ_PI, false>;
    auto pass_lazy = ei ? acquire_system_pass_kernel<AQ_EI, true> : acquire_system_pass_kernel<AQ_PI, true>;
    auto pivot = ei ? acquire_system_pivot_kernel<AQ_EI> : acquire_system_pivot_kernel<AQ_PI>;
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
        TimedRegion timed(ctx, FOKL_K_ACQUIRE_SYSTEM, 0.0, 0.0);         // bytes and flops: below, of the tiles evaluated
        auto launch_pivot = [&](int mode, int parts, int k) {
            const int m0 = split ? watch.mark() : 0;
            hipLaunchKernelGGL(pivot, dim3(1), dim3(WAVE), lds_bytes, ctx->stream, ctx->d_slot_ptr, d_slots, d_models, d_table, d_b,
                               draws, dp, n, d_part, d_part_i, parts, d_evals, mode, k, d_g, d_mask, d_tau, d_cand, d_index, d_gain,
                               d_tiles, d_feasible);
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
                               d_slots, d_models, d_table, d_b, draws, dp, n, d_g, d_mask, d_tau, d_cand, d_part, d_part_i, d_evals,
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
        for (const auto &mk : marks) sum += watch.us(mk.first, mk.second);
        return (int64_t)std::llround(sum);
    };
    const int64_t us_total = span({{total0, total1}}), us_pass = span(pass_marks), us_bound = span(bound_marks),
                  us_pivot = span(pivot_marks);
    if (e == hipSuccess) e = hipMemcpy(index_out, d_index, (size_t)picks * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(gain_out, d_gain, (size_t)picks * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(tiles_out, d_tiles, (size_t)picks * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(feasible_out, d_feasible, (size_t)picks * sizeof(int64_t), hipMemcpyDeviceToHost);
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
        const double bytes = 8.0 * 16.0 * (double)sum * nc_sum + 9.0 * (double)n * (double)(lazy ? 2 * picks - 1 : picks);
        const double flops = 2.0 * 16.0 * (double)ncp_sum * (double)draws * (double)(sum + picks);
        ctx->tslot[FOKL_K_ACQUIRE_SYSTEM].bytes += bytes;
        ctx->tslot[FOKL_K_ACQUIRE_SYSTEM].flops += flops;
        ctx->tslot[FOKL_K_ACQUIRE_SYSTEM].ideal_ms += 1e3 * std::max(bytes / FOKL_PEAK_HBM_BYTES_PER_S, flops / FOKL_PEAK_F64_FLOPS);
    }
    int64_t *rep = ctx->acquire_system_report;
    rep[0] = criterion;
    rep[1] = lazy ? 1 : 0;
    rep[2] = n_constraints;
    rep[3] = grid;
    rep[4] = grid_b;
    rep[5] = tiles;
    rep[6] = (int64_t)lds_bytes;
    rep[7] = 16 * AQ_DT;
    rep[8] = picks;
    rep[9] = launches;
    rep[10] = sum;
    rep[11] = most_lazy;
    rep[12] = us_total;
    rep[13] = us_pass;
    rep[14] = us_bound;
    rep[15] = us_pivot;
    return FOKL_OK;
}

extern "C" int fokl_acquire_system_incumbent(fokl_ctx *ctx, const int32_t *slots, const int32_t *widths, int n_constraints,
                                             const double *betas, int draws, const double *lo, const double *hi, int grid_cap,
                                             double *best_out, int64_t *count_out)
{
    using namespace fokl;
    const std::string who = "fokl_acquire_system_incumbent";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + ": null context");
    std::memset(ctx->acquire_system_report, 0, sizeof ctx->acquire_system_report);
    if (!best_out || !count_out || grid_cap < 0) return fail(ctx, FOKL_ERR_ARG, who + ": bad argument");
    AqsModels models;
    int nc_sum = 0, ncp_sum = 0;
    int rc = aqs_models(ctx, who, slots, widths, n_constraints, betas, draws, lo, hi, &models, &nc_sum, &ncp_sum);
    if (rc) return rc;
    const int64_t n = ctx->n;
    if (n <= 0) return fail(ctx, FOKL_ERR_STATE, who + ": the dataset has no rows");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = check_slots(ctx, slots, nc_sum, who.c_str());
    if (rc) return rc;

    const int dp = (draws + 15) & ~15;
    const size_t lds_bytes = (size_t)ncp_sum * 16 * sizeof(double);
    const int64_t tiles = (n + 15) / 16;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, 160 * 1024 / lds_bytes));
    int grid = (int)std::min<int64_t>(tiles, (int64_t)cu_count(ctx) * per_cu);
    if (grid_cap > 0) grid = std::min(grid, grid_cap);
    const int grid_m = (draws + AQS_MERGE_THREADS - 1) / AQS_MERGE_THREADS;
    const size_t table_bytes = (size_t)ncp_sum * dp * sizeof(double);
    const size_t part_bytes = (size_t)grid * dp * 16 + (size_t)draws * 16;
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_ACQUIRE_FREE_BYTES", &free_bytes));
    if (table_bytes + part_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + ": the call wants " + std::to_string(table_bytes + part_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(table_bytes) +
                    " bytes of coefficients = padded columns of all models x draws x 8, " + std::to_string(part_bytes) +
                    " of per-workgroup results = (workgroups + 1) x draws x 16), the device has " + std::to_string(free_bytes) +
                    " free (FOKL_ACQUIRE_FREE_BYTES caps what counts; thin the draws)");

    std::vector<double> table((size_t)ncp_sum * dp, 0.0);
    aqs_fill_tables(table.data(), models, betas, draws, dp);
    DeviceBuffers buf;
    double *d_table = nullptr, *d_part = nullptr, *d_best = nullptr;
    int64_t *d_part_c = nullptr, *d_count = nullptr;
    int *d_slots = nullptr;
    AqsModels *d_models = nullptr;
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc_sum));
    HIP_TRY(ctx, buf.upload(&d_models, &models, (size_t)1));
    HIP_TRY(ctx, buf.get(&d_part, (size_t)grid * dp));
    HIP_TRY(ctx, buf.get(&d_part_c, (size_t)grid * dp));
    HIP_TRY(ctx, buf.get(&d_best, (size_t)draws));
    HIP_TRY(ctx, buf.get(&d_count, (size_t)draws));
    HIP_TRY(ctx, lds_opt_in(acquire_system_incumbent_kernel, lds_bytes, 160 * 1024));

    hipError_t e = hipSuccess;
    StreamStopwatch watch(ctx, e);
    const double bytes = 8.0 * (double)n * nc_sum + 16.0 * (double)(2 * grid + 1) * dp;
    const double flops = 2.0 * 16.0 * (double)ncp_sum * (double)draws * (double)tiles;
    const int t0 = watch.mark();
    int t1 = t0;
    {
        TimedRegion timed(ctx, FOKL_K_ACQUIRE_SYSTEM, bytes, flops);
        hipLaunchKernelGGL(acquire_system_incumbent_kernel, dim3(grid), dim3(WAVE), lds_bytes, ctx->stream, ctx->d_slot_ptr, d_slots,
                           d_models, d_table, draws, dp, n, d_part, d_part_c);
        if (e == hipSuccess) e = hipGetLastError();
        t1 = watch.mark();
        hipLaunchKernelGGL(acquire_system_merge_kernel, dim3(grid_m), dim3(AQS_MERGE_THREADS), 0, ctx->stream, d_part, d_part_c, grid,
                           draws, dp, d_best, d_count);
        if (e == hipSuccess) e = hipGetLastError();
    }
    const int t2 = watch.mark();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    const int64_t us_total = (int64_t)std::llround(watch.us(t0, t2)), us_rows = (int64_t)std::llround(watch.us(t0, t1)),
                  us_merge = (int64_t)std::llround(watch.us(t1, t2));
    if (e == hipSuccess) e = hipMemcpy(best_out, d_best, (size_t)draws * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(count_out, d_count, (size_t)draws * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, who + ": " + hipGetErrorString(e));

    int64_t *rep = ctx->acquire_system_report;
    rep[0] = AQS_INCUMBENT;
    rep[2] = n_constraints;
    rep[3] = grid;
    rep[4] = grid_m;
    rep[5] = tiles;
    rep[6] = (int64_t)lds_bytes;
    rep[7] = 16 * AQ_DT;
    rep[9] = 2;
    rep[10] = tiles;
    rep[12] = us_total;
    rep[13] = us_rows;
    rep[14] = us_merge;
    return FOKL_OK;
}

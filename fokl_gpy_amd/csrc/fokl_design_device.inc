// design(): which rows of a candidate pool should be measured next -- greedy D- / I-optimal selection (textually included by
// fokl_hip.hip).  The statement is fokl_gpy_amd/design.py: design_host.
//
// The fitted model is linear in its coefficients: with A = G + I / tau^2 the information about them and C = A^-1, a pool row
// x_s (its basis values, ones first) has the predictive variance v_s = x_s' C x_s (in units of sigma^2) and, with M the Gram
// of a target population divided by its rows, the integrated variance w_s / (1 + v_s), w_s = x_s' (C M C) x_s, that measuring
// it would remove.  A pick x* with u = C x*, a = (C M C) x*, v* = x*' u, w* = x*' a, d = 1 + v* changes
//   C   <- C - u u' / d                                      (Sherman-Morrison)
//   CMC <- CMC - (u a' + a u') / d + u u' w* / d^2
//   v_s <- v_s - p_s^2 / d,  w_s <- w_s - 2 p_s q_s / d + p_s^2 w* / d^2     with p_s = x_s' u, q_s = x_s' a
// Three kernels, all queued on the context's stream by fokl_design_select with no host round trip between the picks:
//   design_quadform_kernel   v (and w) of every row from the matrices: the first pass and every refresh.  The draw tile's
//                            shape and tile load (fokl_draw_tile.inc) with a product of its own: one wavefront per 16-row
//                            tile, the tile's basis values in LDS [jp][16], the symmetric
//                            matrix streamed from global memory as the A operand of v_mfma_f64_16x16x4_f64, 16 of its rows
//                            at a time: D[j][row] = sum_k C[j][k] x[k][row], and each lane multiplies its D[j][row] by
//                            x[j][row] and accumulates; the four quarters of a row merge in their order.
//   design_step_kernel       one thread per row, grid-stride: the downdate of the previous pick, the criterion (masked rows
//                            -inf; compared with >, so that NaN never wins) and one (value, index) per workgroup.
//   design_pivot_kernel      one workgroup: the partials in index order, the pick, x* gathered from the slots, u, a, v*, w*
//                            and the two rank-one updates of C / CMC in device memory.
// The best of two candidates is the larger value, on equal values the lower index: associative and commutative, so neither
// the grid nor the order of a reduction changes a bit.  Nothing is accumulated with atomics.  Matrices are stored
// [jp][jp], jp = columns rounded up to 16, zero padded; the k loop runs over the columns rounded up to 4.

namespace fokl {

constexpr int DS_QT = 4;                         // 16-row blocks of the matrix per pass over k: independent MFMA chains
constexpr int DS_STEP_THREADS = 256;
constexpr int DS_PIVOT_THREADS = 1024;
constexpr int DS_MAX_COLUMNS = FOKL_DESIGN_MAX_COLUMNS;
constexpr int64_t DS_NO_ROW = INT64_MAX;

// u [jp] | a [jp] | d | w* of the last pick, as design_pivot_kernel leaves them for design_step_kernel
struct DesignState {
    double *u, *a, *scal;
};

__device__ inline bool ds_better(double v, int64_t i, double bv, int64_t bi) { return v > bv || (v == bv && i < bi); }

template <bool IVR>
__global__ __launch_bounds__(WAVE) void design_quadform_kernel(double *const *__restrict__ slot_ptr,
                                                                const int *__restrict__ slots, int nc, int ncp, int jp,
                                                                const double *__restrict__ Cm,
                                                                const double *__restrict__ CMCm, int64_t n,
                                                                double *__restrict__ v_out, double *__restrict__ w_out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [jp][16]
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int64_t n_tiles = (n + 15) / 16;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * 16 + col;
        const bool in = r < n;
        draw_tile_load(xs, slot_ptr, slots, nc, jp, r, in, quad, col);
        __syncthreads();                                 // one wavefront per workgroup: orders the LDS traffic

        double sv = 0.0, sw = 0.0;
        for (int j0 = 0; j0 < jp; j0 += 16 * DS_QT) {
            d4 acc[DS_QT], acc2[DS_QT];
            const double *a_ptr[DS_QT], *a2_ptr[DS_QT];
#pragma unroll
            for (int t = 0; t < DS_QT; ++t) {
                acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
                acc2[t] = (d4){0.0, 0.0, 0.0, 0.0};
                const size_t off = (size_t)quad * jp + min(j0 + 16 * t, jp - 16) + col;    // past jp: re-read, skipped
                a_ptr[t] = Cm + off;
                a2_ptr[t] = IVR ? CMCm + off : nullptr;
            }
            for (int k0 = 0; k0 < ncp; k0 += 4) {
                const double b = xs[(k0 + quad) * 16 + col];
                double a1[DS_QT], a2[DS_QT];
#pragma unroll
                for (int t = 0; t < DS_QT; ++t) {
                    a1[t] = a_ptr[t][(size_t)k0 * jp];       // C[k0 + quad][j + col] = C[j + col][k0 + quad]: symmetric
                    if (IVR) a2[t] = a2_ptr[t][(size_t)k0 * jp];
                }
#pragma unroll
                for (int t = 0; t < DS_QT; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[t], b, acc[t], 0, 0, 0);
                    if (IVR) acc2[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[t], b, acc2[t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < DS_QT; ++t) {
                if (j0 + 16 * t >= jp) continue;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double xj = xs[(j0 + 16 * t + quad + 4 * v) * 16 + col];   // D[j][row]: j = quad + 4 v, row = col
                    sv += acc[t][v] * xj;
                    if (IVR) sw += acc2[t][v] * xj;
                }
            }
        }
        double V = 0.0, W = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {                    // the row's four quarters, in their order
            V += __shfl(sv, col + 16 * q, WAVE);
            if (IVR) W += __shfl(sw, col + 16 * q, WAVE);
        }
        if (quad == 0 && in) {
            v_out[r] = V;
            if (IVR) w_out[r] = W;
        }
        __syncthreads();                                 // the tile's LDS has been read: the next one may be stored
    }
}

// apply: downdate v (and w) by the last pick first (0: they are fresh from design_quadform_kernel, or nothing was picked)
template <bool IVR>
__global__ __launch_bounds__(DS_STEP_THREADS) void design_step_kernel(double *const *__restrict__ slot_ptr,
                                                                       const int *__restrict__ slots, int nc, int jp,
                                                                       const double *__restrict__ u,
                                                                       const double *__restrict__ a,
                                                                       const double *__restrict__ scal, int apply,
                                                                       const unsigned char *__restrict__ mask, int64_t n,
                                                                       double *__restrict__ v, double *__restrict__ w,
                                                                       double *__restrict__ part_val,
                                                                       int64_t *__restrict__ part_idx)
{
    __shared__ double red_v[DS_STEP_THREADS / WAVE];
    __shared__ int64_t red_i[DS_STEP_THREADS / WAVE];
    const int tid = threadIdx.x;
    const double d = apply ? scal[0] : 1.0, wstar = apply ? scal[1] : 0.0;
    double best = -INFINITY;
    int64_t best_i = DS_NO_ROW;
    for (int64_t s = (int64_t)blockIdx.x * DS_STEP_THREADS + tid; s < n; s += (int64_t)gridDim.x * DS_STEP_THREADS) {
        double vs = v[s], ws = IVR ? w[s] : 0.0;
        if (apply) {
            double p = 0.0, q = 0.0;
            for (int k = 0; k < nc; ++k) {               // the slot's address and u[k], a[k] are uniform
                const double x = *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[k]] + s);
                p += x * u[k];
                if (IVR) q += x * a[k];
            }
            vs = vs - p * p / d;
            v[s] = vs;
            if (IVR) {
                ws = ws - 2.0 * p * q / d + p * p * wstar / (d * d);
                w[s] = ws;
            }
        }
        const double crit = mask[s] ? -INFINITY : (IVR ? ws / (1.0 + vs) : vs);
        if (ds_better(crit, s, best, best_i)) {
            best = crit;
            best_i = s;
        }
    }
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const double ov = __shfl_xor(best, off, WAVE);
        const int64_t oi = __shfl_xor(best_i, off, WAVE);
        if (ds_better(ov, oi, best, best_i)) {
            best = ov;
            best_i = oi;
        }
    }
    if (tid % WAVE == 0) {
        red_v[tid / WAVE] = best;
        red_i[tid / WAVE] = best_i;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < DS_STEP_THREADS / WAVE; ++k)
            if (ds_better(red_v[k], red_i[k], best, best_i)) {
                best = red_v[k];
                best_i = red_i[k];
            }
        part_val[blockIdx.x] = best;
        part_idx[blockIdx.x] = best_i;
    }
}

// sum of one value per thread over the workgroup, in a fixed tree; every thread gets it
__device__ inline double ds_block_sum(double x, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
    for (int half = DS_PIVOT_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) red[tid] += red[tid + half];
        __syncthreads();
    }
    return red[0];
}

template <bool IVR>
__global__ __launch_bounds__(DS_PIVOT_THREADS) void design_pivot_kernel(double *const *__restrict__ slot_ptr,
                                                                         const int *__restrict__ slots, int nc, int jp,
                                                                         const double *__restrict__ part_val,
                                                                         const int64_t *__restrict__ part_idx, int parts,
                                                                         int pick_no, int replicates,
                                                                         double *__restrict__ Cm, double *__restrict__ CMCm,
                                                                         double *__restrict__ u_out, double *__restrict__ a_out,
                                                                         double *__restrict__ scal, unsigned char *__restrict__ mask,
                                                                         int64_t *__restrict__ index_out,
                                                                         double *__restrict__ gain_out,
                                                                         double *__restrict__ vstar_out,
                                                                         double *__restrict__ x_out)
{
    __shared__ double xs[DS_MAX_COLUMNS], us[DS_MAX_COLUMNS], as[DS_MAX_COLUMNS];
    __shared__ double red[DS_PIVOT_THREADS];
    __shared__ int64_t red_i[DS_PIVOT_THREADS];
    const int tid = threadIdx.x;

    // the partials, in index order per thread, then a tree: the comparison is associative and commutative
    double best = -INFINITY;
    int64_t best_i = DS_NO_ROW;
    for (int k = tid; k < parts; k += DS_PIVOT_THREADS)
        if (ds_better(part_val[k], part_idx[k], best, best_i)) {
            best = part_val[k];
            best_i = part_idx[k];
        }
    red[tid] = best;
    red_i[tid] = best_i;
    __syncthreads();
    for (int half = DS_PIVOT_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half && ds_better(red[tid + half], red_i[tid + half], red[tid], red_i[tid])) {
            red[tid] = red[tid + half];
            red_i[tid] = red_i[tid + half];
        }
        __syncthreads();
    }
    best = red[0];
    best_i = red_i[0];
    const bool none = best_i == DS_NO_ROW || !(best > -INFINITY);     // nothing left to take (or every criterion NaN)

    for (int j = tid; j < jp; j += DS_PIVOT_THREADS) {
        const double x = (!none && j < nc) ? slot_ptr[slots[j]][best_i] : 0.0;
        xs[j] = x;
        if (j < nc) x_out[(size_t)pick_no * nc + j] = x;
    }
    __syncthreads();
    // u = C x*, a = CMC x*: thread j sums over k in ascending order down column j (= row j: symmetric), coalesced over j
    for (int j = tid; j < jp; j += DS_PIVOT_THREADS) {
        double su = 0.0, sa = 0.0;
        for (int k = 0; k < nc; ++k) {
            su += Cm[(size_t)k * jp + j] * xs[k];
            if (IVR) sa += CMCm[(size_t)k * jp + j] * xs[k];
        }
        us[j] = su;
        as[j] = sa;
    }
    __syncthreads();
    double pv = 0.0, pw = 0.0;
    for (int j = tid; j < jp; j += DS_PIVOT_THREADS) {
        pv += xs[j] * us[j];
        pw += xs[j] * as[j];
    }
    const double vstar = ds_block_sum(pv, red);
    const double wstar = IVR ? ds_block_sum(pw, red) : 0.0;
    const double d = 1.0 + vstar;

    for (int j = tid; j < jp; j += DS_PIVOT_THREADS) {
        u_out[j] = us[j];
        a_out[j] = as[j];
    }
    if (tid == 0) {
        scal[0] = d;
        scal[1] = wstar;
        index_out[pick_no] = none ? -1 : best_i;
        gain_out[pick_no] = best;
        vstar_out[pick_no] = vstar;
        if (!none && !replicates) mask[best_i] = 1;
    }
    // the rank-one updates; u_i u_j and u_i a_j + a_i u_j are symmetric as rounded, so the matrices stay symmetric
    const double wd2 = wstar / (d * d);
    for (int e = tid; e < jp * jp; e += DS_PIVOT_THREADS) {
        const int i = e / jp, j = e - i * jp;
        const double uu = us[i] * us[j];
        Cm[e] = Cm[e] - uu / d;
        if (IVR) CMCm[e] = CMCm[e] - (us[i] * as[j] + as[i] * us[j]) / d + uu * wd2;
    }
}

}  // namespace fokl

extern "C" int fokl_design_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_design_report: null argument");
    std::memcpy(out, ctx->design_report, sizeof ctx->design_report);
    return FOKL_OK;
}

extern "C" int fokl_design_select(fokl_ctx *ctx, const int32_t *slots, int nc, const double *C0, const double *CMC0, int picks,
                                  int replicates, int refresh_every, int grid_cap, int64_t *index_out, double *gain_out,
                                  double *vstar_out, double *x_out, double *v_out, double *w_out)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_design_select: null context");
    std::memset(ctx->design_report, 0, sizeof ctx->design_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, "fokl_design_select: call fokl_upload first");
    if (nc <= 0 || !C0 || !index_out || !gain_out || !vstar_out || !x_out || refresh_every < 0 || grid_cap < 0)
        return fail(ctx, FOKL_ERR_ARG, "fokl_design_select: bad argument");
    if (nc > FOKL_DESIGN_MAX_COLUMNS)
        return fail(ctx, FOKL_ERR_ARG, "fokl_design_select: " + std::to_string(nc) + " columns, the kernels take at most "
                    "FOKL_DESIGN_MAX_COLUMNS = " + std::to_string(FOKL_DESIGN_MAX_COLUMNS) + " (a 16-row tile of basis values "
                    "in LDS: 96 KiB)");
    if (w_out && !CMC0) return fail(ctx, FOKL_ERR_ARG, "fokl_design_select: w_out is an output of the 'ivr' criterion (CMC0)");
    const bool ivr = CMC0 != nullptr;
    const int64_t n = ctx->n;
    if (n <= 0) return fail(ctx, FOKL_ERR_STATE, "fokl_design_select: the dataset has no rows");
    if (picks < 1) return fail(ctx, FOKL_ERR_ARG, "fokl_design_select: picks must be at least 1");
    if (!replicates && (int64_t)picks > n)
        return fail(ctx, FOKL_ERR_ARG, "fokl_design_select: " + std::to_string(picks) + " picks from a pool of " +
                    std::to_string(n) + " rows need replicates");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_slots(ctx, slots, nc, "fokl_design_select");
    if (rc) return rc;

    const int ncp = (nc + 3) & ~3, jp = (nc + 15) & ~15;
    const size_t lds_bytes = (size_t)jp * 16 * sizeof(double);
    const size_t mat_doubles = (size_t)jp * jp;
    const size_t row_bytes = (size_t)n * (sizeof(double) * (ivr ? 2 : 1) + 1);
    const size_t fixed_bytes = mat_doubles * sizeof(double) * (ivr ? 2 : 1) + (size_t)picks * (nc + 3) * sizeof(double);
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_DESIGN_FREE_BYTES", &free_bytes));
    if (row_bytes + fixed_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, "fokl_design_select: the call wants " + std::to_string(row_bytes + fixed_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(row_bytes) + " per-row bytes = rows x " +
                    std::to_string(ivr ? 17 : 9) + ", " + std::to_string(fixed_bytes) + " of matrices and picks), the device has " +
                    std::to_string(free_bytes) + " free (FOKL_DESIGN_FREE_BYTES caps what counts; select from the pool in parts)");

    // matrices zero padded to [jp][jp]
    std::vector<double> mats(mat_doubles * (ivr ? 2 : 1), 0.0);
    for (int i = 0; i < nc; ++i)
        for (int j = 0; j < nc; ++j) {
            mats[(size_t)i * jp + j] = C0[(size_t)i * nc + j];
            if (ivr) mats[mat_doubles + (size_t)i * jp + j] = CMC0[(size_t)i * nc + j];
        }
    const int64_t tiles = (n + 15) / 16;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, 160 * 1024 / lds_bytes));
    int grid_q = (int)std::min<int64_t>(tiles, (int64_t)cu_count(ctx) * per_cu);
    int grid_s = (int)std::min<int64_t>((n + DS_STEP_THREADS - 1) / DS_STEP_THREADS, (int64_t)cu_count(ctx) * 8);
    if (grid_cap > 0) {
        grid_q = std::min(grid_q, grid_cap);
        grid_s = std::min(grid_s, grid_cap);
    }

    DeviceBuffers buf;
    double *d_mats = nullptr, *d_v = nullptr, *d_w = nullptr, *d_state = nullptr, *d_part = nullptr, *d_res = nullptr;
    int64_t *d_part_i = nullptr, *d_index = nullptr;
    unsigned char *d_mask = nullptr;
    int *d_slots = nullptr;
    HIP_TRY(ctx, buf.upload(&d_mats, mats.data(), mats.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc));
    HIP_TRY(ctx, buf.get(&d_v, (size_t)n));
    if (ivr) HIP_TRY(ctx, buf.get(&d_w, (size_t)n));
    HIP_TRY(ctx, buf.get(&d_mask, (size_t)n));
    HIP_TRY(ctx, buf.get(&d_state, (size_t)2 * jp + 2));
    HIP_TRY(ctx, buf.get(&d_part, (size_t)grid_s));
    HIP_TRY(ctx, buf.get(&d_part_i, (size_t)grid_s));
    HIP_TRY(ctx, buf.get(&d_index, (size_t)picks));
    HIP_TRY(ctx, buf.get(&d_res, (size_t)picks * (nc + 2)));          // gain [picks] | v* [picks] | x* [picks][nc]
    HIP_TRY(ctx, hipMemsetAsync(d_mask, 0, (size_t)n, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_state, 0, ((size_t)2 * jp + 2) * sizeof(double), ctx->stream));
    double *d_C = d_mats, *d_CMC = ivr ? d_mats + mat_doubles : nullptr;
    double *d_u = d_state, *d_a = d_state + jp, *d_scal = d_state + 2 * jp;
    double *d_gain = d_res, *d_vstar = d_res + picks, *d_x = d_res + 2 * (size_t)picks;

    auto quadform = ivr ? design_quadform_kernel<true> : design_quadform_kernel<false>;
    auto step = ivr ? design_step_kernel<true> : design_step_kernel<false>;
    auto pivot = ivr ? design_pivot_kernel<true> : design_pivot_kernel<false>;
    HIP_TRY(ctx, lds_opt_in(quadform, lds_bytes, 160 * 1024));

    // marks: the whole queue and every first-pass / refresh launch always; with timing on also every step and pivot launch
    hipError_t e = hipSuccess;
    StreamStopwatch watch(ctx, e);
    std::vector<std::pair<int, int>> q_marks, s_marks, p_marks;
    const bool split = ctx->timing;
    int refreshes = 0;
    int64_t launches = 0;
    const int total0 = watch.mark();
    {
        const double nn = (double)n, passes = 1.0 + (refresh_every ? (picks - 1) / refresh_every : 0);
        TimedRegion timed(ctx, FOKL_K_DESIGN, 8.0 * nn * ((double)nc * (passes + picks) + 4.0 * picks),
                          (ivr ? 2.0 : 1.0) * 2.0 * nn * ((double)ncp * jp * passes + (double)nc * picks));
        for (int k = 0; k < picks && e == hipSuccess; ++k) {
            const bool fresh = k == 0 || (refresh_every > 0 && k % refresh_every == 0);
            if (fresh) {
                const int m0 = watch.mark();
                hipLaunchKernelGGL(quadform, dim3(grid_q), dim3(WAVE), lds_bytes, ctx->stream, ctx->d_slot_ptr, d_slots, nc, ncp,
                                   jp, d_C, d_CMC, n, d_v, d_w);
                if (e == hipSuccess) e = hipGetLastError();
                q_marks.push_back({m0, watch.mark()});
                refreshes += k > 0;
                ++launches;
            }
            const int m1 = split ? watch.mark() : 0;
            hipLaunchKernelGGL(step, dim3(grid_s), dim3(DS_STEP_THREADS), 0, ctx->stream, ctx->d_slot_ptr, d_slots, nc, jp, d_u,
                               d_a, d_scal, fresh ? 0 : 1, d_mask, n, d_v, d_w, d_part, d_part_i);
            if (e == hipSuccess) e = hipGetLastError();
            const int m2 = split ? watch.mark() : 0;
            hipLaunchKernelGGL(pivot, dim3(1), dim3(DS_PIVOT_THREADS), 0, ctx->stream, ctx->d_slot_ptr, d_slots, nc, jp, d_part,
                               d_part_i, grid_s, k, replicates ? 1 : 0, d_C, d_CMC, d_u, d_a, d_scal, d_mask, d_index, d_gain,
                               d_vstar, d_x);
            if (e == hipSuccess) e = hipGetLastError();
            if (split) {
                s_marks.push_back({m1, m2});
                p_marks.push_back({m2, watch.mark()});
            }
            launches += 2;
        }
        if ((v_out || w_out) && e == hipSuccess) {       // v and w after the last pick: its downdate alone
            hipLaunchKernelGGL(step, dim3(grid_s), dim3(DS_STEP_THREADS), 0, ctx->stream, ctx->d_slot_ptr, d_slots, nc, jp, d_u,
                               d_a, d_scal, 1, d_mask, n, d_v, d_w, d_part, d_part_i);
            e = hipGetLastError();
            ++launches;
        }
    }
    const int total1 = watch.mark();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    auto span = [&](const std::vector<std::pair<int, int>> &marks) -> int64_t {
        double sum = 0.0;
        for (const auto &m : marks) sum += watch.us(m.first, m.second);
        return (int64_t)std::llround(sum);
    };
    const int64_t us_total = span({{total0, total1}}), us_q = span(q_marks), us_s = span(s_marks), us_p = span(p_marks);
    std::vector<double> res((size_t)picks * (nc + 2));
    if (e == hipSuccess) e = hipMemcpy(index_out, d_index, (size_t)picks * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(res.data(), d_res, res.size() * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && v_out) e = hipMemcpy(v_out, d_v, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && w_out) e = hipMemcpy(w_out, d_w, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_design_select: ") + hipGetErrorString(e));
    std::memcpy(gain_out, res.data(), (size_t)picks * sizeof(double));
    std::memcpy(vstar_out, res.data() + picks, (size_t)picks * sizeof(double));
    std::memcpy(x_out, res.data() + 2 * (size_t)picks, (size_t)picks * nc * sizeof(double));

    int64_t *rep = ctx->design_report;
    rep[0] = ivr ? FOKL_DESIGN_IVR : FOKL_DESIGN_VARIANCE;
    rep[1] = grid_q;
    rep[2] = grid_s;
    rep[3] = tiles;
    rep[4] = (int64_t)lds_bytes;
    rep[5] = picks;
    rep[6] = refreshes;
    rep[7] = launches;
    rep[8] = us_total;
    rep[9] = us_q;
    rep[10] = us_s;
    rep[11] = us_p;
    return FOKL_OK;
}

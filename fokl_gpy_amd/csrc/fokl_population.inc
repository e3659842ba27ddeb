// propagate(): a population of inputs through every posterior draw (textually included by fokl_hip.hip).
//
// The transpose of fokl_predict: the same product X betas', reduced over the ROWS for each draw.  D[row][draw] =
// X[row][:] . betas[draw][:] comes out of v_mfma_f64_16x16x4_f64 with the operands of predict_mfma_kernel swapped:
// A = the tile's basis values (lane l: row l & 15, column k0 + (l >> 4)), B = the draw coefficients (lane l: column
// k0 + (l >> 4), draw l & 15), so that lane l ends up with the rows (l >> 4) + 4 v, v = 0..3, of the ONE draw l & 15.
// A lane therefore owns its draw's accumulators for the whole launch and the row loop has no cross-lane traffic:
// sum(y - c), sum((y - c)^2), min, max, n_cuts integer counters (y > cut) and, with data, sum(e), sum(e^2), e = data - y.
//
// A wavefront owns 16 draws, the PP_WAVES wavefronts of a workgroup own neighbouring draw groups and share the tile's
// basis values through LDS ([columns][16], as predict_mfma_kernel's xs: a k-step's A fragment is 64 consecutive doubles),
// so a workgroup reads the columns once for 128 draws.  Two wavefronts per SIMD: one's compares and counters run on the
// VALU while the other's MFMAs (64 cycles each) occupy the matrix pipe.  Grid = row chunks x draw blocks, numbered so that
// the draw blocks of a chunk follow each other on one XCD (workgroups go to the XCDs in turn) and find the chunk's
// columns in its L2.
//
// Coefficients: REG keeps a wavefront's in registers (PP_KS_REG k-steps, one double per lane and step: models of up to
// 128 columns); wider models read them from the transposed table (L2) one k-step ahead and walk the columns in pieces of
// at most PP_KP, so nc is unlimited.  The next tile's basis values of a REG launch travel in registers during a tile's
// MFMAs.
//
// The four quarter-waves that hold one draw are combined once at the end (shuffles), each (row chunk, draw) writes one
// record, and population_reduce_kernel adds the chunks in their order: no floating-point atomics, the same arguments
// give the same bits.  Rows past n and draws past `draws` (padding to the workgroup's 128) contribute nothing: a row is
// masked where its values are used, a padding draw has zero coefficients and its record is never copied out.

namespace fokl {

constexpr int PP_WAVES = 8;                      // wavefronts per workgroup, 16 draws each
constexpr int PP_THREADS = PP_WAVES * WAVE;
constexpr int PP_DRAWS = PP_WAVES * 16;          // draws per workgroup
constexpr int PP_KMAX = 32;                      // cut points per draw
constexpr int PP_KS_REG = 32;                    // k-steps of 4 columns with register coefficients: ncp <= 128
constexpr int PP_PF = PP_KS_REG * 4 * 16 / PP_THREADS;   // basis values a lane carries for the next tile (REG)
constexpr int PP_KP = 1024;                      // columns per piece in LDS (128 KB)
constexpr int PP_REC = 6;                        // doubles per record: sum d, sum d^2, min, max, sum e, sum e^2

template <bool REG>
__global__ __launch_bounds__(PP_THREADS) void population_kernel(double *const *__restrict__ slot_ptr,
                                                                const int *__restrict__ slots, int nc, int ncp,
                                                                const double *__restrict__ betas_t, int draws, int ep,
                                                                const double *__restrict__ shift,
                                                                const double *__restrict__ cuts_t, int n_cuts,
                                                                const double *__restrict__ data, int64_t n,
                                                                int64_t tiles_per_chunk, int n_blocks, int n_chunks,
                                                                double *__restrict__ part_mom,
                                                                unsigned int *__restrict__ part_cnt)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int kp = min(ncp, PP_KP);
    double *xs = lds;                                // [kp][16]
    double *ys = xs + (size_t)kp * 16;               // [16]: the tile's data
    const int tid = threadIdx.x, lane = tid % WAVE, col = lane & 15, quad = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    // workgroup id -> (chunk, draw block): id = xcd + 8 (block + n_blocks * (chunk / 8)), chunk = 8 (chunk / 8) + xcd
    const int id = blockIdx.x, j = id >> 3;
    const int block = j % n_blocks, chunk = (j / n_blocks) * 8 + (id & 7);
    const int draw = block * PP_DRAWS + wave * 16 + col;             // < ep always
    const bool active = block * PP_DRAWS + wave * 16 < draws;        // wave uniform: a wavefront of padding draws only loads
    const int64_t n_tiles = (n + 15) / 16;
    const int64_t t_begin = min(n_tiles, (int64_t)chunk * tiles_per_chunk), t_end = min(n_tiles, t_begin + tiles_per_chunk);
    const int nks = ncp >> 2;

    const double c = shift[draw];
    double cut[PP_KMAX];
#pragma unroll
    for (int k = 0; k < PP_KMAX; ++k) cut[k] = k < n_cuts ? cuts_t[(size_t)k * ep + draw] : INFINITY;   // unused: never exceeded
    double b[REG ? PP_KS_REG : 1];
    if (REG) {
#pragma unroll
        for (int ks = 0; ks < PP_KS_REG; ++ks) b[ks] = ks < nks ? betas_t[(size_t)(4 * ks + quad) * ep + draw] : 0.0;
    }

    double s1 = 0.0, s2 = 0.0, mn = INFINITY, mx = -INFINITY, e1 = 0.0, e2 = 0.0;
    unsigned int cnt[PP_KMAX];
#pragma unroll
    for (int k = 0; k < PP_KMAX; ++k) cnt[k] = 0u;

    // REG: element i of a lane's share of a tile is column (tid >> 4) + 32 i, row tid & 15
    double pf[PP_PF];
    auto fetch = [&](int64_t tile) {
        const int64_t r = tile * 16 + (tid & 15);
#pragma unroll
        for (int i = 0; i < PP_PF; ++i) {
            const int k = (tid >> 4) + (PP_THREADS / 16) * i;
            pf[i] = (r < n && k < nc) ? *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[k]] + r) : 0.0;
        }
    };
    if (REG && t_begin < t_end) fetch(t_begin);

    for (int64_t tile = t_begin; tile < t_end; ++tile) {
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
        if (REG) {
#pragma unroll
            for (int i = 0; i < PP_PF; ++i) {
                const int k = (tid >> 4) + (PP_THREADS / 16) * i;
                if (k < ncp) xs[k * 16 + (tid & 15)] = pf[i];
            }
            if (data && tid < 16) ys[tid] = tile * 16 + tid < n ? data[tile * 16 + tid] : 0.0;
            __syncthreads();
            if (tile + 1 < t_end) fetch(tile + 1);               // in flight during this tile's MFMAs
            if (active) {
#pragma unroll
                for (int ks = 0; ks < PP_KS_REG; ++ks)
                    if (ks < nks)
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[(4 * ks + quad) * 16 + col], b[ks], acc, 0, 0, 0);
            }
        } else {
            for (int p0 = 0; p0 < ncp; p0 += kp) {
                const int kl = min(kp, ncp - p0);
                const int64_t r = tile * 16 + (tid & 15);
                if (p0 > 0) __syncthreads();                     // the piece before has been read
                for (int k = tid >> 4; k < kl; k += PP_THREADS / 16)
                    xs[k * 16 + (tid & 15)] = (r < n && p0 + k < nc)
                        ? *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[p0 + k]] + r) : 0.0;
                if (p0 == 0 && data && tid < 16) ys[tid] = tile * 16 + tid < n ? data[tile * 16 + tid] : 0.0;
                __syncthreads();
                if (active) {
                    const double *bp = betas_t + (size_t)(p0 + quad) * ep + draw;
                    double b_now = bp[0];
                    for (int k0 = 0; k0 < kl; k0 += 4) {
                        const int kn = k0 + 4 < kl ? k0 + 4 : k0;    // the next step's coefficient travels during this MFMA
                        const double b_next = bp[(size_t)kn * ep];
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[(k0 + quad) * 16 + col], b_now, acc, 0, 0, 0);
                        b_now = b_next;
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int rt = quad + 4 * v;
                if (tile * 16 + rt >= n) continue;               // rows past the end (the last tile only)
                const double y = acc[v], d = y - c;
                s1 += d;
                s2 = __builtin_fma(d, d, s2);
                mn = fmin(mn, y);
                mx = fmax(mx, y);
#pragma unroll
                for (int g = 0; g < PP_KMAX; g += 8)             // eight counters at a time, skipped where no cut is set
                    if (g < n_cuts) {
#pragma unroll
                        for (int k = g; k < g + 8; ++k) cnt[k] += y > cut[k] ? 1u : 0u;
                    }
                if (data) {
                    const double e = ys[rt] - y;
                    e1 += e;
                    e2 = __builtin_fma(e, e, e2);
                }
            }
        }
        __syncthreads();                                         // the tile has been read: the next one may be stored
    }

    // the four quarter-waves of a draw, in a fixed order; the first quarter writes the record
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        s1 += __shfl_xor(s1, off, WAVE);
        s2 += __shfl_xor(s2, off, WAVE);
        e1 += __shfl_xor(e1, off, WAVE);
        e2 += __shfl_xor(e2, off, WAVE);
        mn = fmin(mn, __shfl_xor(mn, off, WAVE));
        mx = fmax(mx, __shfl_xor(mx, off, WAVE));
#pragma unroll
        for (int k = 0; k < PP_KMAX; ++k) cnt[k] += __shfl_xor(cnt[k], off, WAVE);
    }
    if (quad == 0 && chunk < n_chunks) {
        double *rec = part_mom + ((size_t)chunk * ep + draw) * PP_REC;
        rec[0] = s1;
        rec[1] = s2;
        rec[2] = mn;
        rec[3] = mx;
        rec[4] = e1;
        rec[5] = e2;
        unsigned int *rc = part_cnt + ((size_t)chunk * ep + draw) * PP_KMAX;
#pragma unroll
        for (int k = 0; k < PP_KMAX; ++k)
            if (k < n_cuts) rc[k] = cnt[k];
    }
}

// One lane per (draw, value): the chunks' records in their order.  Values 0..5 are the moments, 6.. the counters.
__global__ __launch_bounds__(256) void population_reduce_kernel(const double *__restrict__ part_mom,
                                                                const unsigned int *__restrict__ part_cnt, int n_chunks,
                                                                int ep, int draws, int n_cuts, double *__restrict__ mom,
                                                                unsigned long long *__restrict__ above)
{
    const int per = PP_REC + n_cuts;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)draws * per) return;
    const int d = (int)(idx / per), f = (int)(idx % per);
    if (f < PP_REC) {
        double v = f == 2 ? INFINITY : f == 3 ? -INFINITY : 0.0;
        for (int ch = 0; ch < n_chunks; ++ch) {
            const double p = part_mom[((size_t)ch * ep + d) * PP_REC + f];
            v = f == 2 ? fmin(v, p) : f == 3 ? fmax(v, p) : v + p;
        }
        mom[(size_t)d * PP_REC + f] = v;
    } else {
        unsigned long long total = 0ull;
        for (int ch = 0; ch < n_chunks; ++ch) total += part_cnt[((size_t)ch * ep + d) * PP_KMAX + (f - PP_REC)];
        above[(size_t)d * n_cuts + (f - PP_REC)] = total;
    }
}

}  // namespace fokl

extern "C" int fokl_population_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_population_report: null argument");
    std::memcpy(out, ctx->population_report, sizeof ctx->population_report);
    return FOKL_OK;
}

extern "C" int fokl_population_stats(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, int draws,
                                     const double *shift, const double *cuts, int n_cuts, int with_data,
                                     double *moments_out, int64_t *above_out)
{
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_population_stats: null context");
    std::memset(ctx->population_report, 0, sizeof ctx->population_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, "fokl_population_stats: call fokl_upload first");
    if (nc <= 0 || draws <= 0 || !betas || !shift || !moments_out || n_cuts < 0 || n_cuts > PP_KMAX ||
        (n_cuts > 0 && (!cuts || !above_out)))
        return fail(ctx, FOKL_ERR_ARG, "fokl_population_stats: bad argument (at most 32 cut points per draw)");
    if (draws > (1 << 22) || nc > (1 << 20)) return fail(ctx, FOKL_ERR_ARG, "fokl_population_stats: too many draws or columns");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_slots(ctx, slots, nc, "fokl_population_stats");
    if (rc) return rc;
    const int64_t n = ctx->n;
    if (n <= 0) return fail(ctx, FOKL_ERR_STATE, "fokl_population_stats: the dataset has no rows");
    for (size_t i = 0; i < (size_t)draws * nc; ++i)
        if (!std::isfinite(betas[i])) return fail(ctx, FOKL_ERR_ARG, "fokl_population_stats: every coefficient must be finite");

    const int ncp = (nc + 3) & ~3;
    const int n_blocks = (draws + PP_DRAWS - 1) / PP_DRAWS, ep = n_blocks * PP_DRAWS;
    const bool reg = ncp <= 4 * PP_KS_REG;
    const int kp = std::min(ncp, PP_KP);
    const size_t lds_bytes = ((size_t)kp * 16 + 16) * sizeof(double);
    // row chunks: about two workgroups per CU over all draw blocks, each chunk a whole number of 16-row tiles
    const int64_t n_tiles = (n + 15) / 16;
    const int64_t want = std::max<int64_t>(1, ((int64_t)cu_count(ctx) * 2 + n_blocks - 1) / n_blocks);
    const int64_t tiles_per_chunk = (n_tiles + std::min(want, n_tiles) - 1) / std::min(want, n_tiles);
    const int n_chunks = (int)((n_tiles + tiles_per_chunk - 1) / tiles_per_chunk);
    const int chunks8 = (n_chunks + 7) & ~7;                    // the grid's numbering wants a multiple of the XCD count
    const int64_t grid = (int64_t)chunks8 * n_blocks;

    // argument block: slots | betas' [ncp][ep] | shift [ep] | cuts' [n_cuts][ep], zero where padded
    const size_t beta_off = ((size_t)nc * sizeof(int) + 7) & ~(size_t)7;
    const size_t arg_doubles = (size_t)ncp * ep + ep + (size_t)n_cuts * ep;
    const size_t arg_bytes = beta_off + arg_doubles * sizeof(double);
    rc = begin_args(ctx, arg_bytes);
    if (rc) return rc;
    std::memcpy(ctx->h_args, slots, (size_t)nc * sizeof(int));
    double *bt = reinterpret_cast<double *>(ctx->h_args + beta_off);
    std::memset(bt, 0, arg_doubles * sizeof(double));
    for (int d = 0; d < draws; ++d)
        for (int k = 0; k < nc; ++k) bt[(size_t)k * ep + d] = betas[(size_t)d * nc + k];
    double *sh = bt + (size_t)ncp * ep, *ct = sh + ep;
    std::memcpy(sh, shift, (size_t)draws * sizeof(double));
    for (int d = 0; d < draws; ++d)
        for (int k = 0; k < n_cuts; ++k) ct[(size_t)k * ep + d] = cuts[(size_t)d * n_cuts + k];
    rc = push_args(ctx, arg_bytes);
    if (rc) return rc;

    // records of the chunks | reduced moments | reduced counters
    const size_t rec_mom = (size_t)n_chunks * ep * PP_REC, rec_cnt = (size_t)n_chunks * ep * PP_KMAX;
    const size_t out_mom = (size_t)draws * PP_REC, out_cnt = (size_t)draws * n_cuts;
    char *d_buf = nullptr;
    const size_t cnt_off = rec_mom * sizeof(double), mom_off = cnt_off + ((rec_cnt * sizeof(unsigned int) + 7) & ~(size_t)7);
    const size_t above_off = mom_off + out_mom * sizeof(double);
    HIP_TRY(ctx, hipMalloc((void **)&d_buf, above_off + std::max<size_t>(out_cnt, 1) * sizeof(unsigned long long)));
    double *d_part_mom = reinterpret_cast<double *>(d_buf);
    unsigned int *d_part_cnt = reinterpret_cast<unsigned int *>(d_buf + cnt_off);
    double *d_mom = reinterpret_cast<double *>(d_buf + mom_off);
    unsigned long long *d_above = reinterpret_cast<unsigned long long *>(d_buf + above_off);

    auto fn = reg ? fokl::population_kernel<true> : fokl::population_kernel<false>;
    hipError_t e = lds_opt_in(fn, lds_bytes, 136 * 1024);
    if (e == hipSuccess) {
        const double *dev_betas = reinterpret_cast<const double *>(ctx->d_args + beta_off);
        const double *dev_data = with_data ? ctx->slot_ptr[FOKL_SLOT_Y] : nullptr;
        TimedRegion timed(ctx, FOKL_K_POPULATION, 8.0 * (double)n * (nc + (with_data ? 1 : 0)) * n_blocks,
                          2.0 * (double)n * ncp * draws);
        hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(fokl::PP_THREADS), lds_bytes, ctx->stream, ctx->d_slot_ptr,
                           reinterpret_cast<const int *>(ctx->d_args), nc, ncp, dev_betas, draws, ep,
                           dev_betas + (size_t)ncp * ep, dev_betas + (size_t)ncp * ep + ep, n_cuts, dev_data, n,
                           tiles_per_chunk, n_blocks, n_chunks, d_part_mom, d_part_cnt);
        e = hipGetLastError();
        if (e == hipSuccess) {
            const int64_t items = (int64_t)draws * (fokl::PP_REC + n_cuts);
            hipLaunchKernelGGL(fokl::population_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                               ctx->stream, d_part_mom, d_part_cnt, n_chunks, ep, draws, n_cuts, d_mom, d_above);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(moments_out, d_mom, out_mom * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && n_cuts > 0)
        e = hipMemcpy(above_out, d_above, out_cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d_buf);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_population_stats: ") + hipGetErrorString(e));
    int64_t *rep = ctx->population_report;
    rep[0] = reg ? FOKL_POPULATION_REGISTERS : FOKL_POPULATION_TABLE;
    rep[1] = grid;
    rep[2] = n_blocks;
    rep[3] = n_chunks;
    rep[4] = tiles_per_chunk;
    rep[5] = n_tiles;
    rep[6] = (int64_t)lds_bytes;
    rep[7] = (ncp + kp - 1) / kp;
    return FOKL_OK;
}

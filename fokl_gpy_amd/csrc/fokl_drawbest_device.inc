// optimize_pool(): for every posterior draw the best rows of a pool (textually included by fokl_hip.hip).
//
// The product of fokl_population.inc, D[row][draw] = X[row][:] . betas[draw][:], reduced over the ROWS for each draw with
// the row's index attached: A = the tile's basis values (lane l: row l & 15, column k0 + (l >> 4)), B = the draw
// coefficients (lane l: column k0 + (l >> 4), draw l & 15), so that lane l ends up with the rows (l >> 4) + 4 v, v = 0..3,
// of the ONE draw l & 15.  A lane carries its draw's running (best value, best row) in registers for the whole launch and
// the row loop has no cross-lane traffic.  The product loop is population_kernel's, copied (DESIGN: a unification to
// consider); what differs is what a lane keeps and that a tile of basis values is held in LDS whole (no pieces), so a
// model has at most FOKL_DRAWBEST_MAX_COLUMNS columns.
//
// The order is ds_better (fokl_design_device.inc): the larger value, on equal values the lower row.  It is a strict total
// order over distinct rows, so taking the best of a set is associative and commutative: neither the grid, nor the order in
// which a lane meets its rows, nor the order of the merges can change a bit.  The four quarter-waves of a draw are merged
// once at the end (shuffles), each (row chunk, draw) writes one (value, row) record and drawbest_merge_kernel takes the
// chunks in index order.  No atomics.  Rows past n, masked rows and NaN values never enter; a draw past `draws` (padding to
// the workgroup's 128) has zero coefficients and its record is never copied out.
//
// Ranks: rank r > 0 is one more pass of the same kernel with AFTER set: a candidate of draw d must also lie strictly after
// rank r - 1's (value, row) of that draw, ds_better(previous, candidate), the previous pair read once per lane from what the
// merge of round r - 1 wrote.  A draw whose previous rank found nothing stays empty.  All passes and merges of a call are
// queued on the context's stream with no host wait between them.  Registers and LDS are those of rank 0 whatever `ranks`
// is; the price is one pass per rank.

namespace fokl {

constexpr int DB_WAVES = 8;                      // wavefronts per workgroup, 16 draws each
constexpr int DB_THREADS = DB_WAVES * WAVE;
constexpr int DB_DRAWS = DB_WAVES * 16;          // draws per workgroup
constexpr int DB_KS_REG = 32;                    // k-steps of 4 columns with register coefficients: ncp <= 128
constexpr int DB_PF = DB_KS_REG * 4 * 16 / DB_THREADS;   // basis values a lane carries for the next tile (REG)
constexpr int DB_MERGE_THREADS = 256;
constexpr int64_t DB_NO_ROW = INT64_MAX;         // a running best that holds no row yet: loses against every row under ds_better

template <bool REG, bool AFTER>
__global__ __launch_bounds__(DB_THREADS) void drawbest_kernel(double *const *__restrict__ slot_ptr,
                                                              const int *__restrict__ slots, int nc, int ncp,
                                                              const double *__restrict__ betas_t, int draws, int ep,
                                                              const unsigned char *__restrict__ mask,
                                                              const double *__restrict__ prev_val,
                                                              const int64_t *__restrict__ prev_idx, int64_t n,
                                                              int64_t tiles_per_chunk, int n_blocks, int n_chunks,
                                                              double *__restrict__ part_val, int64_t *__restrict__ part_idx)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [ncp][16]
    const int tid = threadIdx.x, lane = tid % WAVE, col = lane & 15, quad = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    // workgroup id -> (chunk, draw block): id = xcd + 8 (block + n_blocks * (chunk / 8)), chunk = 8 (chunk / 8) + xcd
    const int id = blockIdx.x, j = id >> 3;
    const int block = j % n_blocks, chunk = (j / n_blocks) * 8 + (id & 7);
    const int draw = block * DB_DRAWS + wave * 16 + col;             // < ep always
    const bool active = block * DB_DRAWS + wave * 16 < draws;        // wave uniform: a wavefront of padding draws only loads
    const int64_t n_tiles = (n + 15) / 16;
    const int64_t t_begin = min(n_tiles, (int64_t)chunk * tiles_per_chunk), t_end = min(n_tiles, t_begin + tiles_per_chunk);
    const int nks = ncp >> 2;

    double b[REG ? DB_KS_REG : 1];
    if (REG) {
#pragma unroll
        for (int ks = 0; ks < DB_KS_REG; ++ks) b[ks] = ks < nks ? betas_t[(size_t)(4 * ks + quad) * ep + draw] : 0.0;
    }

    // the pair a candidate has to lie strictly after (AFTER); a draw without one takes nothing
    double pv = INFINITY;
    int64_t pi = -1;
    bool open = true;
    if (AFTER) {
        open = draw < draws;
        if (open) {
            pv = prev_val[draw];
            pi = prev_idx[draw];
            open = pi >= 0;
        }
    }
    double bv = -INFINITY;
    int64_t bi = DB_NO_ROW;

    // REG: element i of a lane's share of a tile is column (tid >> 4) + 32 i, row tid & 15
    double pf[DB_PF];
    auto fetch = [&](int64_t tile) {
        const int64_t r = tile * 16 + (tid & 15);
#pragma unroll
        for (int i = 0; i < DB_PF; ++i) {
            const int k = (tid >> 4) + (DB_THREADS / 16) * i;
            pf[i] = (r < n && k < nc) ? *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[k]] + r) : 0.0;
        }
    };
    if (REG && t_begin < t_end) fetch(t_begin);

    for (int64_t tile = t_begin; tile < t_end; ++tile) {
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
        // which of the lane's four rows are candidates at all: inside the pool and not masked (read ahead of the MFMAs)
        bool in[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t row = tile * 16 + quad + 4 * v;
            in[v] = active && open && row < n && !(mask && mask[row]);
        }
        if (REG) {
#pragma unroll
            for (int i = 0; i < DB_PF; ++i) {
                const int k = (tid >> 4) + (DB_THREADS / 16) * i;
                if (k < ncp) xs[k * 16 + (tid & 15)] = pf[i];
            }
            __syncthreads();
            if (tile + 1 < t_end) fetch(tile + 1);               // in flight during this tile's MFMAs
            if (active) {
#pragma unroll
                for (int ks = 0; ks < DB_KS_REG; ++ks)
                    if (ks < nks)
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[(4 * ks + quad) * 16 + col], b[ks], acc, 0, 0, 0);
            }
        } else {
            const int64_t r = tile * 16 + (tid & 15);
            for (int k = tid >> 4; k < ncp; k += DB_THREADS / 16)
                xs[k * 16 + (tid & 15)] = (r < n && k < nc)
                    ? *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[k]] + r) : 0.0;
            __syncthreads();
            if (active) {
                const double *bp = betas_t + (size_t)quad * ep + draw;
                double b_now = bp[0];
                for (int k0 = 0; k0 < ncp; k0 += 4) {
                    const int kn = k0 + 4 < ncp ? k0 + 4 : k0;       // the next step's coefficient travels during this MFMA
                    const double b_next = bp[(size_t)kn * ep];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[(k0 + quad) * 16 + col], b_now, acc, 0, 0, 0);
                    b_now = b_next;
                }
            }
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t row = tile * 16 + quad + 4 * v;
            const double y = acc[v];
            if (!in[v] || y != y) continue;                      // a NaN never ranks
            if (AFTER && !ds_better(pv, pi, y, row)) continue;   // not strictly after the rank before
            if (ds_better(y, row, bv, bi)) {
                bv = y;
                bi = row;
            }
        }
        __syncthreads();                                         // the tile has been read: the next one may be stored
    }

    // the four quarter-waves of a draw; the first quarter writes the record
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const double ov = __shfl_xor(bv, off, WAVE);
        const int64_t oi = __shfl_xor(bi, off, WAVE);
        if (ds_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (quad == 0 && chunk < n_chunks) {
        part_val[(size_t)chunk * ep + draw] = bv;
        part_idx[(size_t)chunk * ep + draw] = bi;
    }
}

// One lane per draw: the chunks' records in index order.  A draw that found no row: index -1, value -inf.
__global__ __launch_bounds__(DB_MERGE_THREADS) void drawbest_merge_kernel(const double *__restrict__ part_val,
                                                                          const int64_t *__restrict__ part_idx, int n_chunks,
                                                                          int ep, int draws, double *__restrict__ value,
                                                                          int64_t *__restrict__ index)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= draws) return;
    double bv = -INFINITY;
    int64_t bi = DB_NO_ROW;
    for (int ch = 0; ch < n_chunks; ++ch) {
        const double v = part_val[(size_t)ch * ep + d];
        const int64_t i = part_idx[(size_t)ch * ep + d];
        if (ds_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
    value[d] = bv;
    index[d] = bi == DB_NO_ROW ? -1 : bi;
}

}  // namespace fokl

extern "C" int fokl_drawbest_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_drawbest_report: null argument");
    std::memcpy(out, ctx->drawbest_report, sizeof ctx->drawbest_report);
    return FOKL_OK;
}

extern "C" int fokl_drawbest_rows(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, int draws,
                                  const unsigned char *mask, int ranks, int grid_cap, int64_t *index_out, double *value_out)
{
    using namespace fokl;
    const std::string who = "fokl_drawbest_rows";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + ": null context");
    std::memset(ctx->drawbest_report, 0, sizeof ctx->drawbest_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, who + ": call fokl_upload first");
    if (nc <= 0 || draws <= 0 || !betas || !index_out || !value_out || grid_cap < 0)
        return fail(ctx, FOKL_ERR_ARG, who + ": bad argument");
    if (draws > (1 << 22)) return fail(ctx, FOKL_ERR_ARG, who + ": too many draws (at most 4194304)");
    if (nc > FOKL_DRAWBEST_MAX_COLUMNS)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(nc) + " columns want " +
                    std::to_string(((size_t)((nc + 3) & ~3)) * 16 * sizeof(double)) +
                    " bytes of LDS per 16-row tile, a compute unit has 163840 (at most " +
                    std::to_string(FOKL_DRAWBEST_MAX_COLUMNS) + " columns)");
    if (ranks < 1 || ranks > FOKL_DRAWBEST_MAX_RANKS)
        return fail(ctx, FOKL_ERR_ARG, who + ": ranks must be in 1.." + std::to_string(FOKL_DRAWBEST_MAX_RANKS) + ", not " +
                    std::to_string(ranks));
    const int64_t n = ctx->n;
    if (n <= 0) return fail(ctx, FOKL_ERR_STATE, who + ": the dataset has no rows");
    for (size_t i = 0; i < (size_t)draws * nc; ++i)
        if (!std::isfinite(betas[i])) return fail(ctx, FOKL_ERR_ARG, who + ": every coefficient must be finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_slots(ctx, slots, nc, who.c_str());
    if (rc) return rc;

    const int ncp = (nc + 3) & ~3;
    const int n_blocks = (draws + DB_DRAWS - 1) / DB_DRAWS, ep = n_blocks * DB_DRAWS;
    const bool reg = ncp <= 4 * DB_KS_REG;
    const size_t lds_bytes = (size_t)ncp * 16 * sizeof(double);
    // row chunks: about two workgroups per CU over all draw blocks, each chunk a whole number of 16-row tiles
    const int64_t n_tiles = (n + 15) / 16;
    int64_t want = std::max<int64_t>(1, ((int64_t)cu_count(ctx) * 2 + n_blocks - 1) / n_blocks);
    if (grid_cap > 0) want = std::min<int64_t>(want, grid_cap);
    want = std::min(want, n_tiles);
    const int64_t tiles_per_chunk = (n_tiles + want - 1) / want;
    const int n_chunks = (int)((n_tiles + tiles_per_chunk - 1) / tiles_per_chunk);
    const int chunks8 = (n_chunks + 7) & ~7;                    // the grid's numbering wants a multiple of the XCD count
    const int64_t grid = (int64_t)chunks8 * n_blocks;
    const int grid_m = (draws + DB_MERGE_THREADS - 1) / DB_MERGE_THREADS;

    const size_t table_bytes = (size_t)ncp * ep * sizeof(double);
    const size_t row_bytes = mask ? (size_t)n : 0;
    const size_t part_bytes = (size_t)n_chunks * ep * 16;
    const size_t rank_bytes = (size_t)ranks * draws * 16;
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_ACQUIRE_FREE_BYTES", &free_bytes));
    if (table_bytes + row_bytes + part_bytes + rank_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + ": the call wants " +
                    std::to_string(table_bytes + row_bytes + part_bytes + rank_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(table_bytes) +
                    " bytes of coefficients = padded columns x padded draws x 8, " + std::to_string(row_bytes) +
                    " of the mask, " + std::to_string(part_bytes) + " of per-chunk records = chunks x padded draws x 16, " +
                    std::to_string(rank_bytes) + " of results = ranks x draws x 16), the device has " +
                    std::to_string(free_bytes) + " free (FOKL_ACQUIRE_FREE_BYTES caps what counts; thin the draws)");

    // coefficients transposed and zero padded [ncp][ep]
    std::vector<double> table((size_t)ncp * ep, 0.0);
    fill_draw_table(table.data(), betas, draws, nc, ncp, ep);

    DeviceBuffers buf;
    double *d_table = nullptr, *d_part_val = nullptr, *d_value = nullptr;
    int64_t *d_part_idx = nullptr, *d_index = nullptr;
    unsigned char *d_mask = nullptr;
    int *d_slots = nullptr;
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc));
    if (mask) HIP_TRY(ctx, buf.upload(&d_mask, mask, (size_t)n));
    HIP_TRY(ctx, buf.get(&d_part_val, (size_t)n_chunks * ep));
    HIP_TRY(ctx, buf.get(&d_part_idx, (size_t)n_chunks * ep));
    HIP_TRY(ctx, buf.get(&d_value, (size_t)ranks * draws));
    HIP_TRY(ctx, buf.get(&d_index, (size_t)ranks * draws));

    auto first = reg ? drawbest_kernel<true, false> : drawbest_kernel<false, false>;
    auto after = reg ? drawbest_kernel<true, true> : drawbest_kernel<false, true>;
    HIP_TRY(ctx, lds_opt_in(first, lds_bytes, 160 * 1024));
    HIP_TRY(ctx, lds_opt_in(after, lds_bytes, 160 * 1024));

    // marks: the whole queue always; with timing on also every launch, by kernel
    hipError_t e = hipSuccess;
    StreamStopwatch watch(ctx, e);
    std::vector<std::pair<int, int>> pass_marks, merge_marks;
    const bool split = ctx->timing;
    int64_t launches = 0;
    const double bytes = (double)ranks * ((8.0 * nc + (mask ? 1.0 : 0.0)) * (double)n * n_blocks + 32.0 * (double)n_chunks * ep);
    const double flops = (double)ranks * 2.0 * (double)n * ncp * draws;
    const int total0 = watch.mark();
    {
        TimedRegion timed(ctx, FOKL_K_DRAWBEST, bytes, flops);
        for (int r = 0; r < ranks && e == hipSuccess; ++r) {
            const double *pv = r ? d_value + (size_t)(r - 1) * draws : nullptr;
            const int64_t *pi = r ? d_index + (size_t)(r - 1) * draws : nullptr;
            const int m0 = split ? watch.mark() : 0;
            hipLaunchKernelGGL(r ? after : first, dim3((unsigned)grid), dim3(DB_THREADS), lds_bytes, ctx->stream, ctx->d_slot_ptr,
                               d_slots, nc, ncp, d_table, draws, ep, d_mask, pv, pi, n, tiles_per_chunk, n_blocks, n_chunks,
                               d_part_val, d_part_idx);
            if (e == hipSuccess) e = hipGetLastError();
            const int m1 = split ? watch.mark() : 0;
            hipLaunchKernelGGL(drawbest_merge_kernel, dim3(grid_m), dim3(DB_MERGE_THREADS), 0, ctx->stream, d_part_val, d_part_idx,
                               n_chunks, ep, draws, d_value + (size_t)r * draws, d_index + (size_t)r * draws);
            if (e == hipSuccess) e = hipGetLastError();
            if (split) {
                pass_marks.push_back({m0, m1});
                merge_marks.push_back({m1, watch.mark()});
            }
            launches += 2;
        }
    }
    const int total1 = watch.mark();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    auto span = [&](const std::vector<std::pair<int, int>> &marks) -> int64_t {
        double sum = 0.0;
        for (const auto &m : marks) sum += watch.us(m.first, m.second);
        return (int64_t)std::llround(sum);
    };
    const int64_t us_total = span({{total0, total1}}), us_pass = span(pass_marks), us_merge = span(merge_marks);
    if (e == hipSuccess) e = hipMemcpy(index_out, d_index, (size_t)ranks * draws * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(value_out, d_value, (size_t)ranks * draws * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, who + ": " + hipGetErrorString(e));

    int64_t *rep = ctx->drawbest_report;
    rep[0] = 1;
    rep[1] = ranks;
    rep[2] = n_tiles;
    rep[3] = n_chunks;
    rep[4] = n_blocks;
    rep[5] = grid;
    rep[6] = grid_m;
    rep[7] = (int64_t)lds_bytes;
    rep[8] = reg ? FOKL_POPULATION_REGISTERS : FOKL_POPULATION_TABLE;
    rep[9] = launches;
    rep[10] = tiles_per_chunk;
    rep[11] = us_total;
    rep[12] = us_pass;
    rep[13] = us_merge;
    return FOKL_OK;
}

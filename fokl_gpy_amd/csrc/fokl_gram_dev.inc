// Development builds only (make DEV=1: -DFOKL_DEV_KERNELS); fokl_hip.hip includes this file in front of launch_gram.
// Everything of a Gram call that the product library does not have: the retired kernels (K2b: round-1 rectangular panels,
// `path` 3; K2d: the tile lists on v_mfma_f64_4x4x4, FOKL_GRAM_MFMA4=2), the A/B routes of the product's two tile kernels that
// only a knob reaches (gram_tiles_kernel on blocks of three tiles or more, with several sub-chunks per chunk or two chunks
// in flight; gram_tiles_dma_kernel with a third LDS buffer or two loader wavefronts), and the knobs themselves.  With every
// knob at its default a development build runs the product's launchers (gram_dev_route answers 0).

namespace fokl {

// ---------------------------------------------------------------------------------------------------------
// K2b: Gram block on fp64 MFMA tiles (v_mfma_f64_16x16x4_f64)
// ---------------------------------------------------------------------------------------------------------
//
// Workgroup = 4 wavefronts.  Per step a chunk of GM_R rows of every column of a row-side panel (16*TI columns)
// and a column-side panel is staged in LDS as [column][GM_R + 2]; the 2-double pad makes the 16-column x 4-row
// fragment reads conflict free (bank pair = 4*col + 2*row mod 64).  Two ways of splitting the 16x16 tiles:
//   ISPLIT  (row side > 32 columns): TI == 4, wave w owns i-tile w and all TJ j-tiles (column panel 16*TJ wide)
//   !ISPLIT (row side <= 32 columns): every wave owns all TI i-tiles and the j-tiles {w, w + 4, ...}
//           (column panel 64*TJ wide)
// so the padded MFMA work stays close to the real block (56 x 58 -> 64 x 64, not 64 x 128).
// Staging uses one 16-byte load per lane (two consecutive rows of one column); the next chunk's loads are
// issued before the MFMAs of the current one (register double buffering).
//
// Operand maps (cdna_hip_programming.md section 3, f64 form): lane l supplies A[m = l & 15][k = l >> 4] and
// B[k = l >> 4][n = l & 15]; result register v of lane l is D[m = (l >> 4) + 4 v][n = l & 15].

constexpr int GM_THREADS = 256;
constexpr int GM_R = 32;
constexpr int GM_PITCH = GM_R + 2;

template <int TI, int TJ, bool ISPLIT>
__global__ __launch_bounds__(GM_THREADS) void gram_mfma_kernel(double *const *__restrict__ slot_ptr,
                                                               const int *__restrict__ row_slots, int nr,
                                                               const int *__restrict__ col_slots, int nc, int64_t n,
                                                               double *__restrict__ slab, int nr_pad, int nc_pad,
                                                               const double *__restrict__ zero_col)
{
    static_assert(!ISPLIT || TI == 4, "i-split needs one i-tile per wavefront");
    constexpr int BI = 16 * TI;
    constexpr int BJ = ISPLIT ? 16 * TJ : 64 * TJ;
    constexpr int NCOL = BI + BJ;
    constexpr int PASSES = (NCOL + 15) / 16;              // 16 columns x 16 row pairs per pass of the block
    constexpr int MI = ISPLIT ? 1 : TI;                    // i-tiles per wave
    __shared__ __attribute__((aligned(16))) double tile[NCOL * GM_PITCH];

    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int i0 = blockIdx.z * BI, j0 = blockIdx.y * BJ;

    // Column pointers of this thread's staging passes live in registers for the whole kernel; columns beyond the
    // block (padding) read a zero-filled column, so every pass is one unconditional 16-byte load and all of them
    // are in flight together (a data-dependent fix-up or branch right after a load would serialise them).
    constexpr int PCHUNK = (NCOL + 15) / 16;

    d4 acc[MI][TJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

    // staging map: thread t loads rows {2 (t & 15), 2 (t & 15) + 1} of column (t >> 4) + 16 * pass
    const int spair = tid & 15, scol = tid >> 4;
    const int64_t n_chunks = (n + GM_R - 1) / GM_R;
    const double *cp[PCHUNK];
    uint32_t padding = 0;                                  // bit p: pass p of this thread is a padding column, which re-reads
#pragma unroll                                             // the first 16 bytes of the zero column (a cache hit) instead
    for (int p = 0; p < PCHUNK; ++p) {                     // of streaming 8 N bytes of zeros per padded column
        const int c = scol + 16 * p;                       // NCOL is a multiple of 16: always a valid panel column
        const double *ptr = zero_col;
        bool real = false;
        if (c < BI) {
            if (i0 + c < nr) {
                ptr = slot_ptr[row_slots[i0 + c]];
                real = true;
            }
        } else {
            if (j0 + (c - BI) < nc) {
                ptr = slot_ptr[col_slots[j0 + (c - BI)]];
                real = true;
            }
        }
        cp[p] = ptr;
        if (!real) padding |= 1u << p;
    }
    d2 stage[PASSES];
    int64_t staged_row = 0;

    auto issue = [&](int64_t chunk) {
        const int64_t r = chunk * GM_R + 2 * spair;
        staged_row = r;
        const int64_t rc = r < n ? r : 0;                  // rows past the end are masked at commit time
#pragma unroll
        for (int p = 0; p < PASSES; ++p) stage[p] = load_d2(cp[p] + ((padding >> p) & 1u ? 0 : rc));
    };
    auto commit = [&]() {
        const bool ok0 = staged_row < n, ok1 = staged_row + 1 < n;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            d2 v = stage[p];
            if (!ok0) v.x = 0.0;
            if (!ok1) v.y = 0.0;
            *reinterpret_cast<d2 *>(&tile[(scol + 16 * p) * GM_PITCH + 2 * spair]) = v;
        }
    };

    int64_t chunk = blockIdx.x;
    if (chunk < n_chunks) issue(chunk);
    const int fm = lane & 15, fk = lane >> 4;
    while (chunk < n_chunks) {
        commit();
        __syncthreads();
        const int64_t next = chunk + gridDim.x;
        if (next < n_chunks) issue(next);
#pragma unroll
        for (int k0 = 0; k0 < GM_R; k0 += 4) {
            double af[MI], bf[TJ];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int it = ISPLIT ? wave : i;
                af[i] = tile[(16 * it + fm) * GM_PITCH + k0 + fk];
            }
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                const int jt = ISPLIT ? j : wave + 4 * j;
                bf[j] = tile[(BI + 16 * jt + fm) * GM_PITCH + k0 + fk];
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        chunk = next;
    }

    double *out = slab + (size_t)blockIdx.x * nr_pad * nc_pad;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int it = ISPLIT ? wave : i;
                const int jt = ISPLIT ? j : wave + 4 * j;
                const int gi = i0 + 16 * it + fk + 4 * v;
                const int gj = j0 + 16 * jt + fm;
                out[(size_t)gi * nc_pad + gj] = acc[i][j][v];
            }
}

// ---------------------------------------------------------------------------------------------------------
// K2d: the same tile lists on v_mfma_f64_4x4x4_4b_f64 (opt-in: FOKL_GRAM_MFMA4=2)
// ---------------------------------------------------------------------------------------------------------
//
// v_mfma_f64_4x4x4_4b_f64: four independent 4 x 4 x 4 blocks, 512 flops; 71-75 TFLOP/s in a C++ loop on register
// operands (tools/mfma_f64_peak.hip), where the same loop on the 16x16x4 form reads 47-49 -- an artefact of that loop, as
// it turned out: written in assembly the 16x16x4 form issues every 64 cycles, 78 TFLOP/s (tools/mfma_f64_issue.hip), so
// the premise of this kernel (a faster instruction) does not hold and neither did its result.  Lane maps of
// the latter (tools/mfma_f64_4x4_map.hip, by experiment): A[blk][i][k] sits in lane i + 4 blk + 16 k, B[blk][k][j]
// in lane j + 4 blk + 16 k, D[blk][i][j] in lane j + 4 blk + 16 i.  Here block blk takes the rows blk + 4 k of a
// group of 16 rows, so one instruction multiplies 4 row-side by 4 column-side columns over 16 rows; a 16 x 16 tile
// is 4 x 4 such instructions on 4 + 4 operand fragments per group of 16 rows, and its 16 accumulators hold four
// partial sums each (one per block) that are added across lanes once, at the end.  The price is registers -- 32 per
// tile instead of 8 -- so a wavefront has at most 4 tiles, a group 16 tiles on at most 8 staged column tiles (more
// groups per launch, each re-staging the columns of its i-tiles), and the LDS pitch is 32 + 8: lanes
// i + 4 blk + 16 k read element (column i, row blk + 4 k), conflict-free in both halves of a ds_read_b64 when
// 2 * pitch = 16 (mod 64); the fragment reads are volatile LDS loads, because merged into ds_read2_b64 they run at
// half the rate on 32 banks, where columns i and i + 2 of this pitch collide.
// Result (N = 1e6, back to back, us; 16x16x4 lists / this kernel): 28 x 38: 92 / 77, 56 x 58: 132 / 127,
// 56 x 80: 167 / 188, 56 x 128: 290 / 353, 56 x 176: 411 / 509, 28 x 120: 181 / 194 -- the faster instruction does
// not pay beyond the smallest blocks.  A second form (8 wavefronts, 40 tiles per group, two LDS buffers and two or
// three sets of staging registers with the loads and their s_waitcnt written by hand, the two wavefronts of a SIMD
// committing at different steps) read 295 / 455 us on 56 x 128 / 56 x 176 whatever the depth of its pipeline, its
// matrix pipe busy 55 % of the time (SQ_VALU_MFMA_BUSY_CYCLES) with the MFMAs alone worth 177 us and everything but
// the MFMAs 185 us: the two do not overlap, for a reason the counters at hand did not name.  It was withdrawn; this
// one stays for A/B runs.  The default is the 16x16x4 kernel for every launch.
constexpr int G4_PITCH = 40;
constexpr int G4S_THREADS = 256;
constexpr int G4S_MAX_NT = 4;
constexpr int G4S_MAX_CT = 8;

template <int NT, int P>
__global__ __launch_bounds__(G4S_THREADS, 2) void gram_tiles4s_kernel(double *const *__restrict__ slot_ptr,
                                                                      const int *__restrict__ icols, int nci,
                                                                      const GramGroup *__restrict__ groups, int ct_count,
                                                                      int64_t n, double *__restrict__ slab, int nr_pad,
                                                                      int nc_pad, const double *__restrict__ zero_col,
                                                                      const double *__restrict__ base)
{
    extern __shared__ __attribute__((aligned(16))) double g4s_tile[];
    constexpr int R = 32, pitch = G4_PITCH;
    const GramGroup &g = groups[blockIdx.y];
    const int tid = threadIdx.x, lane = tid % WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int spair = tid & 15, scol = tid >> 4;               // pass p: column scol of the group's p-th column tile

    uint32_t cb[P];
    uint32_t padding = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const uint32_t u = p < ct_count ? g.col_units[p][scol] : 0x80000000u;
        cb[p] = u & 0x7fffffffu;
        padding |= (u >> 31) << p;
    }

    const int frag = (lane & 3) * pitch + ((lane >> 2) & 3) + 4 * (lane >> 4);
    int aoff[NT], boff[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        aoff[k] = frag + 16 * (int)g.a[wave][k] * pitch;
        boff[k] = frag + 16 * (int)g.b[wave][k] * pitch;
    }
    int real_tiles = 0;
#pragma unroll
    for (int k = 0; k < NT; ++k) real_tiles += g.oi[wave][k] != 0xFFFF ? 1 : 0;
    real_tiles = __builtin_amdgcn_readfirstlane(real_tiles);
    double acc[NT][4][4];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int ia = 0; ia < 4; ++ia)
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) acc[k][ia][jb] = 0.0;

    const int64_t n_chunks = (n + R - 1) / R;
    const int64_t stride = gridDim.x;
    d2 stage[P];

    auto issue = [&](int64_t chunk) {
        const int64_t r = chunk * R + 2 * spair;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int64_t rc = ((padding >> p) & 1u) || r >= n ? 0 : r;
            uint32_t units = cb[p];
            asm volatile("" : "+v"(units));
            stage[p] = load_d2(base + ((size_t)units << 5) + rc);
        }
    };
    auto commit = [&](int64_t chunk) {
        const int64_t r = chunk * R + 2 * spair;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            d2 v = stage[p];
            if (r >= n) v.x = 0.0;
            if (r + 1 >= n) v.y = 0.0;
            *reinterpret_cast<d2 *>(&g4s_tile[(16 * p + scol) * pitch + 2 * spair]) = v;
        }
    };
    auto multiply = [&]() {
        constexpr int STEPS = 2 * NT;
        double af[2][4], bf[2][4];
        typedef __attribute__((address_space(3))) const volatile double lds_cv_double;
        lds_cv_double *lds_v = (lds_cv_double *)g4s_tile;
        auto fetch = [&](int s, int buf) {
            const int k = s % NT, rows = 16 * (s / NT);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                af[buf][q] = lds_v[aoff[k] + 4 * q * pitch + rows];      // (volatile: see above)
                bf[buf][q] = lds_v[boff[k] + 4 * q * pitch + rows];
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            if (s + 1 < STEPS) fetch(s + 1, (s + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            if (s % NT < real_tiles) {
#pragma unroll
                for (int ia = 0; ia < 4; ++ia)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb)
                        acc[s % NT][ia][jb] = __builtin_amdgcn_mfma_f64_4x4x4f64(af[s & 1][ia], bf[s & 1][jb],
                                                                                acc[s % NT][ia][jb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    int64_t chunk = blockIdx.x;
    if (chunk < n_chunks) issue(chunk);
    while (chunk < n_chunks) {
        commit(chunk);
        __syncthreads();
        const int64_t next = chunk + stride;
        if (next < n_chunks) issue(next);
        multiply();
        __syncthreads();
        chunk = next;
    }

    double *out = slab + (size_t)blockIdx.x * nr_pad * nc_pad;
    asm volatile("" ::: "memory");
    const int dj = lane & 3, di = lane >> 4;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int oi = g.oi[wave][k], oj = g.oj[wave][k];
#pragma unroll
        for (int ia = 0; ia < 4; ++ia)
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) {
                double v = acc[k][ia][jb];
                v += __shfl_xor(v, 4, WAVE);
                v += __shfl_xor(v, 8, WAVE);
                if (oi != 0xFFFF && (lane & 12) == 0)
                    out[(size_t)(16 * oi + 4 * ia + di) * nc_pad + 16 * oj + 4 * jb + dj] = v;
            }
    }
}

}  // namespace fokl

// ---- the knobs: the environment laid over the product's configuration, read anew for every call --------------

static LaunchKnobs launch_knobs()
{
    LaunchKnobs k;
    k.path = env_int("FOKL_GRAM_PATH", k.path);
    k.mfma4 = env_int("FOKL_GRAM_MFMA4", k.mfma4);
    k.dma = env_int("FOKL_GRAM_DMA", k.dma);
    k.half = env_int("FOKL_GRAM_HALF", k.half);
    k.bufs = env_int("FOKL_GRAM_BUFS", k.bufs) == 3 ? 3 : 2;
    k.loaders = env_int("FOKL_GRAM_LOADERS", k.loaders);
    if (k.loaders != 2 && k.loaders != 4) k.loaders = 0;
    k.rb = std::max(1, std::min(16, env_int("FOKL_GRAM_RB", k.rb)));
    k.depth = std::max(1, std::min(2, env_int("FOKL_GRAM_DEPTH", k.depth)));
    k.wgs = std::max(1, env_int("FOKL_GRAM_WGS", k.wgs));
    k.k1_wgs = std::max(1, env_int("FOKL_K1_WGS", k.k1_wgs));
    k.tiles4_nt = G4S_MAX_NT;
    k.tiles4_ct = G4S_MAX_CT;
    return k;
}

// One instantiation per tile configuration; the dispatcher below picks the smallest that covers the block.
typedef void (*gram_mfma_fn)(double *const *, const int *, int, const int *, int, int64_t, double *, int, int,
                             const double *);

template <int TJ>
static gram_mfma_fn pick_isplit()
{
    return gram_mfma_kernel<4, TJ, true>;
}

static gram_mfma_fn isplit_kernel(int tj)
{
    switch (tj) {
        case 1: return pick_isplit<1>();
        case 2: return pick_isplit<2>();
        case 3: return pick_isplit<3>();
        case 4: return pick_isplit<4>();
        case 5: return pick_isplit<5>();
        case 6: return pick_isplit<6>();
        case 7: return pick_isplit<7>();
        case 8: return pick_isplit<8>();
        case 9: return pick_isplit<9>();
        case 10: return pick_isplit<10>();
        case 11: return pick_isplit<11>();
        default: return pick_isplit<12>();
    }
}

static gram_mfma_fn jsplit_kernel(int ti, int tj)
{
    if (ti == 1) {
        if (tj == 1) return gram_mfma_kernel<1, 1, false>;
        if (tj == 2) return gram_mfma_kernel<1, 2, false>;
        return gram_mfma_kernel<1, 3, false>;
    }
    if (tj == 1) return gram_mfma_kernel<2, 1, false>;
    if (tj == 2) return gram_mfma_kernel<2, 2, false>;
    return gram_mfma_kernel<2, 3, false>;
}


// Instantiations: NT = 1..4 (HBM-bound shapes) for P = 4, 8, 16 staging passes and one or two chunks in flight, the
// k-split teams (NT = 1) likewise; NT = 5..10 (MFMA-bound) for P = 16, one chunk in flight.
template <int NT, int P>
static gram_tiles_fn tiles_kernel_np(int depth, int ks)
{
    if (NT == 1 && ks == 4) return depth == 2 ? gram_tiles_kernel<1, P, 2, 4> : gram_tiles_kernel<1, P, 1, 4>;
    if (NT == 1 && ks == 2) return depth == 2 ? gram_tiles_kernel<1, P, 2, 2> : gram_tiles_kernel<1, P, 1, 2>;
    if (depth == 2) return gram_tiles_kernel<NT, P, 2, 1>;
    return gram_tiles_kernel<NT, P, 1, 1>;
}

template <int NT>
static gram_tiles_fn tiles_kernel_n(int passes, int depth, int ks)
{
    if (passes <= 4) return tiles_kernel_np<NT, 4>(depth, ks);
    if (passes <= 8) return tiles_kernel_np<NT, 8>(depth, ks);
    return tiles_kernel_np<NT, 16>(depth, ks);
}

static gram_tiles_fn tiles_kernel(int nt, int passes, int depth, int ks)
{
    switch (nt) {
        case 1: return tiles_kernel_n<1>(passes, depth, ks);
        case 2: return tiles_kernel_n<2>(passes, depth, ks);
        case 3: return tiles_kernel_n<3>(passes, depth, ks);
        case 4: return tiles_kernel_n<4>(passes, depth, ks);
        case 5: return gram_tiles_kernel<5, 16, 1, 1>;
        case 6: return gram_tiles_kernel<6, 16, 1, 1>;
        case 7: return gram_tiles_kernel<7, 16, 1, 1>;
        case 8: return gram_tiles_kernel<8, 16, 1, 1>;
        case 9: return gram_tiles_kernel<9, 16, 1, 1>;
        default: return gram_tiles_kernel<10, 16, 1, 1>;
    }
}

typedef void (*gram_tiles4_fn)(double *const *, const int *, int, const GramGroup *, int, int64_t, double *, int, int,
                               const double *, const double *);

template <int NT>
static gram_tiles4_fn tiles4s_kernel_n(int passes)
{
    if (passes <= 2) return gram_tiles4s_kernel<NT, 2>;
    if (passes <= 4) return gram_tiles4s_kernel<NT, 4>;
    if (passes <= 6) return gram_tiles4s_kernel<NT, 6>;
    return gram_tiles4s_kernel<NT, 8>;
}

static gram_tiles4_fn tiles4s_kernel(int nt, int passes)
{
    switch (nt) {
        case 1: return tiles4s_kernel_n<1>(passes);
        case 2: return tiles4s_kernel_n<2>(passes);
        case 3: return tiles4s_kernel_n<3>(passes);
        default: return tiles4s_kernel_n<4>(passes);
    }
}


// gram_tiles_dma_kernel with a third LDS buffer (a chunk's pieces in flight across the barrier; the matrix wavefronts load) or
// with two loader wavefronts; the product's own otherwise
static gram_dma_fn tiles_dma_kernel_ab(int nt8, bool half, int nbuf, int loaders)
{
    if (nbuf == 3) return loaders == 0 ? tiles_dma_kernel_b<3, 0>(nt8, half) : nullptr;
    if (nbuf == 2 && loaders == 2) return tiles_dma_kernel_b<2, 2>(nt8, half);
    return tiles_dma_kernel(nt8, half, nbuf, loaders);
}

// Path 3, gram_mfma_kernel: rectangular panels, one i-tile or j-tile set per wavefront
static int launch_gram_panel(fokl_ctx *ctx, const GramCall &c, GramLaunch &run)
{
    const int *d_rows, *d_cols;
    int rc = push_slot_lists(ctx, c, d_rows, d_cols);
    if (rc) return rc;
    const int nr = c.nr, nc = c.nc;
    gram_mfma_fn mfma_fn = nullptr;
    int BI, BJ;
    const int j_tiles = (nc + 15) / 16;
    if (nr > 32) {                                   // i-split: wave w <-> i-tile w, panel of TJ j-tiles
        const int panels = (j_tiles + 11) / 12;
        const int tj = (j_tiles + panels - 1) / panels;
        mfma_fn = isplit_kernel(tj);
        BI = 64;
        BJ = 16 * tj;
    } else {                                         // j-split: every wave all i-tiles, j-tiles dealt over waves
        const int ti = nr > 16 ? 2 : 1;
        const int per_wave = (j_tiles + 3) / 4;
        const int panels = (per_wave + 2) / 3;
        const int tj = (per_wave + panels - 1) / panels;
        mfma_fn = jsplit_kernel(ti, tj);
        BI = 16 * ti;
        BJ = 64 * tj;
    }
    const int gz = (nr + BI - 1) / BI, gy = (nc + BJ - 1) / BJ;
    run.nr_pad = gz * BI;
    run.nc_pad = gy * BJ;
    const int64_t n_chunks = (ctx->n + GM_R - 1) / GM_R;
    const int per_cu = blocks_per_cu(mfma_fn, GM_THREADS, 0);
    const int target = std::max(1, (per_cu * cu_count(ctx)) / (gz * gy));
    rc = size_slabs(ctx, run, (int)std::max<int64_t>(1, std::min<int64_t>(n_chunks, target)), 1, n_chunks);
    if (rc) return rc;
    run.rep[0] = FOKL_GRAM_PANEL, run.rep[5] = run.rep[6] = 1, run.rep[7] = GM_R, run.rep[8] = gy * gz;
    run.rep[21] = GM_THREADS;
    TimedRegion timed(ctx, c.slot, c.bytes, c.flops);      // brackets the Gram kernel only
    hipLaunchKernelGGL(mfma_fn, dim3(run.S, gy, gz), dim3(GM_THREADS), 0, ctx->stream, ctx->d_slot_ptr, d_rows, nr, d_cols,
                       nc, ctx->n, ctx->d_slab, run.nr_pad, run.nc_pad, ctx->d_zero);
    return FOKL_OK;
}

// FOKL_GRAM_MFMA4=2, gram_tiles4s_kernel: the 4x4x4 form of the fp64 MFMA instruction (slower beyond the smallest blocks)
static int launch_gram_tiles4(fokl_ctx *ctx, const GramCall &c, GramLaunch &run, int wgs_cap)
{
    const GramPlan &pl = run.plan;
    const int P = pl.ct <= 2 ? 2 : pl.ct <= 4 ? 4 : pl.ct <= 6 ? 6 : 8;
    gram_tiles4_fn fn = tiles4s_kernel(pl.nt, pl.ct);
    const size_t lds = (size_t)P * 16 * G4_PITCH * sizeof(double);
    int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(fn), lds);
    if (rc) return rc;
    const int64_t n_chunks = (ctx->n + 31) / 32;
    const int per_cu = std::min(wgs_cap, blocks_per_cu(fn, G4S_THREADS, lds));
    const int target = std::max(1, (per_cu * cu_count(ctx)) / (int)pl.groups.size());      // (A/B kernel: no pinned row cut)
    rc = size_slabs(ctx, run, (int)std::max<int64_t>(1, std::min<int64_t>(n_chunks, target)), 1, n_chunks);
    if (rc) return rc;
    run.rep[0] = FOKL_GRAM_TILES4, run.rep[1] = pl.nt, run.rep[7] = 32, run.rep[12] = (int64_t)lds, run.rep[21] = G4S_THREADS;
    TimedRegion timed(ctx, c.slot, c.bytes, c.flops);      // brackets the Gram kernel only
    hipLaunchKernelGGL(fn, dim3(run.S, (unsigned)pl.groups.size()), dim3(G4S_THREADS), lds, ctx->stream, ctx->d_slot_ptr,
                       run.d_icols, pl.nci, run.d_groups, pl.ct, ctx->n, ctx->d_slab, run.nr_pad, run.nc_pad, ctx->d_zero,
                       run.grid_base);
    return FOKL_OK;
}

// The hook of launch_gram: a call the knobs send off the product's route is launched here (taken), any other is left alone.
static int launch_gram_dev(fokl_ctx *ctx, const GramCall &c, const LaunchKnobs &k, int path, GramLaunch &run, bool &taken)
{
    const GramPlan &pl = run.plan;
    taken = true;
    if (path == 3) return launch_gram_panel(ctx, c, run);
    if (pl.kind == 1) return launch_gram_tiles4(ctx, c, run, k.wgs);
    // FOKL_GRAM_DMA=1: LDS-DMA staging only for the launches the matrix pipe bounds, 0: gram_tiles_kernel for every block.  Its
    // row cut there (ks 1) is the occupancy query's on this device's CUs, as it was before the cut was pinned
    if (pl.ks == 1 && k.dma != 2 && !(k.dma == 1 && c.slot == FOKL_K_GRAM_MFMA)) {
        gram_tiles_fn fn = tiles_kernel(pl.nt, pl.ct << pl.rb_shift, pl.depth, 1);
        const size_t lds = (size_t)pl.ct * 16 * ((32 << pl.rb_shift) + 2) * sizeof(double);
        return launch_gram_tiles(ctx, c, run, fn, k.wgs, blocks_per_cu(fn, GT_THREADS, lds), cu_count(ctx));
    }
    // FOKL_GRAM_RB, FOKL_GRAM_DEPTH: the k-split teams with several sub-chunks per chunk or two chunks in flight: three
    // workgroups per CU by registers except with 16 staging passes and two chunks in flight (187 VGPRs: two)
    if (pl.ks > 1 && (pl.rb_shift != 0 || pl.depth != 1)) {
        const int passes = pl.ct << pl.rb_shift;
        return launch_gram_tiles(ctx, c, run, tiles_kernel(pl.nt, passes, pl.depth, pl.ks), k.wgs, passes > 8 && pl.depth == 2 ? 2 : 3);
    }
    // FOKL_GRAM_BUFS=3: a third LDS buffer where three fit 160 KB (the matrix wavefronts load); FOKL_GRAM_LOADERS=2
    const size_t pieces = (pl.ct * 16 * 34 * 8 + 1023) / 1024;
    const int nbuf = k.bufs == 3 && 3 * pieces * 1024 <= 160 * 1024 ? 3 : 2;
    if (pl.ks == 1 && (nbuf == 3 || k.loaders == 2))
        return launch_gram_dma(ctx, c, run, tiles_dma_kernel_ab, k.wgs, nbuf, nbuf == 2 ? k.loaders : 0);
    taken = false;
    return FOKL_OK;
}

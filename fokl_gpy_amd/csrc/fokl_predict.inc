// evaluate(): posterior-mean prediction and order-statistic bounds (textually included by fokl_hip.hip).
//
// Replaces FoKLRoutines.py:966-978: modells = X betas', mean over draws, and per row the `cut`-th smallest /
// largest draw.  One wavefront per 64 rows; a row's basis values sit in LDS as [column][lane], the draw
// coefficients are wave-uniform (scalar loads), four draws are accumulated at a time, and each lane keeps
// its cut + 1 smallest and cut largest predictions in two small sorted LDS lists.
//
// Predictions that are not finite keep numpy's order: +-inf are numbers like any other, NaN sorts last.  A NaN passes
// neither of the lists' strict comparisons, so it is counted per row instead, and with D of them the bounds read out are
// NaN where sorted[cut] / sorted[draws - cut] lie among the NaN (draws - D <= cut / D >= cut) and else the klo-th smallest and
// the (khi - D)-th largest number (tests/test_predict_nonfinite_gpu.py).  predict_mfma_kernel below counts nothing: after
// it, predict_flag_kernel looks for a mean that is not finite (such a row holds a NaN or an infinity, or its sum overflowed),
// and if there is one this kernel runs once more with `repair` set, over the 64-row blocks that hold such a row, and
// writes those rows again.

namespace fokl {

constexpr int PR_THREADS = 64;
constexpr int PR_MAX_K = 128;

// GLOBAL_LISTS: the two sorted lists of a wavefront live in device memory (`lists`, (klo + khi) x 64 doubles per
// workgroup) instead of LDS -- bounds over more than ~5 000 draws need the 128-th and later order statistics, more than
// LDS holds next to the basis values.  Slow (every insertion shifts through L2) and rare; same arithmetic, same result.
// GLOBAL_X: a model too wide for its rows' basis values to sit in LDS (about 300 terms) reads them from the columns
// themselves, PR_XG at a time so that the loads travel together: once per group of four draws, i.e. once for the
// mean-only call, out of L2 after that (64 rows x nc doubles per wavefront).  Same order of summation.
constexpr int PR_XG = 8;

template <bool GLOBAL_LISTS, bool GLOBAL_X>
__global__ __launch_bounds__(PR_THREADS) void predict_kernel(double *const *__restrict__ slot_ptr,
                                                             const int *__restrict__ slots, int nc,
                                                             const double *__restrict__ betas, int draws, int klo,
                                                             int khi, int64_t n, double *__restrict__ mean,
                                                             double *__restrict__ bounds, double *__restrict__ lists,
                                                             int repair)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xrow = lds;                              // [nc][64] (none with GLOBAL_X)
    // [klo][64] ascending: lo[klo-1] is the klo-th smallest so far; [khi][64] descending: hi[khi-1] the khi-th largest
    double *lo = GLOBAL_LISTS ? lists + (size_t)blockIdx.x * (klo + khi) * PR_THREADS
                              : xrow + (GLOBAL_X ? 0 : (size_t)nc * PR_THREADS);
    double *hi = lo + (size_t)klo * PR_THREADS;
    const int lane = threadIdx.x;
    const bool want_bounds = bounds != nullptr;

    for (int64_t base = (int64_t)blockIdx.x * PR_THREADS; base < n; base += (int64_t)gridDim.x * PR_THREADS) {
        const int64_t r = base + lane;
        const bool in = r < n;
        bool mine = in;                                  // the rows this pass writes
        if (repair) {
            mine = in && !(fabs(mean[r]) < INFINITY);
            if (!__any(mine)) continue;                  // wave-uniform: nothing to repair in this block
        }
        if (!GLOBAL_X)
            for (int j = 0; j < nc; ++j)
                xrow[j * PR_THREADS + lane] = in ? *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[j]] + r) : 0.0;
        if (want_bounds) {
            for (int k = 0; k < klo; ++k) lo[k * PR_THREADS + lane] = INFINITY;
            for (int k = 0; k < khi; ++k) hi[k * PR_THREADS + lane] = -INFINITY;
        }
        double total = 0.0;
        int n_nan = 0;                                   // NaN predictions of this row: they enter neither list
        for (int d0 = 0; d0 < draws; d0 += 4) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const int nd = min(4, draws - d0);
            if (GLOBAL_X) {
                const int64_t rx = in ? r : n - 1;           // a lane past the end reads the last row; it stores nothing
                int j = 0;
                for (; j + PR_XG <= nc; j += PR_XG) {
                    double xg[PR_XG];
#pragma unroll
                    for (int u = 0; u < PR_XG; ++u)
                        xg[u] = *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[j + u]] + rx);
#pragma unroll
                    for (int u = 0; u < PR_XG; ++u)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (q < nd) acc[q] = __builtin_fma(betas[(size_t)(d0 + q) * nc + j + u], xg[u], acc[q]);
                }
                for (; j < nc; ++j) {
                    const double xv = *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[j]] + rx);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nd) acc[q] = __builtin_fma(betas[(size_t)(d0 + q) * nc + j], xv, acc[q]);
                }
            } else {
                for (int j = 0; j < nc; ++j) {
                    const double xv = xrow[j * PR_THREADS + lane];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nd) acc[q] = __builtin_fma(betas[(size_t)(d0 + q) * nc + j], xv, acc[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q >= nd) break;
                const double v = acc[q];
                total += v;
                if (want_bounds) {
                    n_nan += v != v;
                    if (v < lo[(klo - 1) * PR_THREADS + lane]) {       // insert into the ascending list
                        int k = klo - 1;
                        while (k > 0 && lo[(k - 1) * PR_THREADS + lane] > v) {
                            lo[k * PR_THREADS + lane] = lo[(k - 1) * PR_THREADS + lane];
                            --k;
                        }
                        lo[k * PR_THREADS + lane] = v;
                    }
                    if (v > hi[(khi - 1) * PR_THREADS + lane]) {       // insert into the descending list
                        int k = khi - 1;
                        while (k > 0 && hi[(k - 1) * PR_THREADS + lane] < v) {
                            hi[k * PR_THREADS + lane] = hi[(k - 1) * PR_THREADS + lane];
                            --k;
                        }
                        hi[k * PR_THREADS + lane] = v;
                    }
                }
            }
        }
        if (mine) {
            mean[r] = total / (double)draws;
            if (want_bounds) {
                // numpy's order, NaN last: the klo-th smallest is a number while klo numbers exist, and the khi-th largest
                // of all is the (khi - n_nan)-th largest number
                bounds[2 * r] = draws - n_nan >= klo ? lo[(klo - 1) * PR_THREADS + lane] : NAN;
                bounds[2 * r + 1] = n_nan < khi ? hi[(khi - 1 - n_nan) * PR_THREADS + lane] : NAN;
            }
        }
    }
}

// 1 into *flag if a mean is not finite (all such lanes store the same value): whether predict_mfma_kernel's rows need the
// repair pass above.
__global__ __launch_bounds__(256) void predict_flag_kernel(const double *__restrict__ mean, int64_t n,
                                                           unsigned long long *__restrict__ flag)
{
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        any |= !(fabs(mean[i]) < INFINITY);
    if (any) *flag = 1ull;
}

// The same on the matrix pipe, for the case that costs: bounds over many draws.  One wavefront per tile of 16 rows, the
// tile's basis values in LDS [term][row], and D[draw][row] = betas[draw][:] . X[row][:] in blocks of PM_DT x 16 draws: the
// draw tile's product (fokl_draw_tile.inc: the coefficient table, the lane map and what happens past the last draw); a lane
// ends up with a quarter of the draws of one row.
//
// Order statistics without sorting a thousand values per row: the row's predictions have mean x'mean(beta) and
// variance x'Cov(beta)x (O(P^2) per row, against O(P draws) for the predictions), so only values beyond
// mean -/+ z sigma can be among the klo smallest / khi largest -- z is chosen so that about twice as many are
// expected.  Those few are appended (no loop, so no divergence) to per-lane candidate buffers; afterwards every lane
// sorts its handful and the four quarters of a row are merged up to the klo-th / khi-th value.  A row with too few
// candidates, or a lane with more than PM_CAP, sends the tile through the exact fallback: the same pass with
// per-lane sorted lists of the klo / khi best kept up to date draw by draw, merged the same way.  What a launch did is
// counted for fokl_predict_report: tally[0] += the tiles a wavefront processed (lane 0, once, at its end), tally[1] += 1
// for a tile on its way into the fallback (lane 0; nothing is counted inside the filter pass itself).
// NaN is no concern of this kernel: its lists take numbers only, and rows with one are written again by predict_kernel's
// repair pass.  (With a coefficient that is not finite the host's moments are NaN, nothing passes the filter and every tile
// takes the fallback.)
constexpr int PM_THREADS = 64;
constexpr int PM_DT = 4;
constexpr int PM_CAP = 32;

__global__ __launch_bounds__(PM_THREADS) void predict_mfma_kernel(double *const *__restrict__ slot_ptr,
                                                                  const int *__restrict__ slots, int nc, int ncp,
                                                                  const double *__restrict__ betas_t, int draws, int dp,
                                                                  const double *__restrict__ beta_mean,
                                                                  const double *__restrict__ beta_cov, double z,
                                                                  int klo, int khi, int64_t n,
                                                                  double *__restrict__ mean, double *__restrict__ bounds,
                                                                  unsigned long long *__restrict__ tally)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int cap = max(PM_CAP, max(klo, khi));      // rows of the two buffers (the fallback keeps klo / khi per lane)
    double *xs = lds;                                // [ncp][16]
    double *lo = xs + (size_t)ncp * 16;              // [cap][64]: candidates below, or the ascending list of the fallback
    double *hi = lo + (size_t)cap * PM_THREADS;      // [cap][64]: candidates above, or the descending list
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int64_t n_tiles = (n + 15) / 16;
    int64_t tile = blockIdx.x;

    for (; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * 16 + col;
        const bool in = r < n;
        draw_tile_load(xs, slot_ptr, slots, nc, ncp, r, in, quad, col);
        __syncthreads();                                 // one wavefront per workgroup: orders the LDS traffic

        // moments of this row's predictions over the draws; the covariance entries are wave uniform (scalar loads)
        double mu = 0.0, var = 0.0;
        for (int i = 0; i < nc; ++i) {
            const double xi = xs[i * 16 + col];
            double dot = 0.0;
            for (int j = 0; j < nc; ++j) dot = __builtin_fma(beta_cov[i * ncp + j], xs[j * 16 + col], dot);
            var = __builtin_fma(xi, dot, var);
            mu = __builtin_fma(beta_mean[i], xi, mu);
        }
        const double sigma = sqrt(fmax(var, 0.0));

        double total = 0.0, low = 0.0, high = 0.0;
        for (int attempt = 0; attempt < 2; ++attempt) {
            const bool filtered = attempt == 0;
            const double t_lo = mu - z * sigma, t_hi = mu + z * sigma;
            int n_lo = 0, n_hi = 0;                          // candidates of this lane (filtered pass)
            if (!filtered) {
                for (int k = 0; k < klo; ++k) lo[k * PM_THREADS + lane] = INFINITY;
                for (int k = 0; k < khi; ++k) hi[k * PM_THREADS + lane] = -INFINITY;
            }
            total = 0.0;
            for (int d0 = 0; d0 < dp; d0 += 16 * PM_DT) {
                // draw_product<PM_DT> written out (fokl_draw_tile.inc states the format, and why this kernel has a copy)
                d4 acc[PM_DT];
                const double *a_ptr[PM_DT];
#pragma unroll
                for (int t = 0; t < PM_DT; ++t) {
                    acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
                    a_ptr[t] = betas_t + (size_t)quad * dp + min(d0 + 16 * t, dp - 16) + col;   // past dp: re-read, skipped
                }
                double a_now[PM_DT], a_next[PM_DT];
#pragma unroll
                for (int t = 0; t < PM_DT; ++t) a_now[t] = a_ptr[t][0];
                for (int k0 = 0; k0 < ncp; k0 += 4) {
                    const double b = xs[(k0 + quad) * 16 + col];
                    const int kn = k0 + 4 < ncp ? k0 + 4 : k0;       // the next step's coefficients travel during this step's MFMAs
#pragma unroll
                    for (int t = 0; t < PM_DT; ++t) a_next[t] = a_ptr[t][(size_t)kn * dp];
#pragma unroll
                    for (int t = 0; t < PM_DT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_now[t], b, acc[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < PM_DT; ++t) a_now[t] = a_next[t];
                }
#pragma unroll
                for (int t = 0; t < PM_DT; ++t) {
                    if (d0 + 16 * t >= dp) continue;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        if (d0 + 16 * t + quad + 4 * v >= draws) continue;      // padding draws
                        const double val = acc[t][v];
                        total += val;
                        if (filtered) {
                            if (val < t_lo) {
                                if (n_lo < PM_CAP) lo[n_lo * PM_THREADS + lane] = val;
                                ++n_lo;
                            }
                            if (val > t_hi) {
                                if (n_hi < PM_CAP) hi[n_hi * PM_THREADS + lane] = val;
                                ++n_hi;
                            }
                            continue;
                        }
                        if (val < lo[(klo - 1) * PM_THREADS + lane]) {
                            int k = klo - 1;
                            while (k > 0 && lo[(k - 1) * PM_THREADS + lane] > val) {
                                lo[k * PM_THREADS + lane] = lo[(k - 1) * PM_THREADS + lane];
                                --k;
                            }
                            lo[k * PM_THREADS + lane] = val;
                        }
                        if (val > hi[(khi - 1) * PM_THREADS + lane]) {
                            int k = khi - 1;
                            while (k > 0 && hi[(k - 1) * PM_THREADS + lane] < val) {
                                hi[k * PM_THREADS + lane] = hi[(k - 1) * PM_THREADS + lane];
                                --k;
                            }
                            hi[k * PM_THREADS + lane] = val;
                        }
                    }
                }
            }
            __syncthreads();
            if (filtered) {
                // counts of the row's four quarters (wave shuffles: every lane takes part)
                int c_lo[4], c_hi[4], row_lo = 0, row_hi = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c_lo[q] = __shfl(n_lo, col + 16 * q, WAVE);
                    c_hi[q] = __shfl(n_hi, col + 16 * q, WAVE);
                    row_lo += c_lo[q];
                    row_hi += c_hi[q];
                }
                const bool bad = in && (n_lo > PM_CAP || n_hi > PM_CAP || row_lo < klo || row_hi < khi);
                if (__any(bad)) {                            // wave-uniform: the exact fallback for this tile
                    if (lane == 0) atomicAdd(&tally[1], 1ull);
                    continue;
                }
                // sort my few candidates in place (ascending below, descending above), pad to the list length
                for (int i = 1; i < n_lo; ++i) {
                    const double key = lo[i * PM_THREADS + lane];
                    int j = i - 1;
                    while (j >= 0 && lo[j * PM_THREADS + lane] > key) {
                        lo[(j + 1) * PM_THREADS + lane] = lo[j * PM_THREADS + lane];
                        --j;
                    }
                    lo[(j + 1) * PM_THREADS + lane] = key;
                }
                for (int i = n_lo; i < klo; ++i) lo[i * PM_THREADS + lane] = INFINITY;
                for (int i = 1; i < n_hi; ++i) {
                    const double key = hi[i * PM_THREADS + lane];
                    int j = i - 1;
                    while (j >= 0 && hi[j * PM_THREADS + lane] < key) {
                        hi[(j + 1) * PM_THREADS + lane] = hi[j * PM_THREADS + lane];
                        --j;
                    }
                    hi[(j + 1) * PM_THREADS + lane] = key;
                }
                for (int i = n_hi; i < khi; ++i) hi[i * PM_THREADS + lane] = -INFINITY;
                __syncthreads();
            }
            if (quad == 0) {
                // 4-way merge of the quarters' sorted lists (lanes col, col + 16, col + 32, col + 48)
                int p[4] = {0, 0, 0, 0};
                for (int t = 0; t < klo; ++t) {
                    int best = 0;
                    double bv = INFINITY;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double cand = p[q] < klo ? lo[p[q] * PM_THREADS + col + 16 * q] : INFINITY;
                        if (cand < bv) {
                            bv = cand;
                            best = q;
                        }
                    }
                    low = bv;
#pragma unroll
                    for (int q = 0; q < 4; ++q) p[q] += (q == best);
                }
                p[0] = p[1] = p[2] = p[3] = 0;
                for (int t = 0; t < khi; ++t) {
                    int best = 0;
                    double bv = -INFINITY;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double cand = p[q] < khi ? hi[p[q] * PM_THREADS + col + 16 * q] : -INFINITY;
                        if (cand > bv) {
                            bv = cand;
                            best = q;
                        }
                    }
                    high = bv;
#pragma unroll
                    for (int q = 0; q < 4; ++q) p[q] += (q == best);
                }
            }
            __syncthreads();
            if (filtered) break;
        }
        total += __shfl_xor(total, 16, WAVE);
        total += __shfl_xor(total, 32, WAVE);
        if (quad == 0 && in) {
            mean[r] = total / (double)draws;
            bounds[2 * r] = low;
            bounds[2 * r + 1] = high;
        }
        __syncthreads();
    }
    // the trips this wavefront's loop took, from where its tile index ended
    if (lane == 0) atomicAdd(&tally[0], (unsigned long long)((tile - blockIdx.x) / gridDim.x));
}

}  // namespace fokl

// What the last fokl_predict call on a context did (fokl_predict_report): which kernel, over what grid, and how many of
// the matrix-pipe kernel's tiles took the exact fallback.  A call refused before its launch leaves kernel 0.
static void predict_note(fokl_ctx *ctx, int kernel, bool wide, int64_t grid, int64_t tiles)
{
    ctx->predict_report[0] = kernel;
    ctx->predict_report[1] = wide ? 1 : 0;
    ctx->predict_report[2] = grid;
    ctx->predict_report[3] = tiles;
    ctx->predict_report[4] = ctx->predict_report[5] = 0;
}

extern "C" int fokl_predict_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_predict_report: null argument");
    std::memcpy(out, ctx->predict_report, sizeof ctx->predict_report);
    return FOKL_OK;
}

extern "C" int fokl_predict(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, int draws, int cut,
                            double *mean, double *bounds)
{
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_predict: null context");
    predict_note(ctx, FOKL_PREDICT_NONE, false, 0, 0);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, "fokl_predict: call fokl_upload first");
    if (nc <= 0 || draws <= 0 || !betas || !mean) return fail(ctx, FOKL_ERR_ARG, "fokl_predict: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_slots(ctx, slots, nc, "fokl_predict");
    if (rc) return rc;
    // bounds[i] = (sorted[cut], sorted[draws - cut]) -> the (cut + 1)-th smallest and the cut-th largest draw
    int klo = 1, khi = 1;
    if (bounds) {
        if (cut < 1 || cut >= draws) return fail(ctx, FOKL_ERR_ARG, "fokl_predict: need 1 <= cut < draws for bounds");
        klo = cut + 1;
        khi = cut;
    }
    const size_t n = (size_t)ctx->n;
    // Bounds over many draws: the matrix-pipe kernel (FOKL_PREDICT_PATH=valu keeps the VALU kernel, for A/B runs)
    const int ncp = (nc + 3) & ~3, dp = (draws + 15) & ~15;
    const size_t lds_mfma = ((size_t)ncp * 16 + 2 * (size_t)std::max(PM_CAP, std::max(klo, khi)) * PM_THREADS) * sizeof(double);
    const char *forced = std::getenv("FOKL_PREDICT_PATH");
    const bool use_mfma = bounds && draws >= 64 && lds_mfma <= 150 * 1024 && !(forced && std::strcmp(forced, "valu") == 0);
    // mean | bounds on the device; `repair`: the matrix-pipe kernel has filled them, and rows whose mean is not finite are
    // written again by the VALU kernel, which counts a row's NaN predictions (what ran is then still the former's report)
    double *d_res = nullptr;
    bool repair = false;
    int64_t mfma_report[4] = {0, 0, 0, 0};
    if (use_mfma) {
        const size_t beta_off = ((size_t)nc * sizeof(int) + 7) & ~(size_t)7;
        // argument block: slots | betas' | their mean | their covariance | the kernel's two tile counts and predict_flag_kernel's
        // flag (zero on arrival)
        const size_t arg_doubles = (size_t)ncp * dp + ncp + (size_t)ncp * ncp;
        const size_t tally_off = beta_off + arg_doubles * sizeof(double);
        const size_t arg_bytes = tally_off + 3 * sizeof(unsigned long long);
        rc = begin_args(ctx, arg_bytes);
        if (rc) return rc;
        std::memcpy(ctx->h_args, slots, (size_t)nc * sizeof(int));
        double *bt = reinterpret_cast<double *>(ctx->h_args + beta_off);
        std::memset(bt, 0, arg_bytes - beta_off);
        fill_draw_table(bt, betas, draws, nc, ncp, dp);
        // mean and (population) covariance of the draws: the filter's model of a row's predictions
        double *bm = bt + (size_t)ncp * dp, *bc = bm + ncp;
        for (int k = 0; k < nc; ++k) {
            double sum = 0.0;
            for (int d = 0; d < draws; ++d) sum += bt[(size_t)k * dp + d];
            bm[k] = sum / draws;
        }
        for (int i = 0; i < nc; ++i)
            for (int j = i; j < nc; ++j) {
                double sum = 0.0;
                const double *ri = bt + (size_t)i * dp, *rj = bt + (size_t)j * dp;
                for (int d = 0; d < draws; ++d) sum += (ri[d] - bm[i]) * (rj[d] - bm[j]);
                bc[(size_t)i * ncp + j] = bc[(size_t)j * ncp + i] = sum / draws;
            }
        // z with a normal tail of about 2 klo / draws beyond it (twice what the lists need), by bisection on erfc
        const double tail = std::min(0.45, (2.0 * klo + 8.0) / draws);
        double z_lo = 0.0, z_hi = 8.0;
        for (int it = 0; it < 60; ++it) {
            const double mid = 0.5 * (z_lo + z_hi);
            (0.5 * std::erfc(mid / std::sqrt(2.0)) > tail ? z_lo : z_hi) = mid;
        }
        const double z = 0.5 * (z_lo + z_hi);
        rc = push_args(ctx, arg_bytes);
        if (rc) return rc;
        HIP_TRY(ctx, hipMalloc((void **)&d_res, n * 3 * sizeof(double)));
        unsigned long long *d_tally = reinterpret_cast<unsigned long long *>(ctx->d_args + tally_off);
        const int64_t tiles = ((int64_t)n + 15) / 16;
        const int grid = (int)std::min<int64_t>(tiles, (int64_t)cu_count(ctx) * 16);
        hipError_t le = lds_opt_in(predict_mfma_kernel, lds_mfma, 152 * 1024);
        if (le != hipSuccess) {
            (void)hipFree(d_res);
            return fail(ctx, FOKL_ERR_HIP, std::string("fokl_predict: ") + hipGetErrorString(le));
        }
        {
            TimedRegion timed(ctx, FOKL_K_PREDICT, 8.0 * (double)n * (nc + 3), 2.0 * (double)n * nc * draws);
            hipLaunchKernelGGL(predict_mfma_kernel, dim3(grid), dim3(PM_THREADS), lds_mfma, ctx->stream,
                               ctx->d_slot_ptr, reinterpret_cast<const int *>(ctx->d_args), nc, ncp,
                               reinterpret_cast<const double *>(ctx->d_args + beta_off), draws, dp,
                               reinterpret_cast<const double *>(ctx->d_args + beta_off) + (size_t)ncp * dp,
                               reinterpret_cast<const double *>(ctx->d_args + beta_off) + (size_t)ncp * dp + ncp, z,
                               klo, khi, ctx->n, d_res, d_res + n, d_tally);
            le = hipGetLastError();
            if (le != hipSuccess) {
                (void)hipFree(d_res);
                return fail(ctx, FOKL_ERR_HIP, std::string("predict_mfma_kernel launch: ") + hipGetErrorString(le));
            }
            const int flag_grid = (int)std::min<int64_t>(((int64_t)n + 255) / 256, (int64_t)cu_count(ctx) * 8);
            hipLaunchKernelGGL(predict_flag_kernel, dim3(flag_grid), dim3(256), 0, ctx->stream, d_res, ctx->n, d_tally + 2);
            le = hipGetLastError();
            if (le != hipSuccess) {
                (void)hipFree(d_res);
                return fail(ctx, FOKL_ERR_HIP, std::string("predict_flag_kernel launch: ") + hipGetErrorString(le));
            }
        }
        unsigned long long tally[3] = {0, 0, 0};
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(tally, d_tally, sizeof tally, hipMemcpyDeviceToHost);
        repair = e == hipSuccess && tally[2] != 0;
        if (!repair) {
            if (e == hipSuccess) e = hipMemcpy(mean, d_res, n * sizeof(double), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(bounds, d_res + n, n * 2 * sizeof(double), hipMemcpyDeviceToHost);
            (void)hipFree(d_res);
            if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_predict: ") + hipGetErrorString(e));
        }
        mfma_report[0] = grid;
        mfma_report[1] = tiles;
        mfma_report[2] = (int64_t)tally[0];
        mfma_report[3] = (int64_t)tally[1];
        if (!repair) {
            predict_note(ctx, FOKL_PREDICT_MFMA, false, mfma_report[0], mfma_report[1]);
            ctx->predict_report[4] = mfma_report[2];
            ctx->predict_report[5] = mfma_report[3];
            return FOKL_OK;
        }
    }

    // the sorted lists of the order statistics move to device memory when they do not fit LDS next to the basis values
    // (bounds over more than ~5 000 draws: klo > PR_MAX_K) -- the reference sorts any number of draws per row (FR:971-977)
    bool global_lists = bounds && (klo > PR_MAX_K || (size_t)(nc + klo + khi) * PR_THREADS * sizeof(double) > 150 * 1024);
    size_t lds_bytes = (size_t)(nc + (global_lists ? 0 : klo + khi)) * PR_THREADS * sizeof(double);
    // ... and a model whose basis values alone do not fit (about 300 terms) leaves them in the columns: LDS then holds the
    // lists only, which fit whenever klo <= PR_MAX_K -- the reference evaluates a model of any width (FR:966-978)
    const bool wide = lds_bytes > 150 * 1024;
    if (wide) {
        global_lists = bounds && klo > PR_MAX_K;
        lds_bytes = bounds && !global_lists ? (size_t)(klo + khi) * PR_THREADS * sizeof(double) : 0;
    }

    // argument block: slots | betas ; outputs: mean | bounds in a dedicated allocation
    const size_t beta_off = ((size_t)nc * sizeof(int) + 7) & ~(size_t)7;
    const size_t arg_bytes = beta_off + (size_t)draws * nc * sizeof(double);
    rc = begin_args(ctx, arg_bytes);
    if (rc) return rc;
    std::memcpy(ctx->h_args, slots, (size_t)nc * sizeof(int));
    std::memcpy(ctx->h_args + beta_off, betas, (size_t)draws * nc * sizeof(double));
    rc = push_args(ctx, arg_bytes);
    if (rc) return rc;

    if (!repair) HIP_TRY(ctx, hipMalloc((void **)&d_res, n * 3 * sizeof(double)));
    double *d_mean = d_res, *d_bounds = bounds ? d_res + n : nullptr;
    const int64_t row_blocks = ((int64_t)n + PR_THREADS - 1) / PR_THREADS;
    // wavefronts per CU: what LDS admits once the basis values are not in it, enough of them to hide the columns' latency
    const int per_cu = global_lists ? 4 : !wide ? 8 : (int)std::min<size_t>(32, 160 * 1024 / std::max<size_t>(lds_bytes, 1));
    const int grid = (int)std::min<int64_t>(row_blocks, (int64_t)cu_count(ctx) * per_cu);
    double *d_lists = nullptr;
    if (global_lists) {
        hipError_t ea = hipMalloc((void **)&d_lists, (size_t)grid * (klo + khi) * PR_THREADS * sizeof(double));
        if (ea != hipSuccess) {
            (void)hipFree(d_res);
            return fail(ctx, FOKL_ERR_HIP, std::string("fokl_predict: order-statistic lists: ") + hipGetErrorString(ea));
        }
    }
    {
        auto fn = wide ? (global_lists ? predict_kernel<true, true> : predict_kernel<false, true>)
                       : (global_lists ? predict_kernel<true, false> : predict_kernel<false, false>);
        hipError_t e = lds_opt_in(fn, lds_bytes, 152 * 1024);
        if (e == hipSuccess) {
            TimedRegion timed(ctx, FOKL_K_PREDICT, 8.0 * (double)n * (nc + 3), 2.0 * (double)n * nc * draws);
            hipLaunchKernelGGL(fn, dim3(grid), dim3(PR_THREADS), lds_bytes, ctx->stream, ctx->d_slot_ptr,
                               reinterpret_cast<const int *>(ctx->d_args), nc,
                               reinterpret_cast<const double *>(ctx->d_args + beta_off), draws, klo, khi, ctx->n, d_mean,
                               d_bounds, d_lists, repair ? 1 : 0);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            (void)hipFree(d_res);
            if (d_lists) (void)hipFree(d_lists);
            return fail(ctx, FOKL_ERR_HIP, std::string("predict_kernel launch: ") + hipGetErrorString(e));
        }
    }
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (d_lists) (void)hipFree(d_lists);
    if (e == hipSuccess) e = hipMemcpy(mean, d_mean, n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && bounds) e = hipMemcpy(bounds, d_bounds, n * 2 * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d_res);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_predict: ") + hipGetErrorString(e));
    if (repair) {
        predict_note(ctx, FOKL_PREDICT_MFMA, false, mfma_report[0], mfma_report[1]);
        ctx->predict_report[4] = mfma_report[2];
        ctx->predict_report[5] = mfma_report[3];
        return FOKL_OK;
    }
    predict_note(ctx, global_lists ? FOKL_PREDICT_VALU_GLOBAL : FOKL_PREDICT_VALU_LDS, wide, grid, row_blocks);
    return FOKL_OK;
}

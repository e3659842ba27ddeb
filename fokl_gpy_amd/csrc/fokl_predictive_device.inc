// predictive(): the posterior predictive distribution of every row over all posterior draws -- PIT, quantiles, brackets
// (textually included by fokl_hip.hip).  The statement is fokl_gpy_amd/predictive.py: predictive_rows_host.
//
// The predictive of a row is the equal-weight mixture over the draws of N(mu_d, sd_d^2), mu_d = X_row . beta_d.  The product
// is the draw tile's (fokl_draw_tile.inc: the coefficient table and the lane map): one wavefront per tile of 16 rows, the
// tile's basis values in LDS [ncp][16], blocks of PD_DT x 16 draws.  mu is never stored: the PASS LOOP goes around the
// product, which is recomputed in every pass, so that there is no limit on the draws and LDS holds the columns only.
//   pass 0      s1 = sum(mu - mu0), s2 = sum((mu - mu0)^2), min and max of mu, per quantile j the exact bracket lo_j =
//               min(mu + sd z_j), hi_j = max(mu + sd z_j) and, with data, pit = sum 0.5 erfc((mu - y) rinv) / E
//   first trial q_j = mean + z_j sqrt(var) where strictly inside (lo_j, hi_j), else the midpoint
//   pass k >= 1 for every (row, quantile) not done: F = sum 0.5 erfc(-t) / E and f = sum exp(-t^2) rinv / (E sqrt(pi)), t =
//               (q - mu) rinv; r = F - p; the bracket takes q; done on |r| <= ftol or on the width; else a Newton step where
//               it is safe (f > 0, strictly inside the bracket, |r| at most half the residual before a Newton step), else
//               the midpoint
// Each of the four lanes that share a row keeps the partial sums over its quarter of the draws; at the end of a pass they
// merge in the order of the quarters, q = 0 .. 3, and the bracket update and the proposal are computed redundantly in the
// four lanes.  Nothing is accumulated with atomics: the same arguments give the same bits.  Rows past n compute on zeros,
// count as done and store nothing; padding draws (to a multiple of 16) are skipped.  The test that ends a tile's passes is
// wave-uniform (__any), every loop has a fixed bound.

namespace fokl {

constexpr int PD_THREADS = 64;
constexpr int PD_DT = 4;                         // 16-draw tiles per block: independent MFMA chains
constexpr int PD_QMAX = FOKL_PREDICTIVE_MAX_QUANTILES;

struct PdArgs {
    double p[PD_QMAX], z[PD_QMAX];
    double ftol, xtol, mean_sigsqd, sd_max, e_sqrt_pi;
    int Q, max_passes;
};

// acc[i >> 2][i & 3] for a wave-uniform i: a chain of selects, so that the loop over a lane's sixteen draws can stay rolled
// without the accumulators leaving their registers
__device__ __forceinline__ double pd_pick(const d4 (&acc)[PD_DT], int i)
{
    double m = acc[0][0];
#pragma unroll
    for (int t = 0; t < PD_DT; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) m = (i == 4 * t + v) ? acc[t][v] : m;
    return m;
}

// QM: the quantiles the instance keeps in registers (0: PIT only); args.Q <= QM of them are live
template <int QM>
__global__ __launch_bounds__(PD_THREADS) void predictive_kernel(double *const *__restrict__ slot_ptr,
                                                                const int *__restrict__ slots, int nc, int ncp,
                                                                const double *__restrict__ betas_t,
                                                                const double *__restrict__ scal, int draws, int dp,
                                                                const double *__restrict__ data, int64_t n, const PdArgs args,
                                                                double *__restrict__ out, int *__restrict__ tile_passes)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [ncp][16]
    constexpr int QA = QM > 0 ? QM : 1;
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int Q = args.Q < QM ? args.Q : QM;
    const int64_t n_tiles = (n + 15) / 16;
    const double E = (double)draws;
    const unsigned all_done = (1u << QM) - 1u;
    const int stride = 6 + 5 * args.Q;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * 16 + col;
        const bool in = r < n;
        draw_tile_load(xs, slot_ptr, slots, nc, ncp, r, in, quad, col);
        const double yv = (in && data) ? data[r] : 0.0;
        __syncthreads();                                 // one wavefront per workgroup: orders the LDS traffic

        // ---- pass 0
        double s1 = 0.0, s2 = 0.0, mn = INFINITY, mx = -INFINITY, ps = 0.0, mu0 = 0.0;
        double lo[QA], hi[QA], q[QA], res[QA], rprev[QA];
        int used[QA];
#pragma unroll
        for (int j = 0; j < QA; ++j) {
            lo[j] = INFINITY;
            hi[j] = -INFINITY;
        }
        for (int d0 = 0; d0 < dp; d0 += 16 * PD_DT) {
            d4 acc[PD_DT];
            draw_product<PD_DT>(xs, betas_t, ncp, dp, d0, quad, col, acc);
            if (d0 == 0) mu0 = __shfl(acc[0][0], col, WAVE);         // draw 0 of row col: quarter 0, v = 0
#pragma unroll 1
            for (int i = 0; i < 4 * PD_DT; ++i) {                    // rolled: one copy of erfc in the code, not sixteen
                const int d = d0 + 16 * (i >> 2) + quad + 4 * (i & 3);
                if (d >= draws) continue;                            // padding draws (and blocks past dp)
                const double m = pd_pick(acc, i), sdv = scal[d];
                const double dd = m - mu0;
                s1 += dd;
                s2 += dd * dd;
                mn = fmin(mn, m);
                mx = fmax(mx, m);
                if (data) ps += 0.5 * erfc((m - yv) * scal[dp + d]);
#pragma unroll
                for (int j = 0; j < QM; ++j) {
                    if (j >= Q) break;
                    const double c = m + sdv * args.z[j];
                    lo[j] = fmin(lo[j], c);
                    hi[j] = fmax(hi[j], c);
                }
            }
        }
        // the row's four quarters, in their order
        double S1 = 0.0, S2 = 0.0, MN = INFINITY, MX = -INFINITY, PS = 0.0;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            S1 += __shfl(s1, col + 16 * qd, WAVE);
            S2 += __shfl(s2, col + 16 * qd, WAVE);
            MN = fmin(MN, __shfl(mn, col + 16 * qd, WAVE));
            MX = fmax(MX, __shfl(mx, col + 16 * qd, WAVE));
            PS += __shfl(ps, col + 16 * qd, WAVE);
        }
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            double a = INFINITY, b = -INFINITY;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                a = fmin(a, __shfl(lo[j], col + 16 * qd, WAVE));
                b = fmax(b, __shfl(hi[j], col + 16 * qd, WAVE));
            }
            lo[j] = a;
            hi[j] = b;
        }
        const double mean = mu0 + S1 / E;
        const double var = fmax((S2 - S1 * S1 / E) / E, 0.0) + args.mean_sigsqd;
        const double sdp = sqrt(var), width = MX - MN + args.sd_max;
        unsigned done = in ? 0u : all_done;
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            if (j >= Q) done |= 1u << j;
            const double trial = mean + args.z[j < Q ? j : 0] * sdp;
            q[j] = (trial > lo[j] && trial < hi[j]) ? trial : 0.5 * (lo[j] + hi[j]);
            res[j] = INFINITY;
            rprev[j] = INFINITY;
            used[j] = 0;
        }

        // ---- passes 1 .. max_passes
        int ran = 0;
        if (QM > 0) {
            for (int k = 1; k <= args.max_passes; ++k) {
                if (!__any(done != all_done)) break;                 // wave uniform: every row of the tile is done
                ++ran;
                double Fs[QA], fs[QA];
#pragma unroll
                for (int j = 0; j < QA; ++j) {
                    Fs[j] = 0.0;
                    fs[j] = 0.0;
                }
                for (int d0 = 0; d0 < dp; d0 += 16 * PD_DT) {
                    d4 acc[PD_DT];
                    draw_product<PD_DT>(xs, betas_t, ncp, dp, d0, quad, col, acc);
#pragma unroll 1
                    for (int i = 0; i < 4 * PD_DT; ++i) {            // rolled: QM copies of erfc and exp, not 16 QM
                        const int d = d0 + 16 * (i >> 2) + quad + 4 * (i & 3);
                        if (d >= draws) continue;                    // padding draws (and blocks past dp)
                        const double m = pd_pick(acc, i), rv = scal[dp + d];
#pragma unroll
                        for (int j = 0; j < QM; ++j) {
                            if ((done >> j) & 1u) continue;
                            const double tt = (q[j] - m) * rv;
                            Fs[j] += 0.5 * erfc(-tt);
                            fs[j] += exp(-(tt * tt)) * rv;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < QM; ++j) {
                    double F = 0.0, f = 0.0;
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) {                 // every lane takes part in the shuffles
                        F += __shfl(Fs[j], col + 16 * qd, WAVE);
                        f += __shfl(fs[j], col + 16 * qd, WAVE);
                    }
                    if ((done >> j) & 1u) continue;
                    F = F / E;
                    f = f / args.e_sqrt_pi;
                    const double rr = F - args.p[j];
                    res[j] = rr;
                    used[j] = k;
                    if (rr < 0.0) lo[j] = q[j];
                    else hi[j] = q[j];
                    if (fabs(rr) <= args.ftol || hi[j] - lo[j] <= args.xtol * width) {
                        done |= 1u << j;
                        continue;
                    }
                    const double newton = q[j] - rr / f;
                    const bool take = f > 0.0 && newton > lo[j] && newton < hi[j] && fabs(rr) <= rprev[j] / 2.0;
                    rprev[j] = take ? fabs(rr) : INFINITY;
                    if (k < args.max_passes) q[j] = take ? newton : 0.5 * (lo[j] + hi[j]);   // q stays the last point evaluated
                }
            }
        }
        if (lane == 0) tile_passes[tile] = ran;
        if (quad == 0 && in) {
            double *o = out + (size_t)r * stride;
            o[0] = mu0;
            o[1] = S1;
            o[2] = S2;
            o[3] = MN;
            o[4] = MX;
            o[5] = data ? PS / E : 0.0;
#pragma unroll
            for (int j = 0; j < QM; ++j) {
                if (j >= Q) break;
                o[6 + 5 * j] = q[j];
                o[7 + 5 * j] = res[j];
                o[8 + 5 * j] = lo[j];
                o[9 + 5 * j] = hi[j];
                o[10 + 5 * j] = (double)used[j];
            }
        }
        __syncthreads();                                 // the tile's LDS has been read: the next one may be stored
    }
}

}  // namespace fokl

extern "C" int fokl_predictive_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_predictive_report: null argument");
    std::memcpy(out, ctx->predictive_report, sizeof ctx->predictive_report);
    return FOKL_OK;
}

extern "C" int fokl_predictive_rows(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sd,
                                    const double *rinv, int draws, double mean_sigsqd, int with_data, const double *p,
                                    const double *z, int nq, int max_passes, double ftol, double xtol, double *out)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_predictive_rows: null context");
    std::memset(ctx->predictive_report, 0, sizeof ctx->predictive_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, "fokl_predictive_rows: call fokl_upload first");
    if (nc <= 0 || draws <= 0 || !betas || !sd || !rinv || !out || (nq > 0 && (!p || !z)))
        return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: bad argument");
    if (draws > (1 << 22) || nc > (1 << 20)) return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: too many draws or columns");
    if (nq < 0 || nq > FOKL_PREDICTIVE_MAX_QUANTILES)
        return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: " + std::to_string(nq) + " quantiles, one call takes at most "
                    "FOKL_PREDICTIVE_MAX_QUANTILES = " + std::to_string(FOKL_PREDICTIVE_MAX_QUANTILES));
    if (!with_data && nq == 0)
        return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: neither data nor quantiles, nothing would be computed");
    if (max_passes < 0) return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: max_passes must be >= 0");
    if (!std::isfinite(ftol) || ftol < 0.0 || !std::isfinite(xtol) || xtol < 0.0)
        return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: ftol and xtol must be finite and >= 0");
    if (!std::isfinite(mean_sigsqd) || !(mean_sigsqd > 0.0))
        return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: the mean of sigsqd must be positive and finite");
    double sd_max = 0.0;
    for (int d = 0; d < draws; ++d) {
        if (!(sd[d] > 0.0) || !std::isfinite(sd[d]) || !(rinv[d] > 0.0) || !std::isfinite(rinv[d]))
            return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: every sd and rinv must be positive and finite");
        sd_max = std::max(sd_max, sd[d]);
    }
    for (int j = 0; j < nq; ++j) {
        if (!std::isfinite(p[j]) || !(p[j] > 0.0) || !(p[j] < 1.0) || !std::isfinite(z[j]))
            return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: every quantile must lie strictly inside (0, 1), with a finite z");
        for (int k = 0; k < j; ++k)
            if (p[k] == p[j]) return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: the quantiles repeat a value");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_slots(ctx, slots, nc, "fokl_predictive_rows");
    if (rc) return rc;
    const int64_t n = ctx->n;
    if (n <= 0) return fail(ctx, FOKL_ERR_STATE, "fokl_predictive_rows: the dataset has no rows");

    const int ncp = (nc + 3) & ~3, dp = (draws + 15) & ~15, stride = 6 + 5 * nq;
    const size_t lds_bytes = ((size_t)ncp * 16 + 16) * sizeof(double);
    if (lds_bytes > 160 * 1024)
        return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: " + std::to_string(nc) + " columns want " + std::to_string(lds_bytes) +
                    " bytes of LDS per 16-row tile, a compute unit has 163840");
    const int64_t tiles = (n + 15) / 16;
    const size_t table_bytes = ((size_t)ncp + 2) * dp * sizeof(double);
    const size_t out_bytes = (size_t)n * stride * sizeof(double);
    const size_t count_bytes = (size_t)tiles * sizeof(int);
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_PREDICTIVE_FREE_BYTES", &free_bytes));
    if (table_bytes + out_bytes + count_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, "fokl_predictive_rows: the call wants " + std::to_string(table_bytes + out_bytes + count_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(table_bytes) +
                    " bytes of coefficients = (columns + 2) x draws x 8, " + std::to_string(out_bytes) + " of results = rows x (6 + 5 Q) x 8, " +
                    std::to_string(count_bytes) + " of pass counts), the device has " + std::to_string(free_bytes) + " free" +
                    (table_bytes > out_bytes ? " (thin the draws)" : " (take the rows in parts)"));

    // coefficients transposed and zero padded [ncp][dp] | sd [dp] | rinv [dp] (padding draws: zeros, never used)
    std::vector<double> table(((size_t)ncp + 2) * dp, 0.0);
    fill_draw_table(table.data(), betas, draws, nc, ncp, dp);
    double *scal = table.data() + (size_t)ncp * dp;
    for (int d = 0; d < draws; ++d) {
        scal[d] = sd[d];
        scal[dp + d] = rinv[d];
    }
    PdArgs args = {};
    for (int j = 0; j < nq; ++j) {
        args.p[j] = p[j];
        args.z[j] = z[j];
    }
    args.ftol = ftol;
    args.xtol = xtol;
    args.mean_sigsqd = mean_sigsqd;
    args.sd_max = sd_max;
    args.e_sqrt_pi = (double)draws * std::sqrt(M_PI);
    args.Q = nq;
    args.max_passes = max_passes;

    DeviceBuffers buf;
    double *d_table = nullptr, *d_out = nullptr;
    int *d_slots = nullptr, *d_count = nullptr;
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc));
    HIP_TRY(ctx, buf.get(&d_out, (size_t)n * stride));
    HIP_TRY(ctx, buf.get(&d_count, (size_t)tiles));

    // the instance: 0, 4 or 8 quantiles in registers (2, 1 and 1 wavefronts per SIMD as compiled).  The grid asks for more
    // workgroups per CU than are resident: the rest queue behind them, which evens out tiles of different pass counts
    auto fn = nq == 0 ? predictive_kernel<0> : nq <= 4 ? predictive_kernel<4> : predictive_kernel<8>;
    const int waves = nq == 0 ? 16 : nq <= 4 ? 12 : 8;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(waves, 160 * 1024 / lds_bytes));
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)cu_count(ctx) * per_cu);
    hipError_t e = lds_opt_in(fn, lds_bytes, 160 * 1024);
    StreamStopwatch watch(ctx, e);
    const int t0 = watch.mark();
    if (e == hipSuccess) {
        TimedRegion timed(ctx, FOKL_K_PREDICTIVE, 0.0, 0.0);             // bytes and flops: below, of the passes that ran
        hipLaunchKernelGGL(fn, dim3(grid), dim3(PD_THREADS), lds_bytes, ctx->stream, ctx->d_slot_ptr, d_slots, nc, ncp, d_table,
                           d_table + (size_t)ncp * dp, draws, dp, with_data ? ctx->slot_ptr[FOKL_SLOT_Y] : (double *)nullptr, n,
                           args, d_out, d_count);
        e = hipGetLastError();
    }
    const int t1 = watch.mark();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    const double kernel_us = watch.us(t0, t1);
    std::vector<int> count((size_t)tiles, 0);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(count.data(), d_count, count_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_predictive_rows: ") + hipGetErrorString(e));

    int64_t most = 0, sum = 0, unresolved = 0;
    for (int64_t t = 0; t < tiles; ++t) {
        most = std::max<int64_t>(most, count[(size_t)t]);
        sum += count[(size_t)t];
    }
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < nq; ++j) unresolved += std::fabs(out[(size_t)i * stride + 7 + 5 * j]) <= ftol ? 0 : 1;
    if (ctx->timing) {
        const double bytes = 8.0 * (double)n * (nc + 1 + stride);
        const double flops = 2.0 * 16.0 * (double)ncp * (double)draws * (double)(tiles + sum);   // pass 0 and the passes run
        ctx->tslot[FOKL_K_PREDICTIVE].bytes += bytes;
        ctx->tslot[FOKL_K_PREDICTIVE].flops += flops;
        ctx->tslot[FOKL_K_PREDICTIVE].ideal_ms += 1e3 * std::max(bytes / FOKL_PEAK_HBM_BYTES_PER_S, flops / FOKL_PEAK_F64_FLOPS);
    }
    int64_t *rep = ctx->predictive_report;
    rep[0] = (with_data ? FOKL_PREDICTIVE_PIT : 0) | (nq > 0 ? FOKL_PREDICTIVE_QUANTILES : 0);
    rep[1] = grid;
    rep[2] = tiles;
    rep[3] = (int64_t)lds_bytes;
    rep[4] = nq;
    rep[5] = most;
    rep[6] = sum;
    rep[7] = unresolved;
    rep[8] = (int64_t)std::llround(kernel_us);
    return FOKL_OK;
}

// score(): the pointwise log predictive density of every row over all posterior draws -- WAIC and PSIS-LOO (textually
// included by fokl_hip.hip).  The statement is fokl_gpy_amd/score.py: score_rows_host.
//
// ll[row][d] = c_d - (y_row - X_row . beta_d)^2 h_d with c_d = -log(2 pi sigsqd_d) / 2 and h_d = 0.5 / sigsqd_d (formed on
// the host).  The product is the draw tile's (fokl_draw_tile.inc: the coefficient table and the lane map): one wavefront per
// tile of 16 rows, the tile's basis values in LDS [column][row], blocks of SC_DT x 16 draws.  ll is never stored.  Per row
// the four lanes that share it keep, each over its quarter of the draws,
//   * an online max and sum of exp(ll - max)                          -> lppd
//   * sum(ll - ll0) and sum((ll - ll0)^2), ll0 = ll[row][0]           -> ll_mean, p_waic
// and, for PSIS, together
//   * the M + 1 largest log ratios r = -ll, unsorted in LDS [M + 1][16], with the smallest of them and its place (the
//     threshold test in front of the list) in registers, the same in all four lanes.  A value above the threshold replaces
//     the smallest and the four lanes look for the new smallest together ((M + 1) / 4 LDS reads each and two shuffles);
//     the quarters insert in turn, q = 0 .. 3, so that the list has one writer at a time.
//   * an online max and sum of exp(r - max) over every value that did NOT stay in the list (rejected or evicted): the
//     body's raw weights are summed directly, never as "all minus tail".
// At the end of the draws the list is sorted in place (odd-even transposition, M + 1 phases), shifted by its largest
// entry, written to tail_out if wanted, and the generalised Pareto fit (Zhang-Stephens, 30 + sqrt(M') grid points dealt to
// the four lanes of the row) runs over it in the same launch.  Since w_d and ll_d are tied through r, the body's terms of
// sum exp(w_d + ll_d) are all exp(-max r): elpd_loo = -max r + log(n_body + sum_tail W_j / exp(s_j)) - log(sum_body exp(s_d)
// + sum_tail W_j), W_j the smoothed weights.
//
// Every merge across lanes runs in the order of the quarters, nothing is accumulated with atomics: the same arguments give
// the same bits.  Rows past n compute on zeros and store nothing; padding draws (to a multiple of 16) are skipped.
//
// NOISE selects the likelihood (fokl_score_rows_noise; the statement is score.log_likelihood with nu and sw); only ll differs:
//   SC_GAUSSIAN           the text above, and the code it compiled to before there was a choice
//   SC_GAUSSIAN_WEIGHTED  ll = (c_d + lw) - (sw e)^2 h_d: sw = sqrt(w_row) is read once per row next to y, lw = log(sw) there
//   SC_STUDENT            ll = (c_d + lw) - hp log1p((sw e)^2 g_d), hp = (nu + 1) / 2, with the t constant c_d and g_d = 1 / (nu
//                         sigsqd_d) in the two rows of cons (sw = 1, lw = 0 without weights)

namespace fokl {

constexpr int SC_THREADS = 64;
constexpr int SC_DT = 4;                         // 16-draw tiles per block: independent MFMA chains
constexpr int SC_GRID_MAX = 64;                  // rows of the Pareto fit's profile likelihood in LDS: 30 + sqrt(511) = 52 used
constexpr double SC_LOG_DBL_MIN = -708.3964185322641;   // log(DBL_MIN)

// (m, s) <- (m, s) + x: s = sum exp(. - m).  m = -inf to start with: d = +inf, e = 0.
__device__ inline void sc_lse_add(double &m, double &s, double x)
{
    const double d = x - m, e = exp(-fabs(d));
    if (d > 0.0) {
        s = s * e + 1.0;
        m = x;
    } else {
        s += e;
    }
}

__device__ inline void sc_lse_merge(double &m, double &s, double m2, double s2)
{
    if (!(s2 > 0.0)) return;
    if (!(s > 0.0)) {
        m = m2;
        s = s2;
        return;
    }
    const double nm = fmax(m, m2);
    s = s * exp(m - nm) + s2 * exp(m2 - nm);
    m = nm;
}

enum { SC_GAUSSIAN = FOKL_NOISE_GAUSSIAN, SC_GAUSSIAN_WEIGHTED = FOKL_NOISE_GAUSSIAN_WEIGHTED, SC_STUDENT = FOKL_NOISE_STUDENT };

// what an instance needs beyond the Gaussian one's arguments: the last kernel argument, empty for SC_GAUSSIAN
template <int NOISE> struct ScNoise {};
template <> struct ScNoise<SC_GAUSSIAN_WEIGHTED> {
    const double *sw;                            // [n] or null (ones)
};
template <> struct ScNoise<SC_STUDENT> {
    const double *sw;                            // [n] or null (ones)
    double hp;                                   // (nu + 1) / 2
};

template <bool LOO, int NOISE>
__global__ __launch_bounds__(SC_THREADS) void score_kernel(double *const *__restrict__ slot_ptr,
                                                           const int *__restrict__ slots, int nc, int ncp,
                                                           const double *__restrict__ betas_t,
                                                           const double *__restrict__ cons, int draws, int dp,
                                                           const double *__restrict__ data, int64_t n, int M,
                                                           double *__restrict__ stats, double *__restrict__ tail_out,
                                                           const ScNoise<NOISE> nz)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *xs = lds;                                // [ncp][16]
    double *list = xs + (size_t)ncp * 16;            // [M + 1][16]
    double *prof = list + (size_t)(M + 1) * 16;      // [SC_GRID_MAX][16]
    const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
    const int cnt = M + 1;
    const int64_t n_tiles = (n + 15) / 16;
    const double E = (double)draws;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * 16 + col;
        const bool in = r < n;
        draw_tile_load(xs, slot_ptr, slots, nc, ncp, r, in, quad, col);
        if (LOO)
            for (int k = quad; k < cnt; k += 4) list[k * 16 + col] = -INFINITY;
        const double yv = in ? data[r] : 0.0;
        [[maybe_unused]] double swv = 1.0, lwv = 0.0;
        if constexpr (NOISE != SC_GAUSSIAN) {
            swv = (in && nz.sw) ? nz.sw[r] : 1.0;
            lwv = log(swv);
        }
        __syncthreads();                                 // one wavefront per workgroup: orders the LDS traffic

        double lm = -INFINITY, ls = 0.0, s1 = 0.0, s2 = 0.0, ll0 = 0.0;
        double bm = -INFINITY, bs = 0.0, thr = -INFINITY;
        int pos = 0;

        for (int d0 = 0; d0 < dp; d0 += 16 * SC_DT) {
            // draw_product<SC_DT> written out (fokl_draw_tile.inc states the format, and why this kernel has a copy)
            d4 acc[SC_DT];
            const double *a_ptr[SC_DT];
#pragma unroll
            for (int t = 0; t < SC_DT; ++t) {
                acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
                a_ptr[t] = betas_t + (size_t)quad * dp + min(d0 + 16 * t, dp - 16) + col;   // past dp: re-read, skipped
            }
            double a_now[SC_DT], a_next[SC_DT];
#pragma unroll
            for (int t = 0; t < SC_DT; ++t) a_now[t] = a_ptr[t][0];
            for (int k0 = 0; k0 < ncp; k0 += 4) {
                const double b = xs[(k0 + quad) * 16 + col];
                const int kn = k0 + 4 < ncp ? k0 + 4 : k0;           // the next step's coefficients travel during this step's MFMAs
#pragma unroll
                for (int t = 0; t < SC_DT; ++t) a_next[t] = a_ptr[t][(size_t)kn * dp];
#pragma unroll
                for (int t = 0; t < SC_DT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_now[t], b, acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < SC_DT; ++t) a_now[t] = a_next[t];
            }
            double llv[SC_DT][4];
#pragma unroll
            for (int t = 0; t < SC_DT; ++t)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int d = min(d0 + 16 * t + quad + 4 * v, dp - 1);
                    if constexpr (NOISE == SC_GAUSSIAN) {
                        const double e = yv - acc[t][v];
                        llv[t][v] = cons[d] - (e * e) * cons[dp + d];
                    } else {
                        const double e = swv * (yv - acc[t][v]);
                        if constexpr (NOISE == SC_STUDENT) llv[t][v] = (cons[d] + lwv) - nz.hp * log1p((e * e) * cons[dp + d]);
                        else llv[t][v] = (cons[d] + lwv) - (e * e) * cons[dp + d];
                    }
                }
            if (d0 == 0) ll0 = __shfl(llv[0][0], col, WAVE);         // draw 0 of row col: quarter 0, v = 0
#pragma unroll
            for (int t = 0; t < SC_DT; ++t) {
                if (d0 + 16 * t >= dp) continue;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const bool valid = d0 + 16 * t + quad + 4 * v < draws;   // padding draws
                    const double ll = llv[t][v];
                    if (valid) {
                        sc_lse_add(lm, ls, ll);
                        const double dd = ll - ll0;
                        s1 += dd;
                        s2 += dd * dd;
                    }
                    if (!LOO) continue;
                    const double rr = -ll;
                    const bool cand = valid && rr > thr;
                    if (valid && !cand) sc_lse_add(bm, bs, rr);
                    if (!__any(cand)) continue;                      // wave uniform
                    for (int q = 0; q < 4; ++q) {
                        const bool mine = cand && quad == q;
                        const bool ins = mine && rr > thr;           // an earlier quarter may have raised the threshold
                        if (mine && !ins) sc_lse_add(bm, bs, rr);
                        if (!__any(ins)) continue;                   // wave uniform
                        if (ins) {
                            if (thr > -INFINITY) sc_lse_add(bm, bs, thr);     // the evicted value joins the body
                            list[pos * 16 + col] = rr;
                        }
                        __syncthreads();
                        double mv = INFINITY;
                        int mp = 0;
                        for (int k = quad; k < cnt; k += 4) {
                            const double lv = list[k * 16 + col];
                            if (lv < mv) {
                                mv = lv;
                                mp = k;
                            }
                        }
#pragma unroll
                        for (int off = 16; off <= 32; off <<= 1) {
                            const double ov = __shfl_xor(mv, off, WAVE);
                            const int op = __shfl_xor(mp, off, WAVE);
                            if (ov < mv || (ov == mv && op < mp)) {
                                mv = ov;
                                mp = op;
                            }
                        }
                        thr = mv;
                        pos = mp;
                        __syncthreads();
                    }
                }
            }
        }

        // the row's four quarters, in their order
        double LM = -INFINITY, LS = 0.0, S1 = 0.0, S2 = 0.0, BM = -INFINITY, BS = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sc_lse_merge(LM, LS, __shfl(lm, col + 16 * q, WAVE), __shfl(ls, col + 16 * q, WAVE));
            S1 += __shfl(s1, col + 16 * q, WAVE);
            S2 += __shfl(s2, col + 16 * q, WAVE);
            if (LOO) sc_lse_merge(BM, BS, __shfl(bm, col + 16 * q, WAVE), __shfl(bs, col + 16 * q, WAVE));
        }
        const double lppd = LM + (log(LS) - log(E));
        const double ll_mean = ll0 + S1 / E;
        const double p_waic = draws > 1 ? fmax((S2 - S1 * S1 / E) / (E - 1.0), 0.0) : 0.0;
        double elpd_loo = 0.0, khat = 0.0, sigma = 0.0, rmax = 0.0, m_tail = 0.0;

        if (LOO) {
            __syncthreads();
            // sort the list in place, ascending: odd-even transposition, the pairs of a phase dealt to the four lanes
            for (int ph = 0; ph < cnt; ++ph) {
                for (int i = (ph & 1) + 2 * quad; i + 1 < cnt; i += 8) {
                    const double a = list[i * 16 + col], b = list[(i + 1) * 16 + col];
                    if (a > b) {
                        list[i * 16 + col] = b;
                        list[(i + 1) * 16 + col] = a;
                    }
                }
                __syncthreads();
            }
            rmax = list[M * 16 + col];
            __syncthreads();
            for (int k = quad; k < cnt; k += 4) {
                const double s = list[k * 16 + col] - rmax;
                list[k * 16 + col] = s;
                if (tail_out && in) tail_out[(size_t)r * cnt + k] = s;
            }
            __syncthreads();
            // the cutoff, the tail strictly above it, and the raw weights of everything else
            const double u = fmax(list[col], SC_LOG_DBL_MIN), eu = exp(u);
            double B = BS > 0.0 ? BS * exp(BM - rmax) : 0.0;
            B += exp(list[col]);
            int below = 0;
            for (int k = 1; k < cnt; ++k) {
                const double s = list[k * 16 + col];
                if (!(s > u)) {
                    ++below;
                    B += exp(s);
                }
            }
            const int k0 = 1 + below, Mp = M - below;
            m_tail = (double)Mp;
            __syncthreads();
            for (int k = k0 + quad; k < cnt; k += 4) list[k * 16 + col] = exp(list[k * 16 + col]) - eu;   // exceedances
            __syncthreads();
            const int iq = min(max(k0 + (int)floor(Mp / 4.0 + 0.5) - 1, 0), M);
            const double eq = list[iq * 16 + col], emax = list[M * 16 + col];
            const bool fit = Mp > 4 && eq > 0.0;
            const int m = fit ? 30 + (int)floor(sqrt((double)Mp)) : 0;
            const double dm = (double)m, dn = (double)Mp;
            for (int j = quad + 1; j <= m; j += 4) {
                const double bj = (1.0 - sqrt(dm / ((double)j - 0.5))) / (3.0 * eq) + 1.0 / emax;
                double sum = 0.0;
                for (int k = k0; k < cnt; ++k) sum += log1p(-bj * list[k * 16 + col]);
                const double kj = sum / dn;
                prof[(j - 1) * 16 + col] = dn * (log(-bj / kj) - kj - 1.0);
            }
            __syncthreads();
            double numer = E, denom = B;
            if (fit) {
                double lmax = -INFINITY;
                for (int j = 0; j < m; ++j) lmax = fmax(lmax, prof[j * 16 + col]);
                double sw = 0.0, sb = 0.0;
                for (int j = 1; j <= m; ++j) {
                    const double bj = (1.0 - sqrt(dm / ((double)j - 0.5))) / (3.0 * eq) + 1.0 / emax;
                    const double w = exp(prof[(j - 1) * 16 + col] - lmax);
                    sw += w;
                    sb += w * bj;
                }
                const double bb = sb / sw;
                double sum = 0.0;
                for (int k = k0; k < cnt; ++k) sum += log1p(-bb * list[k * 16 + col]);
                const double kk = sum / dn;
                sigma = -kk / bb;
                khat = (dn * kk + 5.0) / (dn + 10.0);
            } else {
                khat = INFINITY;
            }
            // the tail's weights: smoothed in rank order (fit), or raw
            double sw = 0.0, sn = 0.0;
            for (int j = quad; j < Mp; j += 4) {
                const double ex = list[(k0 + j) * 16 + col], raw = ex + eu;
                double W = raw;
                if (fit) {
                    const double p = ((double)j + 0.5) / dn;
                    W = fmin(eu + sigma * expm1(-khat * log1p(-p)) / khat, 1.0);
                }
                sw += W;
                sn += W / raw;
            }
            double SW = 0.0, SN = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                SW += __shfl(sw, col + 16 * q, WAVE);
                SN += __shfl(sn, col + 16 * q, WAVE);
            }
            numer = (E - dn) + SN;
            denom = B + SW;
            elpd_loo = -rmax + (log(numer) - log(denom));
        }
        if (quad == 0 && in) {
            double *out = stats + (size_t)r * 8;
            out[0] = lppd;
            out[1] = ll_mean;
            out[2] = p_waic;
            out[3] = elpd_loo;
            out[4] = khat;
            out[5] = sigma;
            out[6] = rmax;
            out[7] = m_tail;
        }
        __syncthreads();                                 // the tile's LDS has been read: the next one may be stored
    }
}

}  // namespace fokl

extern "C" int fokl_score_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_score_report: null argument");
    std::memcpy(out, ctx->score_report, sizeof ctx->score_report);
    return FOKL_OK;
}

// fokl_score_rows (nu = INFINITY, sw = null: the Gaussian instances) and fokl_score_rows_noise; `name` opens the messages
static int score_rows_any(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sigsqd, int draws,
                          int want_loo, double *stats_out, double *tail_out, double nu, const double *sw, const char *name)
{
    using namespace fokl;
    const std::string who = name;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + ": null context");
    std::memset(ctx->score_report, 0, sizeof ctx->score_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, who + ": call fokl_upload first");
    if (nc <= 0 || draws <= 0 || !betas || !sigsqd || !stats_out)
        return fail(ctx, FOKL_ERR_ARG, who + ": bad argument");
    if (draws > (1 << 22) || nc > (1 << 20)) return fail(ctx, FOKL_ERR_ARG, who + ": too many draws or columns");
    if (tail_out && !want_loo) return fail(ctx, FOKL_ERR_ARG, who + ": tail_out is an output of want_loo");
    for (int d = 0; d < draws; ++d)
        if (!(sigsqd[d] > 0.0) || !std::isfinite(sigsqd[d]))
            return fail(ctx, FOKL_ERR_ARG, who + ": every sigsqd must be positive and finite");
    if (!(nu >= 1.0))
        return fail(ctx, FOKL_ERR_ARG, who + ": nu is NaN or < 1: Student-t noise needs nu >= 1 (INFINITY is Gaussian noise)");
    const bool student = std::isfinite(nu);
    const int noise = student ? SC_STUDENT : sw ? SC_GAUSSIAN_WEIGHTED : SC_GAUSSIAN;
    int M = 0;
    if (want_loo) {
        if (draws < FOKL_SCORE_MIN_DRAWS)
            return fail(ctx, FOKL_ERR_ARG, who + ": PSIS needs at least " + std::to_string(FOKL_SCORE_MIN_DRAWS) +
                        " draws, there are " + std::to_string(draws));
        M = std::min(draws / 5, (int)std::ceil(3.0 * std::sqrt((double)draws)));
        if (M + 1 > FOKL_SCORE_MAX_TAIL)
            return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(draws) + " draws want a tail list of " +
                        std::to_string(M + 1) + " entries per row, the kernel's LDS list holds FOKL_SCORE_MAX_TAIL = " +
                        std::to_string(FOKL_SCORE_MAX_TAIL) + " (thin the draws; want_loo = 0 has no limit)");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_slots(ctx, slots, nc, who.c_str());
    if (rc) return rc;
    const int64_t n = ctx->n;
    if (n <= 0) return fail(ctx, FOKL_ERR_STATE, who + ": the dataset has no rows");
    for (size_t i = 0; i < (size_t)draws * nc; ++i)
        if (!std::isfinite(betas[i])) return fail(ctx, FOKL_ERR_ARG, who + ": every coefficient must be finite");
    if (sw)
        for (int64_t i = 0; i < n; ++i)
            if (!(sw[i] > 0.0) || !std::isfinite(sw[i]))
                return fail(ctx, FOKL_ERR_ARG, who + ": every sw (the square root of a row's precision) must be finite and > 0");

    const int ncp = (nc + 3) & ~3, dp = (draws + 15) & ~15, cnt = M + 1;
    const size_t lds_bytes = ((size_t)ncp * 16 + (want_loo ? (size_t)cnt * 16 + (size_t)SC_GRID_MAX * 16 : 16)) * sizeof(double);
    if (lds_bytes > 160 * 1024)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(nc) + " columns and a tail list of " +
                    std::to_string(want_loo ? cnt : 0) + " entries want " + std::to_string(lds_bytes) +
                    " bytes of LDS per 16-row tile, a compute unit has 163840");
    const size_t tail_bytes = tail_out ? (size_t)n * cnt * sizeof(double) : 0;
    const size_t table_bytes = ((size_t)ncp + 2) * dp * sizeof(double);
    const size_t stats_bytes = (size_t)n * 8 * sizeof(double);
    const size_t sw_bytes = sw ? (size_t)n * sizeof(double) : 0;
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_SCORE_FREE_BYTES", &free_bytes));
    if (tail_bytes + table_bytes + stats_bytes + sw_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + ": the call wants " + std::to_string(tail_bytes + table_bytes + stats_bytes + sw_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(tail_bytes) + " bytes of tail_out = rows x (M + 1) x 8, " +
                    std::to_string(table_bytes) + " of coefficients = (columns + 2) x draws x 8, " + std::to_string(stats_bytes) +
                    " of statistics = rows x 64" + (sw ? ", " + std::to_string(sw_bytes) + " of row precisions" : std::string()) +
                    "), the device has " + std::to_string(free_bytes) + " free" +
                    (tail_bytes > table_bytes + stats_bytes ? " (pass no tail_out, or score the rows in parts)"
                     : table_bytes > stats_bytes ? " (thin the draws)" : " (score the rows in parts)"));

    // coefficients transposed and zero padded [ncp][dp] | c [dp] | h [dp] (padding draws: c = 0, h = 0, never used)
    std::vector<double> table(((size_t)ncp + 2) * dp, 0.0);
    fill_draw_table(table.data(), betas, draws, nc, ncp, dp);
    double *cons = table.data() + (size_t)ncp * dp;
    for (int d = 0; d < draws; ++d) {
        cons[d] = -0.5 * std::log(2.0 * M_PI * sigsqd[d]);
        cons[dp + d] = 0.5 / sigsqd[d];
    }
    if (student) {                                   // c [dp] | g [dp] of the t likelihood (score.student_constants)
        const double lead = std::log(student_gamma_ratio(0.5 * nu));
        for (int d = 0; d < draws; ++d) {
            cons[d] = lead - 0.5 * std::log(nu * M_PI * sigsqd[d]);
            cons[dp + d] = 1.0 / (nu * sigsqd[d]);
        }
    }
    DeviceBuffers buf;
    double *d_table = nullptr, *d_stats = nullptr, *d_tail = nullptr;
    int *d_slots = nullptr;
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc));
    HIP_TRY(ctx, buf.get(&d_stats, (size_t)n * 8));
    if (tail_out) HIP_TRY(ctx, buf.get(&d_tail, (size_t)n * cnt));
    double *d_sw = nullptr;
    if (sw) HIP_TRY(ctx, buf.upload(&d_sw, sw, (size_t)n));

    const int64_t tiles = (n + 15) / 16;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, 160 * 1024 / lds_bytes));
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)cu_count(ctx) * per_cu);
    hipError_t e = hipSuccess;
    double kernel_us = 0.0;
    auto run = [&](auto fn, auto nz) {
        e = lds_opt_in(fn, lds_bytes, 160 * 1024);
        StreamStopwatch watch(ctx, e);
        const int t0 = watch.mark();
        if (e == hipSuccess) {
            TimedRegion timed(ctx, FOKL_K_SCORE, 8.0 * (double)n * (nc + 9) + (double)tail_bytes, 2.0 * (double)n * ncp * draws);
            hipLaunchKernelGGL(fn, dim3(grid), dim3(SC_THREADS), lds_bytes, ctx->stream, ctx->d_slot_ptr, d_slots, nc, ncp,
                               d_table, d_table + (size_t)ncp * dp, draws, dp, ctx->slot_ptr[FOKL_SLOT_Y], n, M, d_stats, d_tail, nz);
            e = hipGetLastError();
        }
        const int t1 = watch.mark();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        kernel_us = watch.us(t0, t1);
    };
    if (noise == SC_STUDENT) {
        const ScNoise<SC_STUDENT> nz = {d_sw, 0.5 * (nu + 1.0)};
        want_loo ? run(score_kernel<true, SC_STUDENT>, nz) : run(score_kernel<false, SC_STUDENT>, nz);
    } else if (noise == SC_GAUSSIAN_WEIGHTED) {
        const ScNoise<SC_GAUSSIAN_WEIGHTED> nz = {d_sw};
        want_loo ? run(score_kernel<true, SC_GAUSSIAN_WEIGHTED>, nz) : run(score_kernel<false, SC_GAUSSIAN_WEIGHTED>, nz);
    } else {
        want_loo ? run(score_kernel<true, SC_GAUSSIAN>, ScNoise<SC_GAUSSIAN>{}) : run(score_kernel<false, SC_GAUSSIAN>, ScNoise<SC_GAUSSIAN>{});
    }
    if (e == hipSuccess) e = hipMemcpy(stats_out, d_stats, (size_t)n * 8 * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && tail_out) e = hipMemcpy(tail_out, d_tail, tail_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string(who + ": ") + hipGetErrorString(e));

    int64_t raw_rows = 0;
    if (want_loo)
        for (int64_t i = 0; i < n; ++i) raw_rows += std::isinf(stats_out[(size_t)i * 8 + 4]) ? 1 : 0;
    int64_t *rep = ctx->score_report;
    rep[0] = want_loo ? FOKL_SCORE_WAIC_LOO : FOKL_SCORE_WAIC;
    rep[1] = grid;
    rep[2] = tiles;
    rep[3] = (int64_t)lds_bytes;
    rep[4] = want_loo ? cnt : 0;
    rep[5] = raw_rows;
    rep[6] = (int64_t)std::llround(kernel_us);
    rep[7] = noise;
    return FOKL_OK;
}

extern "C" int fokl_score_rows(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sigsqd,
                               int draws, int want_loo, double *stats_out, double *tail_out)
{
    return score_rows_any(ctx, slots, nc, betas, sigsqd, draws, want_loo, stats_out, tail_out, INFINITY, nullptr, "fokl_score_rows");
}

// nu = INFINITY with sw = null is routed to fokl_score_rows' instances: the same kernel, the same bits
extern "C" int fokl_score_rows_noise(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sigsqd,
                                     int draws, int want_loo, double *stats_out, double *tail_out, double nu, const double *sw)
{
    return score_rows_any(ctx, slots, nc, betas, sigsqd, draws, want_loo, stats_out, tail_out, nu, sw, "fokl_score_rows_noise");
}

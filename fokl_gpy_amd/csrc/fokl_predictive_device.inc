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
//
// NOISE selects the instance (fokl_predictive_rows_noise; the statement is predictive.noise_rows_from_means):
//   PD_GAUSSIAN           the text above, and the code it compiled to before there was a choice
//   PD_GAUSSIAN_WEIGHTED  row i's components are N(mu_d, sd_d^2 / w_i): sw_i = sqrt(w_i) is read once per row next to y, rinv_d
//                         sw_i stands for rinv_d, sd_d / sw_i for sd_d in the brackets and the width, mean_sigsqd / sw_i^2 in
//                         the first trial
//   PD_STUDENT            the components are t_nu with the scale sd_d / sw_i: scal's second row holds 1 / sd_d, k = sw_i / sd_d
//                         stands for rinv_d, F = sum T_nu(t) / E and f = sum f_nu(t) k / E with student_terms
//                         (fokl_student.inc).  ONE copy of student_terms is in the code: the loop over the quantiles inside
//                         the per-draw loop is rolled too (q, and the sums it adds to, are picked by chains of selects), and
//                         the PIT is taken in a pass of its own in front of pass 1 (k = 0: the target is y, nothing is
//                         decided), not in pass 0.  Every lane calls student_terms on every draw, padding draws included
//                         (their k is 0), and adds only what counts.

namespace fokl {

constexpr int PD_THREADS = 64;
constexpr int PD_DT = 4;                         // 16-draw tiles per block: independent MFMA chains
constexpr int PD_QMAX = FOKL_PREDICTIVE_MAX_QUANTILES;

enum { PD_GAUSSIAN = FOKL_NOISE_GAUSSIAN, PD_GAUSSIAN_WEIGHTED = FOKL_NOISE_GAUSSIAN_WEIGHTED, PD_STUDENT = FOKL_NOISE_STUDENT };

// what an instance needs beyond the Gaussian one's arguments: the last kernel argument, empty for PD_GAUSSIAN
template <int NOISE> struct PdNoise {};
template <> struct PdNoise<PD_GAUSSIAN_WEIGHTED> {
    const double *sw;                            // [n] or null (ones)
};
template <> struct PdNoise<PD_STUDENT> {
    const double *sw;                            // [n] or null (ones)
    const double *tab;                           // the continued fractions' coefficients [4][ST_ROW]
    StudentArgs k;
};

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

// q[j] for a wave-uniform j, as pd_pick
template <int QA>
__device__ __forceinline__ double pd_pick_q(const double (&q)[QA], int j)
{
    double m = q[0];
#pragma unroll
    for (int t = 1; t < QA; ++t) m = (j == t) ? q[t] : m;
    return m;
}

// QM: the quantiles the instance keeps in registers (0: PIT only); args.Q <= QM of them are live
template <int QM, int NOISE>
__global__ __launch_bounds__(PD_THREADS) void predictive_kernel(double *const *__restrict__ slot_ptr,
                                                                const int *__restrict__ slots, int nc, int ncp,
                                                                const double *__restrict__ betas_t,
                                                                const double *__restrict__ scal, int draws, int dp,
                                                                const double *__restrict__ data, int64_t n, const PdArgs args,
                                                                double *__restrict__ out, int *__restrict__ tile_passes,
                                                                const PdNoise<NOISE> nz)
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
        [[maybe_unused]] double swv = 1.0, isw = 1.0;
        if constexpr (NOISE != PD_GAUSSIAN) {
            swv = (in && nz.sw) ? nz.sw[r] : 1.0;
            isw = 1.0 / swv;
        }
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
                if constexpr (NOISE == PD_GAUSSIAN) {
                    if (data) ps += 0.5 * erfc((m - yv) * scal[dp + d]);
                } else if constexpr (NOISE == PD_GAUSSIAN_WEIGHTED) {
                    if (data) ps += 0.5 * erfc((m - yv) * (scal[dp + d] * swv));
                }
#pragma unroll
                for (int j = 0; j < QM; ++j) {
                    if (j >= Q) break;
                    double c;
                    if constexpr (NOISE == PD_GAUSSIAN) c = m + sdv * args.z[j];
                    else c = m + (sdv * isw) * args.z[j];
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
        double var, width;
        if constexpr (NOISE == PD_GAUSSIAN) {
            var = fmax((S2 - S1 * S1 / E) / E, 0.0) + args.mean_sigsqd;
            width = MX - MN + args.sd_max;
        } else {
            var = fmax((S2 - S1 * S1 / E) / E, 0.0) + args.mean_sigsqd * (isw * isw);
            width = MX - MN + args.sd_max * isw;
        }
        const double sdp = sqrt(var);
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
        if (QM > 0 || NOISE == PD_STUDENT) {
            for (int k = (NOISE == PD_STUDENT && data) ? 0 : 1; k <= args.max_passes; ++k) {
                if constexpr (NOISE == PD_STUDENT) {
                    if (k > 0 && (QM == 0 || !__any(done != all_done))) break;
                    ran += k > 0;                                    // the PIT's pass is not counted, as pass 0 is not
                } else {
                    if (!__any(done != all_done)) break;             // wave uniform: every row of the tile is done
                    ++ran;
                }
                double Fs[QA], fs[QA];
#pragma unroll
                for (int j = 0; j < QA; ++j) {
                    Fs[j] = 0.0;
                    fs[j] = 0.0;
                }
                for (int d0 = 0; d0 < dp; d0 += 16 * PD_DT) {
                    d4 acc[PD_DT];
                    draw_product<PD_DT>(xs, betas_t, ncp, dp, d0, quad, col, acc);
                    if constexpr (NOISE == PD_STUDENT) {
                        const int targets = k == 0 ? 1 : Q;
#pragma unroll 1
                        for (int i = 0; i < 4 * PD_DT; ++i) {
                            const int d = d0 + 16 * (i >> 2) + quad + 4 * (i & 3);
                            const bool valid = d < draws;            // no lane leaves: student_terms is a wavefront's call
                            const double m = pd_pick(acc, i), kv = scal[dp + min(d, dp - 1)] * swv;
#pragma unroll 1
                            for (int jj = 0; jj < targets; ++jj) {   // rolled: ONE copy of student_terms
                                if (k > 0 && !__any(!((done >> jj) & 1u))) continue;     // wave uniform
                                const double target = k == 0 ? yv : pd_pick_q(q, jj);
                                double T, f;
                                student_terms((target - m) * kv, nz.k, nz.tab, T, f);
                                if (k == 0) {
                                    if (valid) ps += T;
                                    continue;
                                }
                                const bool add = valid && !((done >> jj) & 1u);
#pragma unroll
                                for (int j = 0; j < QM; ++j) {
                                    if (j == jj && add) {
                                        Fs[j] += T;
                                        fs[j] += f * kv;
                                    }
                                }
                            }
                        }
                        continue;
                    }
#pragma unroll 1
                    for (int i = 0; i < 4 * PD_DT; ++i) {            // rolled: QM copies of erfc and exp, not 16 QM
                        const int d = d0 + 16 * (i >> 2) + quad + 4 * (i & 3);
                        if (d >= draws) continue;                    // padding draws (and blocks past dp)
                        const double m = pd_pick(acc, i);
                        double rv;
                        if constexpr (NOISE == PD_GAUSSIAN) rv = scal[dp + d];
                        else rv = scal[dp + d] * swv;
#pragma unroll
                        for (int j = 0; j < QM; ++j) {
                            if ((done >> j) & 1u) continue;
                            const double tt = (q[j] - m) * rv;
                            Fs[j] += 0.5 * erfc(-tt);
                            fs[j] += exp(-(tt * tt)) * rv;
                        }
                    }
                }
                if constexpr (NOISE == PD_STUDENT) {
                    if (k == 0) {                                    // the PIT's pass: the quarters in their order, no decision
#pragma unroll
                        for (int qd = 0; qd < 4; ++qd) PS += __shfl(ps, col + 16 * qd, WAVE);
                        continue;
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

// fokl_predictive_rows (nu = INFINITY, sw = null: the Gaussian instances) and fokl_predictive_rows_noise; `name` opens the messages
static int predictive_rows_any(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sd,
                               const double *rinv, int draws, double mean_sigsqd, int with_data, const double *p, const double *z,
                               int nq, int max_passes, double ftol, double xtol, double *out, double nu, const double *sw,
                               const char *name)
{
    using namespace fokl;
    const std::string who = name;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + ": null context");
    std::memset(ctx->predictive_report, 0, sizeof ctx->predictive_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, who + ": call fokl_upload first");
    if (nc <= 0 || draws <= 0 || !betas || !sd || !rinv || !out || (nq > 0 && (!p || !z)))
        return fail(ctx, FOKL_ERR_ARG, who + ": bad argument");
    if (draws > (1 << 22) || nc > (1 << 20)) return fail(ctx, FOKL_ERR_ARG, who + ": too many draws or columns");
    if (nq < 0 || nq > FOKL_PREDICTIVE_MAX_QUANTILES)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(nq) + " quantiles, one call takes at most "
                    "FOKL_PREDICTIVE_MAX_QUANTILES = " + std::to_string(FOKL_PREDICTIVE_MAX_QUANTILES));
    if (!with_data && nq == 0)
        return fail(ctx, FOKL_ERR_ARG, who + ": neither data nor quantiles, nothing would be computed");
    if (max_passes < 0) return fail(ctx, FOKL_ERR_ARG, who + ": max_passes must be >= 0");
    if (!std::isfinite(ftol) || ftol < 0.0 || !std::isfinite(xtol) || xtol < 0.0)
        return fail(ctx, FOKL_ERR_ARG, who + ": ftol and xtol must be finite and >= 0");
    if (!(nu >= 1.0))
        return fail(ctx, FOKL_ERR_ARG, who + ": nu is NaN or < 1: Student-t noise needs nu >= 1 (INFINITY is Gaussian noise)");
    const bool student = std::isfinite(nu);
    if (student && nu > FOKL_PREDICTIVE_NU_MAX)
        return fail(ctx, FOKL_ERR_ARG, who + ": nu = " + std::to_string(nu) + " is beyond FOKL_PREDICTIVE_NU_MAX = " +
                    std::to_string(FOKL_PREDICTIVE_NU_MAX) + ", as far as the t CDF's continued fraction is bounded and tested");
    const int noise = student ? PD_STUDENT : sw ? PD_GAUSSIAN_WEIGHTED : PD_GAUSSIAN;
    if (!std::isfinite(mean_sigsqd) || !(mean_sigsqd > 0.0))
        return fail(ctx, FOKL_ERR_ARG, who + ": the mean of sigsqd must be positive and finite");
    double sd_max = 0.0;
    for (int d = 0; d < draws; ++d) {
        if (!(sd[d] > 0.0) || !std::isfinite(sd[d]) || !(rinv[d] > 0.0) || !std::isfinite(rinv[d]))
            return fail(ctx, FOKL_ERR_ARG, who + ": every sd and rinv must be positive and finite");
        sd_max = std::max(sd_max, sd[d]);
    }
    for (int j = 0; j < nq; ++j) {
        if (!std::isfinite(p[j]) || !(p[j] > 0.0) || !(p[j] < 1.0) || !std::isfinite(z[j]))
            return fail(ctx, FOKL_ERR_ARG, who + ": every quantile must lie strictly inside (0, 1), with a finite z");
        for (int k = 0; k < j; ++k)
            if (p[k] == p[j]) return fail(ctx, FOKL_ERR_ARG, who + ": the quantiles repeat a value");
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

    const int ncp = (nc + 3) & ~3, dp = (draws + 15) & ~15, stride = 6 + 5 * nq;
    const size_t lds_bytes = ((size_t)ncp * 16 + 16) * sizeof(double);
    if (lds_bytes > 160 * 1024)
        return fail(ctx, FOKL_ERR_ARG, who + ": " + std::to_string(nc) + " columns want " + std::to_string(lds_bytes) +
                    " bytes of LDS per 16-row tile, a compute unit has 163840");
    const int64_t tiles = (n + 15) / 16;
    const size_t table_bytes = ((size_t)ncp + 2) * dp * sizeof(double);
    const size_t out_bytes = (size_t)n * stride * sizeof(double);
    const size_t count_bytes = (size_t)tiles * sizeof(int);
    const size_t noise_bytes = (sw ? (size_t)n : 0) * sizeof(double) + (student ? 4 * ST_ROW * sizeof(double) : 0);
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_PREDICTIVE_FREE_BYTES", &free_bytes));
    if (table_bytes + out_bytes + count_bytes + noise_bytes + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, who + ": the call wants " + std::to_string(table_bytes + out_bytes + count_bytes + noise_bytes) +
                    " bytes on the device and 64 MiB to spare (" + std::to_string(table_bytes) +
                    " bytes of coefficients = (columns + 2) x draws x 8, " + std::to_string(out_bytes) + " of results = rows x (6 + 5 Q) x 8, " +
                    std::to_string(count_bytes) + " of pass counts" +
                    (noise_bytes ? ", " + std::to_string(noise_bytes) + " of row precisions and t coefficients" : std::string()) +
                    "), the device has " + std::to_string(free_bytes) + " free" +
                    (table_bytes > out_bytes ? " (thin the draws)" : " (take the rows in parts)"));

    // coefficients transposed and zero padded [ncp][dp] | sd [dp] | rinv [dp], under t noise 1 / sd [dp] (padding draws: zeros)
    std::vector<double> table(((size_t)ncp + 2) * dp, 0.0);
    fill_draw_table(table.data(), betas, draws, nc, ncp, dp);
    double *scal = table.data() + (size_t)ncp * dp;
    for (int d = 0; d < draws; ++d) {
        scal[d] = sd[d];
        scal[dp + d] = student ? 1.0 / sd[d] : rinv[d];
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
    args.e_sqrt_pi = student ? (double)draws : (double)draws * std::sqrt(M_PI);     // what the sum of densities is divided by
    args.Q = nq;
    args.max_passes = max_passes;

    DeviceBuffers buf;
    double *d_table = nullptr, *d_out = nullptr;
    int *d_slots = nullptr, *d_count = nullptr;
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_slots, slots, (size_t)nc));
    HIP_TRY(ctx, buf.get(&d_out, (size_t)n * stride));
    HIP_TRY(ctx, buf.get(&d_count, (size_t)tiles));
    double *d_sw = nullptr, *d_tab = nullptr;
    StudentArgs sk = {};
    if (sw) HIP_TRY(ctx, buf.upload(&d_sw, sw, (size_t)n));
    if (student) {
        std::vector<double> tab(4 * ST_ROW);
        sk = student_fill(nu, tab.data());
        HIP_TRY(ctx, buf.upload(&d_tab, tab.data(), tab.size()));
    }

    // the instance: 0, 4 or 8 quantiles in registers (Gaussian: 2, 1 and 1 wavefronts per SIMD as compiled).  The grid asks
    // for more workgroups per CU than are resident: the rest queue behind them, which evens out tiles of different pass counts
    const int waves = nq == 0 ? 16 : nq <= 4 ? 12 : 8;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(waves, 160 * 1024 / lds_bytes));
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)cu_count(ctx) * per_cu);
    hipError_t e = hipSuccess;
    double kernel_us = 0.0;
    auto run = [&](auto fn, auto nz) {
        e = lds_opt_in(fn, lds_bytes, 160 * 1024);
        StreamStopwatch watch(ctx, e);
        const int t0 = watch.mark();
        if (e == hipSuccess) {
            TimedRegion timed(ctx, FOKL_K_PREDICTIVE, 0.0, 0.0);         // bytes and flops: below, of the passes that ran
            hipLaunchKernelGGL(fn, dim3(grid), dim3(PD_THREADS), lds_bytes, ctx->stream, ctx->d_slot_ptr, d_slots, nc, ncp, d_table,
                               d_table + (size_t)ncp * dp, draws, dp, with_data ? ctx->slot_ptr[FOKL_SLOT_Y] : (double *)nullptr, n,
                               args, d_out, d_count, nz);
            e = hipGetLastError();
        }
        const int t1 = watch.mark();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        kernel_us = watch.us(t0, t1);
    };
    auto pick = [&](auto tag, auto nz) {
        constexpr int NOISE = decltype(tag)::value;
        if (nq == 0) run(predictive_kernel<0, NOISE>, nz);
        else if (nq <= 4) run(predictive_kernel<4, NOISE>, nz);
        else run(predictive_kernel<8, NOISE>, nz);
    };
    if (noise == PD_STUDENT) pick(std::integral_constant<int, PD_STUDENT>(), PdNoise<PD_STUDENT>{d_sw, d_tab, sk});
    else if (noise == PD_GAUSSIAN_WEIGHTED) pick(std::integral_constant<int, PD_GAUSSIAN_WEIGHTED>(), PdNoise<PD_GAUSSIAN_WEIGHTED>{d_sw});
    else pick(std::integral_constant<int, PD_GAUSSIAN>(), PdNoise<PD_GAUSSIAN>{});
    std::vector<int> count((size_t)tiles, 0);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(count.data(), d_count, count_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string(who + ": ") + hipGetErrorString(e));

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
    rep[9] = noise;
    return FOKL_OK;
}

extern "C" int fokl_predictive_rows(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sd,
                                    const double *rinv, int draws, double mean_sigsqd, int with_data, const double *p,
                                    const double *z, int nq, int max_passes, double ftol, double xtol, double *out)
{
    return predictive_rows_any(ctx, slots, nc, betas, sd, rinv, draws, mean_sigsqd, with_data, p, z, nq, max_passes, ftol, xtol,
                               out, INFINITY, nullptr, "fokl_predictive_rows");
}

// nu = INFINITY with sw = null is routed to fokl_predictive_rows' instances: the same kernel, the same bits
extern "C" int fokl_predictive_rows_noise(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sd,
                                          const double *rinv, int draws, double mean_sigsqd, int with_data, const double *p,
                                          const double *z, int nq, int max_passes, double ftol, double xtol, double *out, double nu,
                                          const double *sw)
{
    return predictive_rows_any(ctx, slots, nc, betas, sd, rinv, draws, mean_sigsqd, with_data, p, z, nq, max_passes, ftol, xtol,
                               out, nu, sw, "fokl_predictive_rows_noise");
}

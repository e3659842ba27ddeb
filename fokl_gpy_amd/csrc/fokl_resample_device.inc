// resample(): many independent Gibbs chains of a fitted model on the device (textually included by fokl_hip.hip).
//
// The recursion of fokl_gibbs_chain (include/fokl_hip.h: FR:1519-1548 in the eigenbasis of the Gram matrix), with the
// random numbers drawn where they are used: Philox 4x32-10 (fokl_philox.h), key (seed, chain), counter (iteration,
// purpose, index, 0).  Nothing of it depends on a stream position, so a chain needs no tape and no other chain: one
// WAVEFRONT per chain, lane l owns the eigen-coordinates l + 64 t, t < T (lam, qty, the shift and the running sums in
// registers, as gibbs_chain_kernel lays them out), RS_WAVES chains per workgroup by default, grid = chains / RS_WAVES.
// No LDS, no barrier, no atomics: a wavefront never waits for another one, and what a chain computes does not depend on
// the grid or on which chains share its workgroup.
//
// One iteration k (burn-in included):
//   g_s, g_t   the two STANDARD gamma variates of shapes astar / atau_star by Marsaglia-Tsang: attempt a draws a normal x
//              (purpose *_NORMAL, index a) and a uniform u (purpose *_UNIFORM, index a); v = (1 + c x)^3 (rejected when
//              1 + c x <= 0); accepted when u < 1 - 0.0331 (x^2)^2 or ln u < x^2 / 2 + b (1 - v + ln v) -> b v, with
//              b = shape - 1/3, c = 1 / sqrt(9 b).  Every lane evaluates the same numbers (wave-uniform: no divergence).
//              They depend on the shapes only, not on the chain's state, so they stand at the head of the iteration next
//              to the coordinates' normals and off the recursion's critical path.  At most `attempt_cap` attempts: a draw
//              that meets the cap flags the chain (reason 2) and is NaN.
//   w_i        = d_i qty_i + sqrt(sigsqd) (sqrt(d_i) z_i), d_i = 1 / (lam_i + 1 / tausqd), z_i the normal of purpose BETA, index i
//   the sums   w' diag(lam) w, w' qty, w' w: per lane over t ascending, then wave_total's fixed tree (rows of 16 by
//              DPP, the four row sums through scalar registers)
//   bstar      = b + (w'lam w - 2 w'qty + dtd + w'w / tausqd) / 2;   sigsqd = 1 / ((1 / bstar) g_s), or NaN and the chain
//              flagged (reason 1) where bstar < 0;   tausqd = 1 / ((1 / (w'w / (2 sigsqd) + btau)) g_t)
// A flagged chain is not stopped: NaN spreads through its own arithmetic from that iteration on, as FR:1538-1541 leaves it.
//
// Kept iterations (k >= burnin, (k - burnin) % thin == 0) write their row of w (P + 1 consecutive doubles), sigsqd, tausqd
// and the attempts both gammas took.  Every post-burn-in iteration adds w_i - shift_i, its square, and sigsqd, tausqd and
// their squares to running sums that are written out and cleared at the middle and at the end of the post-burn-in run (and
// once more for the odd last iteration): the per-chain sums of the two halves split R-hat needs, with no row kept.

namespace fokl {

constexpr int RS_WAVES = 4;                      // chains per workgroup by default: one wavefront on each SIMD of a CU
constexpr int RS_MAX_WAVES = 4;                  // at most: one wavefront per SIMD may use all 512 registers (T = 12 needs ~300)
constexpr int RS_MAX_T = 12;                     // elements per lane: models of up to 768 columns (kChainMaxT's bar)
constexpr int RS_ATTEMPT_CAP = 64;               // Marsaglia-Tsang accepts > 95 % of its attempts at any shape >= 1
constexpr int RS_SEGMENTS = 3;                   // first half, second half, the odd last iteration

struct ResampleArgs {
    const double *lamb, *qty, *shift;            // [p1]
    const double *sig0, *tau0;                   // [chains]: where each chain starts
    double *w;                                   // [chains][kept][p1], or null: no rows
    double *sig, *tau;                           // [chains][kept] (with w)
    int32_t *attempts;                           // [chains][kept] (with w): attempts of the row's two gammas
    double *sums;                                // [chains][RS_SEGMENTS][2][p1 + 2]: sum, sum of squares | w - shift, sigsqd, tausqd
    long long *counts;                           // [chains][4]: first flagged iteration (-1), reason, attempts, most of one draw
    double sig_b, sig_c, tau_b, tau_c;           // Marsaglia-Tsang constants of the two shapes
    double b, btau, dtd;
    int p1, chains, burnin, draws, thin, kept, attempt_cap;
    uint32_t seed;
};

// One standard gamma variate of shape b + 1/3, wave-uniform.  -> NaN after `cap` rejected attempts.
__device__ __forceinline__ double resample_gamma(uint32_t seed, uint32_t chain, uint32_t k, int purpose_normal,
                                                 int purpose_uniform, double b, double c, int cap, int &attempts)
{
    for (int a = 0; a < cap; ++a) {
        ++attempts;
        const double x = emb_normal(seed, chain, k, (uint32_t)purpose_normal, (uint32_t)a);
        const double u = emb_uniform(seed, chain, k, (uint32_t)purpose_uniform, (uint32_t)a);
        const double v1 = 1.0 + c * x;
        if (v1 <= 0.0) continue;
        const double v = (v1 * v1) * v1, x2 = x * x;
        if (u < 1.0 - 0.0331 * (x2 * x2) || log(u) < 0.5 * x2 + b * ((1.0 - v) + log(v))) return b * v;
    }
    return __builtin_nan("");
}

template <int T>
__global__ __launch_bounds__(64 * RS_MAX_WAVES) void resample_chains_kernel(const ResampleArgs a)
{
    const int lane = threadIdx.x & 63;
    const int chain = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (chain >= a.chains) return;               // (no barrier anywhere below)
    const int p1 = a.p1;
    double lam[T], qt[T], sh[T], run_s[T], run_q[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int i = lane + 64 * t;
        lam[t] = i < p1 ? a.lamb[i] : 1.0;
        qt[t] = i < p1 ? a.qty[i] : 0.0;
        sh[t] = i < p1 ? a.shift[i] : 0.0;
        run_s[t] = run_q[t] = 0.0;
    }
    double sigsqd = a.sig0[chain], tausqd = a.tau0[chain];
    double sig_s = 0.0, sig_q = 0.0, tau_s = 0.0, tau_q = 0.0;
    long long flagged_at = -1, attempts_total = 0;
    int reason = 0, attempts_most = 0;
    const int total = a.burnin + a.draws, half = a.draws / 2, stride = p1 + 2;
    double *my_sums = a.sums + (size_t)chain * RS_SEGMENTS * 2 * stride;

    auto flush = [&](int segment) {
        double *s = my_sums + (size_t)segment * 2 * stride, *q = s + stride;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int i = lane + 64 * t;
            if (i < p1) {
                s[i] = run_s[t];
                q[i] = run_q[t];
            }
            run_s[t] = run_q[t] = 0.0;
        }
        if (lane == 0) {
            s[p1] = sig_s, s[p1 + 1] = tau_s;
            q[p1] = sig_q, q[p1 + 1] = tau_q;
        }
        sig_s = sig_q = tau_s = tau_q = 0.0;
    };

    for (int k = 0; k < total; ++k) {
        // what does not depend on the chain's state: the two gamma variates and the coordinates' normals
        int att_s = 0, att_t = 0;
        const double gs = resample_gamma(a.seed, (uint32_t)chain, (uint32_t)k, RES_PURPOSE_SIG_NORMAL, RES_PURPOSE_SIG_UNIFORM,
                                         a.sig_b, a.sig_c, a.attempt_cap, att_s);
        const double gt = resample_gamma(a.seed, (uint32_t)chain, (uint32_t)k, RES_PURPOSE_TAU_NORMAL, RES_PURPOSE_TAU_UNIFORM,
                                         a.tau_b, a.tau_c, a.attempt_cap, att_t);
        double z[T];
#pragma unroll
        for (int t = 0; t < T; ++t)
            z[t] = emb_normal(a.seed, (uint32_t)chain, (uint32_t)k, (uint32_t)RES_PURPOSE_BETA, (uint32_t)(lane + 64 * t));

        const double inv_tau = 1.0 / tausqd, sig = sqrt(sigsqd);
        double w[T], p_lam = 0.0, p_ty = 0.0, p_ww = 0.0;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const double d = 1.0 / (lam[t] + inv_tau);
            const double wi = d * qt[t] + sig * (sqrt(d) * z[t]);
            const double ww = wi * wi;
            const bool mine = lane + 64 * t < p1;
            w[t] = wi;
            p_lam += mine ? lam[t] * ww : 0.0;
            p_ty += mine ? wi * qt[t] : 0.0;
            p_ww += mine ? ww : 0.0;
        }
        const double q_lam = wave_total(p_lam), q_ty = wave_total(p_ty), q_ww = wave_total(p_ww);
        const double bstar = a.b + 0.5 * (((q_lam - 2.0 * q_ty) + a.dtd) + q_ww / tausqd);
        const bool negative = bstar < 0.0;
        sigsqd = negative ? __builtin_nan("") : 1.0 / ((1.0 / bstar) * gs);
        const double btau_star = (1.0 / (2.0 * sigsqd)) * q_ww + a.btau;
        tausqd = 1.0 / ((1.0 / btau_star) * gt);

        const bool capped = gs != gs || gt != gt;
        if ((negative || capped) && flagged_at < 0) {
            flagged_at = k;
            reason = negative ? 1 : 2;
        }
        attempts_total += att_s + att_t;
        attempts_most = max(attempts_most, max(att_s, att_t));

        const int j = k - a.burnin;
        if (j < 0) continue;
        if (a.w && j % a.thin == 0) {
            const size_t row = (size_t)chain * a.kept + (size_t)(j / a.thin);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int i = lane + 64 * t;
                if (i < p1) a.w[row * p1 + i] = w[t];
            }
            if (lane == 0) {
                a.sig[row] = sigsqd;
                a.tau[row] = tausqd;
                a.attempts[row] = att_s + att_t;
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const double d = w[t] - sh[t];
            run_s[t] += d;
            run_q[t] += d * d;
        }
        sig_s += sigsqd, sig_q += sigsqd * sigsqd;
        tau_s += tausqd, tau_q += tausqd * tausqd;
        if (j + 1 == half) flush(0);
        else if (j + 1 == 2 * half) flush(1);
    }
    if (a.draws & 1) flush(2);
    if (lane == 0) {
        long long *c = a.counts + (size_t)chain * 4;
        c[0] = flagged_at;
        c[1] = reason;
        c[2] = attempts_total;
        c[3] = attempts_most;
    }
}

template <int T>
static hipError_t launch_resample(const ResampleArgs &args, int waves, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args.chains + waves - 1) / waves);
    hipLaunchKernelGGL((resample_chains_kernel<T>), dim3(grid), dim3(64 * waves), 0, stream, args);
    return hipGetLastError();
}

}  // namespace fokl

extern "C" int fokl_resample_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_resample_report: null argument");
    std::memcpy(out, ctx->resample_report, sizeof ctx->resample_report);
    return FOKL_OK;
}

extern "C" int fokl_resample_chains(fokl_ctx *ctx, int p1, const double *lamb, const double *qty, const double *shift,
                                    double astar, double atau_star, double b, double btau, double dtd, int chains,
                                    const double *sigsqd0, const double *tausqd0, int burnin, int draws, int thin,
                                    uint32_t seed, int chains_per_group, int attempt_cap, double *w_out, double *sig_out,
                                    double *tau_out, int32_t *attempts_out, double *sums_out, int64_t *counts_out)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_resample_chains: null context");
    std::memset(ctx->resample_report, 0, sizeof ctx->resample_report);
    if (!lamb || !qty || !shift || !sigsqd0 || !tausqd0 || !sums_out || !counts_out)
        return fail(ctx, FOKL_ERR_ARG, "fokl_resample_chains: null argument");
    if (p1 < 1 || p1 > 64 * RS_MAX_T)
        return fail(ctx, FOKL_ERR_ARG, "fokl_resample_chains: the model has " + std::to_string(p1) + " columns, the kernel is "
                    "instantiated for at most " + std::to_string(64 * RS_MAX_T) + " (12 per lane: the bar of the device chain "
                    "engine, FOKL_DCHAIN_MAX_COLUMNS, not a register budget)");
    if (!(astar >= 1.0) || !(atau_star >= 1.0))
        return fail(ctx, FOKL_ERR_ARG, "fokl_resample_chains: the gamma sampler is Marsaglia-Tsang's for shapes >= 1 "
                    "(astar and atau + P / 2 must be at least 1)");
    if (chains < 1 || chains > (1 << 20) || burnin < 0 || draws < 1 || thin < 1 || (int64_t)burnin + draws > (1 << 30))
        return fail(ctx, FOKL_ERR_ARG, "fokl_resample_chains: chains in 1 .. 1 048 576, burnin >= 0, draws >= 1, thin >= 1, "
                    "burnin + draws <= 2^30");
    if (chains_per_group < 0 || chains_per_group > RS_MAX_WAVES || attempt_cap < 0 || attempt_cap > 1024)
        return fail(ctx, FOKL_ERR_ARG, "fokl_resample_chains: chains per workgroup in 1 .. 4 (0: the default, 4), attempt "
                    "cap in 1 .. 1024 (0: the default, 64)");
    const bool rows = w_out != nullptr;
    if (rows != (sig_out != nullptr) || rows != (tau_out != nullptr) || rows != (attempts_out != nullptr))
        return fail(ctx, FOKL_ERR_ARG, "fokl_resample_chains: rows are kept (w, sigsqd, tausqd, attempts) or not at all");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int kept = (draws + thin - 1) / thin, waves = chains_per_group ? chains_per_group : RS_WAVES;
    const size_t n_rows = rows ? (size_t)chains * kept : 0, row_bytes = n_rows * (size_t)p1 * sizeof(double);
    const size_t n_sums = (size_t)chains * RS_SEGMENTS * 2 * (p1 + 2);
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    const size_t other = n_rows * (2 * sizeof(double) + sizeof(int32_t)) + n_sums * sizeof(double) + (64 << 20);
    if (row_bytes + other > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, "fokl_resample_chains: chains x kept x (P + 1) x 8 = " + std::to_string(row_bytes) +
                    " bytes of rows, the device has " + std::to_string(free_bytes) + " free (thin, or keep no rows)");

    DeviceBuffers buf;
    ResampleArgs args = {};
    double *d_lamb = nullptr, *d_qty = nullptr, *d_shift = nullptr, *d_sig0 = nullptr, *d_tau0 = nullptr;
    HIP_TRY(ctx, buf.upload(&d_lamb, lamb, (size_t)p1));
    HIP_TRY(ctx, buf.upload(&d_qty, qty, (size_t)p1));
    HIP_TRY(ctx, buf.upload(&d_shift, shift, (size_t)p1));
    HIP_TRY(ctx, buf.upload(&d_sig0, sigsqd0, (size_t)chains));
    HIP_TRY(ctx, buf.upload(&d_tau0, tausqd0, (size_t)chains));
    HIP_TRY(ctx, buf.get(&args.sums, n_sums));
    HIP_TRY(ctx, buf.get(&args.counts, (size_t)chains * 4));
    HIP_TRY(ctx, hipMemsetAsync(args.sums, 0, n_sums * sizeof(double), ctx->stream));   // (a segment without iterations stays 0)
    if (rows) {
        HIP_TRY(ctx, buf.get(&args.w, n_rows * (size_t)p1));
        HIP_TRY(ctx, buf.get(&args.sig, n_rows));
        HIP_TRY(ctx, buf.get(&args.tau, n_rows));
        HIP_TRY(ctx, buf.get(&args.attempts, n_rows));
    }
    args.lamb = d_lamb, args.qty = d_qty, args.shift = d_shift, args.sig0 = d_sig0, args.tau0 = d_tau0;
    args.sig_b = astar - 1.0 / 3.0, args.sig_c = 1.0 / std::sqrt(9.0 * args.sig_b);
    args.tau_b = atau_star - 1.0 / 3.0, args.tau_c = 1.0 / std::sqrt(9.0 * args.tau_b);
    args.b = b, args.btau = btau, args.dtd = dtd;
    args.p1 = p1, args.chains = chains, args.burnin = burnin, args.draws = draws, args.thin = thin, args.kept = kept;
    args.attempt_cap = attempt_cap ? attempt_cap : RS_ATTEMPT_CAP;
    args.seed = seed;

    // the smallest instance that holds the model: T = 1, 2, 3, 4, 6, 8, 12 elements per lane
    const int need = (p1 + 63) / 64;
    const int T = need <= 4 ? need : need <= 6 ? 6 : need <= 8 ? 8 : 12;
    hipError_t e = hipSuccess;
    StreamStopwatch watch(ctx, e);
    const int t0 = watch.mark();
    if (e == hipSuccess) {
        const int64_t iters = (int64_t)burnin + draws;
        TimedRegion timed(ctx, FOKL_K_RESAMPLE, (double)row_bytes, 40.0 * (double)chains * (double)iters * p1);
        switch (T) {
        case 1: e = launch_resample<1>(args, waves, ctx->stream); break;
        case 2: e = launch_resample<2>(args, waves, ctx->stream); break;
        case 3: e = launch_resample<3>(args, waves, ctx->stream); break;
        case 4: e = launch_resample<4>(args, waves, ctx->stream); break;
        case 6: e = launch_resample<6>(args, waves, ctx->stream); break;
        case 8: e = launch_resample<8>(args, waves, ctx->stream); break;
        default: e = launch_resample<12>(args, waves, ctx->stream); break;
        }
    }
    const int t1 = watch.mark();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    const double kernel_us = watch.us(t0, t1);
    if (e == hipSuccess) e = hipMemcpy(sums_out, args.sums, n_sums * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(counts_out, args.counts, (size_t)chains * 4 * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows) e = hipMemcpy(w_out, args.w, row_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows) e = hipMemcpy(sig_out, args.sig, n_rows * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows) e = hipMemcpy(tau_out, args.tau, n_rows * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows) e = hipMemcpy(attempts_out, args.attempts, n_rows * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_resample_chains: ") + hipGetErrorString(e));

    int64_t *rep = ctx->resample_report;
    int64_t attempts = 0, most = 0, flagged = 0;
    for (int c = 0; c < chains; ++c) {
        flagged += counts_out[(size_t)c * 4] >= 0;
        attempts += counts_out[(size_t)c * 4 + 2];
        most = std::max(most, counts_out[(size_t)c * 4 + 3]);
    }
    rep[0] = T;
    rep[1] = chains;
    rep[2] = (int64_t)burnin + draws;
    rep[3] = waves;
    rep[4] = attempts;
    rep[5] = most;
    rep[6] = (int64_t)std::llround(kernel_us);
    rep[7] = (chains + waves - 1) / waves;
    rep[8] = flagged;
    rep[9] = kept;
    return FOKL_OK;
}

// resample_robust(): Gibbs chains under Student-t noise and given row weights (textually included by fokl_hip.hip).  The
// statement is fokl_gpy_amd/robust.py: pass_host, step_host, robust_host.
//
// With a latent precision lam_i per row the Gram [1|X|y]' diag(w lam) [1|X|y] changes every iteration, so an iteration is
// a weighted pass over all rows.  Three kernels per iteration on the context's stream, no host round trip between
// iterations; the grid's second dimension is the chain:
//
//   robust_pass_kernel<NB>   a workgroup of four wavefronts owns a range of 64-row chunks that depends on n alone.  Per
//       chunk it stages the m = P + 2 columns [1|X|y] from the slots into LDS [column][row] (the next chunk's values
//       travel in registers meanwhile), forms x . beta per row (quarter q of the workgroup adds the columns q, q + 4, ...,
//       then (q0 + q1) + (q2 + q3)), the residual and lam_i = g_i / ((nu + w_i r_i^2 / sigsqd) / 2) with g_i a standard
//       gamma of shape (nu + 1) / 2 by Marsaglia-Tsang (Philox family 4: key (seed, chain), counter (iteration, purpose +
//       16 attempt, row, 4)), adds lam_i into the chain's per-row accumulator once the iteration is past the burn-in, and
//       accumulates the upper block triangle of G on v_mfma_f64_16x16x4_f64: A = a 16-column block [row][column], B =
//       a 16-column block times w lam.  The NB (NB + 1) / 2 block pairs are dealt to the four wavefronts (pair p to
//       wavefront p & 3: 9 each at NB = 8) and stay in their registers for the whole range: no reduction across
//       wavefronts, no atomics.  Each workgroup writes one partial G [pair][16][16] and its attempt counters.
//   robust_reduce_kernel     one workgroup per block pair and chain sums the partials in workgroup order and writes G
//       [16 NB][16 NB] symmetric (the lower block triangle, and the lower triangle of a diagonal block, are copies).
//   robust_step_kernel       one workgroup per chain, G in LDS: A = G_xx + I / tausqd = L L' in place in the lower triangle
//       (right-looking, no pivoting; the upper triangle and a saved diagonal keep G), L u = c, L' beta = u + sqrt(sigsqd) z,
//       S = G_yy - 2 beta . c + beta' G_xx beta by wave_total's tree, the two gamma variates, the kept row and the sums.
//
// lam = 1 at iteration 0 and under nu = inf.  Rows past n and columns past m are zeros in LDS.  A row whose variate meets
// the attempt cap is NaN, and so is its chain from there on; so is a chain with bstar < 0 or a pivot that is not positive.

namespace fokl {

constexpr int RB_THREADS = 256;
constexpr int RB_ROWS = 64;                      // rows of a chunk
constexpr int RB_LD = 66;                        // doubles between two columns of a chunk in LDS: 16 columns x 2 row quarters read 32 banks pairs apart
constexpr int RB_MAX_GROUPS = 256;               // workgroups (partials) per chain at most
constexpr int RB_MAX_NB = 8;
constexpr int RB_STATE_LD = 128;                 // doubles of a chain's beta in the state buffer
constexpr int RB_TIMED = 64;                     // iterations (the last ones) whose launches are timed one by one

struct RobustArgs {
    double *const *slot_ptr;
    const int *slots;                            // [m]: the columns, then y
    const double *weights;                       // [n], or null: ones
    const int *chain_ids;                        // [chains]: what keys the generator
    int64_t n, chunks, chunks_per_group;
    int nc, m, nb, groups, chains;
    int draw, attempt_cap;                       // draw: nu is finite
    double nu, lam_b, lam_c;
    uint32_t seed;
    // state and workspaces
    double *beta;                                // [chains][RB_STATE_LD]
    double *sig, *tau;                           // [chains]
    double *partial;                             // [chains][groups][pairs][256]
    long long *pcount;                           // [chains][groups][4]: attempts, capped rows, the most of one row
    double *G;                                   // [chains][16 nb][16 nb]
    long long *gcount;                           // [chains][4]: the same, summed over the groups
    double *lam_out;                             // [n] or null (chain 0: fokl_robust_pass)
    int *att_out;                                // [n] or null
    double *lam_sum;                             // [chains][n] or null
    // the step
    const double *shift;                         // [nc]
    double sig_b, sig_c, tau_b, tau_c, b, btau;
    int burnin, draws, thin, kept;
    double *betas_out, *sig_out, *tau_out;       // [chains][kept][nc], [chains][kept], or null
    long long *attempts_out;                     // [chains][kept]
    double *run;                                 // [chains][2][nc + 2]
    double *sums;                                // [chains][3][2][nc + 2]
    long long *counts;                           // [chains][4]
};

// One standard gamma variate of shape b + 1/3 of (chain, iteration k) for `index`.  -> NaN after `cap` rejected attempts.
__device__ inline double robust_gamma(uint32_t seed, uint32_t chain, uint32_t k, int purpose_normal, int purpose_uniform,
                                      uint32_t index, double b, double c, int cap, int &attempts)
{
    for (int a = 0; a < cap; ++a) {
        ++attempts;
        const double x = rob_normal(seed, chain, k, (uint32_t)(purpose_normal + ROB_ATTEMPT_STRIDE * a), index);
        const double u = rob_uniform(seed, chain, k, (uint32_t)(purpose_uniform + ROB_ATTEMPT_STRIDE * a), index);
        const double v1 = 1.0 + c * x;
        if (v1 <= 0.0) continue;
        const double v = (v1 * v1) * v1, x2 = x * x;
        if (u < 1.0 - 0.0331 * (x2 * x2) || log(u) < 0.5 * x2 + b * ((1.0 - v) + log(v))) return b * v;
    }
    return __builtin_nan("");
}

// The product phase of one chunk for wavefront Q: 16 steps of 4 rows; pair p = (bi <= bj) in row-major order is Q's when
// (p & 3) == Q and lives in acc[p >> 2].
template <int NB, int Q>
__device__ __forceinline__ void robust_products(const double *zs, const double *wl, int col, int quad, d4 *acc)
{
    for (int r0 = 0; r0 < RB_ROWS; r0 += 4) {
        const double wv = wl[r0 + quad];
        double az[NB], bz[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            az[b] = zs[(16 * b + col) * RB_LD + r0 + quad];
            bz[b] = az[b] * wv;
        }
        int p = 0;
#pragma unroll
        for (int bi = 0; bi < NB; ++bi)
#pragma unroll
            for (int bj = bi; bj < NB; ++bj, ++p)
                if ((p & 3) == Q) acc[p >> 2] = __builtin_amdgcn_mfma_f64_16x16x4f64(az[bi], bz[bj], acc[p >> 2], 0, 0, 0);
    }
}

template <int NB, int Q>
__device__ __forceinline__ void robust_store_pairs(double *out, int col, int quad, const d4 *acc)
{
    int p = 0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
        for (int bj = bi; bj < NB; ++bj, ++p)
            if ((p & 3) == Q) {
#pragma unroll
                for (int v = 0; v < 4; ++v) out[(size_t)p * 256 + (quad + 4 * v) * 16 + col] = acc[p >> 2][v];
            }
}

template <int NB>
__global__ __launch_bounds__(RB_THREADS) void robust_pass_kernel(const RobustArgs a, uint32_t k, int accumulate)
{
    constexpr int NP = NB * (NB + 1) / 2, OWN = (NP + 3) / 4, PER = NB * 4;   // PER: columns a thread stages
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *zs = lds;                                // [16 NB][RB_LD]
    double *wl = zs + 16 * NB * RB_LD;               // [64]: w lam of the chunk's rows
    double *part = wl + RB_ROWS;                     // [4][64]: the quarters' partial x . beta
    double *bs = part + 4 * RB_ROWS;                 // [16 NB]: beta
    const double **cp = (const double **)(bs + 16 * NB);   // [16 NB]: the columns' base pointers
    const int t = threadIdx.x, r = t & 63, q = t >> 6, col = r & 15, quad = r >> 4;
    const int c = blockIdx.y, g = blockIdx.x;
    const uint32_t chain = (uint32_t)a.chain_ids[c];
    const bool draw = a.draw && k > 0;
    if (t < 16 * NB) {
        bs[t] = (draw && t < a.nc) ? a.beta[(size_t)c * RB_STATE_LD + t] : 0.0;
        cp[t] = t < a.m ? a.slot_ptr[a.slots[t]] : nullptr;
    }
    const double sig = draw ? a.sig[c] : 1.0;
    d4 acc[OWN];
#pragma unroll
    for (int o = 0; o < OWN; ++o) acc[o] = (d4){0.0, 0.0, 0.0, 0.0};
    long long att_sum = 0, capped = 0;
    int att_most = 0;
    const int64_t chunk0 = (int64_t)g * a.chunks_per_group;
    const int64_t chunk1 = chunk0 + a.chunks_per_group < a.chunks ? chunk0 + a.chunks_per_group : a.chunks;
    __syncthreads();                                 // cp

    double pre[PER];
    auto fetch = [&](int64_t chunk) {
        const int64_t row = chunk * RB_ROWS + r;
        const bool in = row < a.n;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int kk = q + 4 * i;
            pre[i] = (in && kk < a.m) ? cp[kk][row] : 0.0;
        }
    };
    if (chunk0 < chunk1) fetch(chunk0);
    for (int64_t chunk = chunk0; chunk < chunk1; ++chunk) {
        const int64_t row = chunk * RB_ROWS + r;
        const bool in = row < a.n;
#pragma unroll
        for (int i = 0; i < PER; ++i) zs[(q + 4 * i) * RB_LD + r] = pre[i];
        __syncthreads();
        if (chunk + 1 < chunk1) fetch(chunk + 1);    // on its way during this chunk's arithmetic
        if (draw) {
            double p = 0.0;
            for (int kk = q; kk < a.nc; kk += 4) p += zs[kk * RB_LD + r] * bs[kk];
            part[q * RB_ROWS + r] = p;
            __syncthreads();
        }
        if (q == 0) {
            const double wv = in ? (a.weights ? a.weights[row] : 1.0) : 0.0;
            double lam = 1.0;
            int att = 0;
            if (draw && in) {
                const double xb = (part[r] + part[RB_ROWS + r]) + (part[2 * RB_ROWS + r] + part[3 * RB_ROWS + r]);
                const double res = zs[a.nc * RB_LD + r] - xb;
                const double gam = robust_gamma(a.seed, chain, k, ROB_PURPOSE_LAM_NORMAL, ROB_PURPOSE_LAM_UNIFORM, (uint32_t)row,
                                                a.lam_b, a.lam_c, a.attempt_cap, att);
                lam = gam / (0.5 * (a.nu + (wv * (res * res)) / sig));
                att_sum += att;
                att_most = att > att_most ? att : att_most;
                capped += gam != gam;
            }
            wl[r] = in ? wv * lam : 0.0;
            if (in) {
                if (a.lam_out) a.lam_out[row] = lam;
                if (a.att_out) a.att_out[row] = att;
                if (accumulate && a.lam_sum) a.lam_sum[(size_t)c * a.n + row] += lam;   // this row has one owner
            }
        }
        __syncthreads();
        switch (q) {
        case 0: robust_products<NB, 0>(zs, wl, col, quad, acc); break;
        case 1: robust_products<NB, 1>(zs, wl, col, quad, acc); break;
        case 2: robust_products<NB, 2>(zs, wl, col, quad, acc); break;
        default: robust_products<NB, 3>(zs, wl, col, quad, acc); break;
        }
        __syncthreads();                             // the chunk's LDS has been read: the next one may be stored
    }

    double *out = a.partial + ((size_t)c * a.groups + g) * ((size_t)NP * 256);
    switch (q) {
    case 0: robust_store_pairs<NB, 0>(out, col, quad, acc); break;
    case 1: robust_store_pairs<NB, 1>(out, col, quad, acc); break;
    case 2: robust_store_pairs<NB, 2>(out, col, quad, acc); break;
    default: robust_store_pairs<NB, 3>(out, col, quad, acc); break;
    }
    long long *cnt = (long long *)part;              // [3][64] (the last chunk's barrier is behind)
    if (q == 0) {
        cnt[r] = att_sum;
        cnt[RB_ROWS + r] = capped;
        cnt[2 * RB_ROWS + r] = att_most;
    }
    __syncthreads();
    if (t == 0) {
        long long s = 0, cap = 0, most = 0;
        for (int i = 0; i < RB_ROWS; ++i) {
            s += cnt[i];
            cap += cnt[RB_ROWS + i];
            most = cnt[2 * RB_ROWS + i] > most ? cnt[2 * RB_ROWS + i] : most;
        }
        long long *pc = a.pcount + ((size_t)c * a.groups + g) * 4;
        pc[0] = s, pc[1] = cap, pc[2] = most, pc[3] = 0;
    }
}

// grid (pairs, chains): element e of pair p summed over the groups in their order.
__global__ __launch_bounds__(RB_THREADS) void robust_reduce_kernel(const RobustArgs a)
{
    __shared__ long long cnt[3][RB_MAX_GROUPS];
    const int p = blockIdx.x, c = blockIdx.y, e = threadIdx.x;
    const int nb = a.nb, np = nb * (nb + 1) / 2, ld = 16 * nb;
    const size_t stride = (size_t)np * 256;
    const double *src = a.partial + (size_t)c * a.groups * stride + (size_t)p * 256 + e;
    double s = 0.0;
#pragma unroll 8
    for (int g = 0; g < a.groups; ++g) s += src[(size_t)g * stride];
    int bi = 0, rest = p;
    while (rest >= nb - bi) {
        rest -= nb - bi;
        ++bi;
    }
    const int bj = bi + rest, i = 16 * bi + (e >> 4), j = 16 * bj + (e & 15);
    double *G = a.G + (size_t)c * ld * ld;
    if (i <= j) {                                    // (a diagonal block: its upper triangle, mirrored)
        G[(size_t)i * ld + j] = s;
        G[(size_t)j * ld + i] = s;
    }
    if (p != 0) return;
    const long long *pc = a.pcount + (size_t)c * a.groups * 4;
    for (int w = 0; w < 3; ++w) cnt[w][e] = e < a.groups ? pc[(size_t)e * 4 + w] : 0;
    __syncthreads();
    if (e == 0) {
        long long sum = 0, cap = 0, most = 0;
        for (int g = 0; g < a.groups; ++g) {
            sum += cnt[0][g];
            cap += cnt[1][g];
            most = cnt[2][g] > most ? cnt[2][g] : most;
        }
        long long *gc = a.gcount + (size_t)c * 4;
        gc[0] = sum, gc[1] = cap, gc[2] = most, gc[3] = 0;
    }
}

// grid (chains): steps 2-4 of iteration k on the chain's G.
__global__ __launch_bounds__(RB_THREADS) void robust_step_kernel(const RobustArgs a, uint32_t k)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x, c = blockIdx.x, nc = a.nc, m = a.m, ld = 16 * a.nb, lda = m | 1;
    double *Gs = lds;                                // [m][lda]: upper triangle G, lower triangle L (below the diagonal)
    double *gdiag = Gs + (size_t)m * lda;            // [128] the diagonal of G
    double *dvec = gdiag + 128;                      // [128] the diagonal of L
    double *uvec = dvec + 128;                       // [128] right-hand side at work
    double *usol = uvec + 128;                       // [128] u, then beta
    double *term = usol + 128;                       // [3][128]
    double *totals = term + 3 * 128;                 // [3] (no static LDS: the dynamic limit is raised to all 160 KiB)
    const uint32_t chain = (uint32_t)a.chain_ids[c];
    const double *G = a.G + (size_t)c * ld * ld;
    const double sigsqd = a.sig[c], tausqd = a.tau[c];
    const double inv_tau = 1.0 / tausqd, root_sig = sqrt(sigsqd);

    for (int e = t; e < m * m; e += RB_THREADS) {
        const int i = e / m, j = e - i * m;
        Gs[i * lda + j] = i <= j ? G[(size_t)i * ld + j] : G[(size_t)j * ld + i];   // the upper triangle is what is read
    }
    __syncthreads();
    if (t < m) gdiag[t] = Gs[t * lda + t];
    __syncthreads();
    if (t < nc) Gs[t * lda + t] = gdiag[t] + inv_tau;
    __syncthreads();

    bool bad = false;
    for (int j = 0; j < nc; ++j) {
        double pivot = Gs[j * lda + j];
        if (!(pivot > 0.0)) {
            bad = true;
            pivot = __builtin_nan("");
        }
        const double d = sqrt(pivot);
        if (t == 0) dvec[j] = d;
        for (int i = j + 1 + t; i < nc; i += RB_THREADS) Gs[i * lda + j] = Gs[i * lda + j] / d;
        __syncthreads();
        for (int i = j + 1 + (t >> 4); i < nc; i += RB_THREADS / 16) {
            const double lij = Gs[i * lda + j];
            for (int kk = j + 1 + (t & 15); kk <= i; kk += 16) Gs[i * lda + kk] = Gs[i * lda + kk] - lij * Gs[kk * lda + j];
        }
        __syncthreads();
    }

    if (t < nc) uvec[t] = Gs[t * lda + nc];          // c = G_xy
    __syncthreads();
    for (int j = 0; j < nc; ++j) {                   // L u = c
        const double uj = uvec[j] / dvec[j];
        if (t == 0) usol[j] = uj;
        for (int i = j + 1 + t; i < nc; i += RB_THREADS) uvec[i] = uvec[i] - Gs[i * lda + j] * uj;
        __syncthreads();
    }
    if (t < nc) uvec[t] = usol[t] + root_sig * rob_normal(a.seed, chain, k, (uint32_t)ROB_PURPOSE_BETA, (uint32_t)t);
    __syncthreads();
    for (int j = nc - 1; j >= 0; --j) {              // L' beta = u + sqrt(sigsqd) z
        const double bj = uvec[j] / dvec[j];
        if (t == 0) usol[j] = bj;
        for (int i = t; i < j; i += RB_THREADS) uvec[i] = uvec[i] - Gs[j * lda + i] * bj;
        __syncthreads();
    }
    if (t < 128) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        if (t < nc) {
            double gb = 0.0;                         // (G_xx beta)_t, columns in ascending order
            for (int j = 0; j < nc; ++j) {
                const double gij = j > t ? Gs[t * lda + j] : (j < t ? Gs[j * lda + t] : gdiag[t]);
                gb = gb + gij * usol[j];
            }
            const double bt = usol[t];
            t0 = bt * Gs[t * lda + nc], t1 = bt * gb, t2 = bt * bt;
        }
        term[t] = t0, term[128 + t] = t1, term[256 + t] = t2;
    }
    __syncthreads();
    if (t < 64) {                                    // resample's wave_sum: lane l adds its elements l, l + 64, then the tree
        const double q0 = wave_total((0.0 + term[t]) + term[64 + t]);
        const double q1 = wave_total((0.0 + term[128 + t]) + term[128 + 64 + t]);
        const double q2 = wave_total((0.0 + term[256 + t]) + term[256 + 64 + t]);
        if (t == 0) totals[0] = q0, totals[1] = q1, totals[2] = q2;
    }
    __syncthreads();

    const int j = (int)k - a.burnin, half = a.draws / 2, stride = nc + 2;
    const bool keep = j >= 0 && a.betas_out && j % a.thin == 0;
    const size_t row = (size_t)c * a.kept + (size_t)(j >= 0 ? j / a.thin : 0);
    double *run_s = a.run + (size_t)c * 2 * stride, *run_q = run_s + stride;
    if (t < nc) {
        const double bt = usol[t];
        a.beta[(size_t)c * RB_STATE_LD + t] = bt;
        if (keep) a.betas_out[row * nc + t] = bt;
        if (j >= 0) {
            const double d = bt - a.shift[t];
            run_s[t] += d;
            run_q[t] += d * d;
        }
    }
    if (t == 0) {
        int att_s = 0, att_t = 0;
        const double gs = robust_gamma(a.seed, chain, k, ROB_PURPOSE_SIG_NORMAL, ROB_PURPOSE_SIG_UNIFORM, 0u, a.sig_b, a.sig_c,
                                       a.attempt_cap, att_s);
        const double gt = robust_gamma(a.seed, chain, k, ROB_PURPOSE_TAU_NORMAL, ROB_PURPOSE_TAU_UNIFORM, 0u, a.tau_b, a.tau_c,
                                       a.attempt_cap, att_t);
        const double gyy = gdiag[nc], q_bc = totals[0], q_bgb = totals[1], q_bb = totals[2];
        const double S = (gyy - 2.0 * q_bc) + q_bgb;
        const double bstar = a.b + 0.5 * (S + q_bb / tausqd);
        const bool negative = bstar < 0.0;
        const double sig = negative ? __builtin_nan("") : 1.0 / ((1.0 / bstar) * gs);
        const double btau_star = (1.0 / (2.0 * sig)) * q_bb + a.btau;
        const double tau = 1.0 / ((1.0 / btau_star) * gt);
        a.sig[c] = sig;
        a.tau[c] = tau;
        const bool capped = gs != gs || gt != gt || gyy != gyy;
        long long *cn = a.counts + (size_t)c * 4;
        const long long *gc = a.gcount + (size_t)c * 4;
        if ((negative || capped || bad) && cn[0] < 0) {
            cn[0] = k;
            cn[1] = negative ? 1 : (capped ? 2 : 3);
        }
        const long long spent = gc[0] + att_s + att_t;
        long long most = gc[2] > att_s ? gc[2] : att_s;
        most = most > att_t ? most : att_t;
        cn[2] += spent;
        cn[3] = cn[3] > most ? cn[3] : most;
        if (keep) {
            a.sig_out[row] = sig;
            a.tau_out[row] = tau;
            a.attempts_out[row] = spent;
        }
        if (j >= 0) {
            run_s[nc] += sig, run_q[nc] += sig * sig;
            run_s[nc + 1] += tau, run_q[nc + 1] += tau * tau;
        }
    }
    if (j < 0) return;
    const int segment = j + 1 == half ? 0 : (j + 1 == 2 * half ? 1 : ((a.draws & 1) && j + 1 == a.draws ? 2 : -1));
    if (segment < 0) return;
    __syncthreads();                                 // thread 0's two entries
    double *out = a.sums + ((size_t)c * RS_SEGMENTS + segment) * 2 * stride;
    for (int e = t; e < 2 * stride; e += RB_THREADS) {
        out[e] = run_s[e];
        run_s[e] = 0.0;
    }
}

static size_t robust_pass_lds(int nb) { return ((size_t)16 * nb * RB_LD + 5 * RB_ROWS + 32 * nb) * sizeof(double); }
static size_t robust_step_lds(int m) { return ((size_t)m * (m | 1) + 7 * 128 + 8) * sizeof(double); }

typedef void (*robust_pass_fn)(const RobustArgs, uint32_t, int);

static robust_pass_fn robust_pass_instance(int nb)
{
    switch (nb) {
    case 1: return robust_pass_kernel<1>;
    case 2: return robust_pass_kernel<2>;
    case 3: return robust_pass_kernel<3>;
    case 4: return robust_pass_kernel<4>;
    case 5: return robust_pass_kernel<5>;
    case 6: return robust_pass_kernel<6>;
    case 7: return robust_pass_kernel<7>;
    default: return robust_pass_kernel<8>;
    }
}

// What every entry shares: the plan (groups, blocks), the checks that need the context, and the workspaces.
struct RobustRun {
    DeviceBuffers buf;
    RobustArgs args = {};
    robust_pass_fn pass = nullptr;
    size_t pass_lds = 0, step_lds = 0, partial_doubles = 0;
    int pairs = 0;
    float us[3] = {0.f, 0.f, 0.f};                   // summed over the timed iterations
    int timed = 0;
};

static int robust_plan(fokl_ctx *ctx, RobustRun &run, int nc, int64_t n, int chains, const char *who)
{
    RobustArgs &a = run.args;
    a.nc = nc, a.m = nc + 1, a.nb = (a.m + 15) / 16, a.n = n, a.chains = chains;
    a.chunks = (n + RB_ROWS - 1) / RB_ROWS;
    a.chunks_per_group = (a.chunks + RB_MAX_GROUPS - 1) / RB_MAX_GROUPS;
    a.groups = (int)((a.chunks + a.chunks_per_group - 1) / a.chunks_per_group);
    run.pairs = a.nb * (a.nb + 1) / 2;
    run.partial_doubles = (size_t)run.pairs * 256;
    run.pass = robust_pass_instance(a.nb);
    run.pass_lds = robust_pass_lds(a.nb);
    run.step_lds = robust_step_lds(a.m);
    if (run.pass_lds > 64 * 1024) {
        int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(run.pass), run.pass_lds);
        if (rc) return rc;
    }
    if (run.step_lds > 64 * 1024) {
        int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(robust_step_kernel), run.step_lds);
        if (rc) return rc;
    }
    (void)who;
    return FOKL_OK;
}

static int robust_check_columns(fokl_ctx *ctx, int nc, const char *who)
{
    if (nc < 1 || nc > FOKL_ROBUST_MAX_COLUMNS)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + ": the model has " + std::to_string(nc) + " columns, the robust pass "
                    "holds at most " + std::to_string(FOKL_ROBUST_MAX_COLUMNS) + " ([1 | X | y] fills eight 16-column blocks)");
    return FOKL_OK;
}

// The workspaces of `chains` chains (state, partials, G, counters) and the slot list with y behind the columns.
static int robust_workspaces(fokl_ctx *ctx, RobustRun &run, const int32_t *slots, const double *weights, const int32_t *chain_ids)
{
    RobustArgs &a = run.args;
    const size_t chains = (size_t)a.chains, ld = (size_t)16 * a.nb;
    std::vector<int> all(slots, slots + a.nc);
    all.push_back(FOKL_SLOT_Y);
    std::vector<int> ids(chains);
    for (size_t c = 0; c < chains; ++c) ids[c] = chain_ids ? chain_ids[c] : (int)c;
    int *d_slots = nullptr, *d_ids = nullptr;
    double *d_w = nullptr;
    HIP_TRY(ctx, run.buf.upload(&d_slots, all.data(), all.size()));
    HIP_TRY(ctx, run.buf.upload(&d_ids, ids.data(), chains));
    if (weights) HIP_TRY(ctx, run.buf.upload(&d_w, weights, (size_t)a.n));
    a.slot_ptr = ctx->d_slot_ptr, a.slots = d_slots, a.chain_ids = d_ids, a.weights = d_w;
    HIP_TRY(ctx, run.buf.get(&a.beta, chains * RB_STATE_LD));
    HIP_TRY(ctx, run.buf.get(&a.sig, chains));
    HIP_TRY(ctx, run.buf.get(&a.tau, chains));
    HIP_TRY(ctx, run.buf.get(&a.partial, chains * a.groups * run.partial_doubles));
    HIP_TRY(ctx, run.buf.get(&a.pcount, chains * a.groups * 4));
    HIP_TRY(ctx, run.buf.get(&a.G, chains * ld * ld));
    HIP_TRY(ctx, run.buf.get(&a.gcount, chains * 4));
    HIP_TRY(ctx, hipMemsetAsync(a.beta, 0, chains * RB_STATE_LD * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.gcount, 0, chains * 4 * sizeof(long long), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the callers' blocking copies into the state come after these)
    return FOKL_OK;
}

static void robust_set_shapes(RobustArgs &a, double nu, double astar, double atau_star, int attempt_cap)
{
    a.draw = std::isinf(nu) ? 0 : 1;
    a.nu = nu;
    a.lam_b = (a.draw ? (nu + 1.0) / 2.0 : 1.0) - 1.0 / 3.0, a.lam_c = 1.0 / std::sqrt(9.0 * a.lam_b);
    a.sig_b = astar - 1.0 / 3.0, a.sig_c = 1.0 / std::sqrt(9.0 * a.sig_b);
    a.tau_b = atau_star - 1.0 / 3.0, a.tau_c = 1.0 / std::sqrt(9.0 * a.tau_b);
    a.attempt_cap = attempt_cap ? attempt_cap : RS_ATTEMPT_CAP;
}

// Queue iteration k: pass, reduce, step (what == 7), or some of them.  `ev`: four events around the three launches, or null.
static hipError_t robust_enqueue(fokl_ctx *ctx, RobustRun &run, uint32_t k, int accumulate, int what, hipEvent_t *ev)
{
    const RobustArgs &a = run.args;
    hipError_t e = hipSuccess;
    const double rows = (double)a.n * a.chains;
    if (ev) e = hipEventRecord(ev[0], ctx->stream);
    if (e == hipSuccess && (what & 1)) {
        TimedRegion timed(ctx, FOKL_K_ROBUST, 8.0 * rows * (a.m + 2) + 8.0 * a.chains * a.groups * (double)run.partial_doubles,
                          2.0 * rows * 256.0 * run.pairs);
        hipLaunchKernelGGL(run.pass, dim3(a.groups, a.chains), dim3(RB_THREADS), run.pass_lds, ctx->stream, a, k, accumulate);
        e = hipGetLastError();
    }
    if (e == hipSuccess && ev) e = hipEventRecord(ev[1], ctx->stream);
    if (e == hipSuccess && (what & 2)) {
        TimedRegion timed(ctx, FOKL_K_ROBUST, 8.0 * a.chains * (a.groups + 2) * (double)run.partial_doubles,
                          (double)a.chains * a.groups * (double)run.partial_doubles);
        hipLaunchKernelGGL(robust_reduce_kernel, dim3(run.pairs, a.chains), dim3(RB_THREADS), 0, ctx->stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess && ev) e = hipEventRecord(ev[2], ctx->stream);
    if (e == hipSuccess && (what & 4)) {
        TimedRegion timed(ctx, FOKL_K_ROBUST, 8.0 * a.chains * 256.0 * a.nb * a.nb, (double)a.chains * a.nc * a.nc * (a.nc / 3.0 + 6.0));
        hipLaunchKernelGGL(robust_step_kernel, dim3(a.chains), dim3(RB_THREADS), run.step_lds, ctx->stream, a, k);
        e = hipGetLastError();
    }
    if (e == hipSuccess && ev) e = hipEventRecord(ev[3], ctx->stream);
    return e;
}

static void robust_fill_report(fokl_ctx *ctx, const RobustRun &run, int64_t iterations, int64_t kept, int64_t attempts,
                               int64_t flagged, float total_ms)
{
    const RobustArgs &a = run.args;
    int64_t *rep = ctx->robust_report;
    rep[0] = a.groups, rep[1] = a.chains, rep[2] = (int64_t)run.partial_doubles;
    rep[3] = (int64_t)run.pass_lds, rep[4] = (int64_t)run.step_lds;
    rep[5] = a.m, rep[6] = a.nb, rep[7] = iterations, rep[8] = kept, rep[9] = attempts, rep[10] = flagged;
    for (int i = 0; i < 3; ++i) rep[11 + i] = (int64_t)std::llround((double)run.us[i]);
    rep[14] = run.timed;
    rep[15] = (int64_t)std::llround((double)total_ms * 1000.0);
}

}  // namespace fokl

extern "C" int fokl_robust_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_robust_report: null argument");
    std::memcpy(out, ctx->robust_report, sizeof ctx->robust_report);
    return FOKL_OK;
}

extern "C" int fokl_robust_pass(fokl_ctx *ctx, const int32_t *slots, int nc, const double *weights, int64_t n_weights,
                                const double *beta, double sigsqd, double nu, uint32_t seed, uint32_t chain, uint32_t iteration,
                                int attempt_cap, double *G_out, double *lam_out, int32_t *attempts_out)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_robust_pass: null context");
    std::memset(ctx->robust_report, 0, sizeof ctx->robust_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, "fokl_robust_pass: call fokl_upload first");
    if (!slots || !G_out) return fail(ctx, FOKL_ERR_ARG, "fokl_robust_pass: null argument");
    int rc = robust_check_columns(ctx, nc, "fokl_robust_pass");
    if (rc) return rc;
    if (!(nu >= 1.0))
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_pass: nu < 1 or NaN: the gamma sampler is Marsaglia-Tsang's for shapes (nu + 1) / 2 >= 1");
    const bool draws = !std::isinf(nu) && iteration > 0;
    if (draws && (!beta || !(sigsqd > 0.0) || !std::isfinite(sigsqd)))
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_pass: a drawn pass needs beta and a positive finite sigsqd");
    if (attempt_cap < 0 || attempt_cap > 1024) return fail(ctx, FOKL_ERR_ARG, "fokl_robust_pass: attempt cap in 1 .. 1024 (0: the default, 64)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = check_slots(ctx, slots, nc, "fokl_robust_pass");
    if (rc) return rc;
    const int64_t n = ctx->n;
    if (n <= 0 || n >= ((int64_t)1 << 32)) return fail(ctx, FOKL_ERR_STATE, "fokl_robust_pass: the dataset has no rows, or 2^32 and more");
    if (weights && n_weights != n)
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_pass: " + std::to_string(n_weights) + " weights for " + std::to_string(n) + " rows");

    RobustRun run;
    rc = robust_plan(ctx, run, nc, n, 1, "fokl_robust_pass");
    if (rc) return rc;
    RobustArgs &a = run.args;
    const size_t ld = (size_t)16 * a.nb;
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_ROBUST_FREE_BYTES", &free_bytes));
    const size_t want = ((size_t)a.groups * run.partial_doubles + ld * ld + (size_t)n * 3) * sizeof(double);
    if (want + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_pass: the call wants " + std::to_string(want) + " bytes on the device (rows and "
                    "partial Grams) and 64 MiB to spare, the device has " + std::to_string(free_bytes) + " free");
    const int32_t id = (int32_t)chain;
    rc = robust_workspaces(ctx, run, slots, weights, &id);
    if (rc) return rc;
    robust_set_shapes(a, nu, 1.0, 1.0, attempt_cap);
    a.seed = seed;
    if (lam_out) HIP_TRY(ctx, run.buf.get(&a.lam_out, (size_t)n));
    if (attempts_out) HIP_TRY(ctx, run.buf.get(&a.att_out, (size_t)n));
    if (draws) {
        HIP_TRY(ctx, hipMemcpy(a.beta, beta, (size_t)nc * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(a.sig, &sigsqd, sizeof(double), hipMemcpyHostToDevice));
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess) e = robust_enqueue(ctx, run, iteration, 0, 3, ev);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    float total = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&total, ev[0], ev[2]);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
        run.us[i] = ms * 1000.f;
    }
    run.timed = 1;
    for (int i = 0; i < 4; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    std::vector<double> full(ld * ld);
    long long gc[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(full.data(), a.G, ld * ld * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(gc, a.gcount, sizeof gc, hipMemcpyDeviceToHost);
    if (e == hipSuccess && lam_out) e = hipMemcpy(lam_out, a.lam_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && attempts_out) e = hipMemcpy(attempts_out, a.att_out, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_robust_pass: ") + hipGetErrorString(e));
    for (int i = 0; i < a.m; ++i)
        for (int j = 0; j < a.m; ++j) G_out[(size_t)i * a.m + j] = full[(size_t)i * ld + j];
    robust_fill_report(ctx, run, 1, 0, gc[0], gc[1] > 0, total);
    return FOKL_OK;
}

extern "C" int fokl_robust_step(fokl_ctx *ctx, int nc, const double *G, double sigsqd, double tausqd, double astar,
                                double atau_star, double b, double btau, uint32_t seed, uint32_t chain, uint32_t iteration,
                                int attempt_cap, double *beta_out, double *state_out, int64_t *counts_out)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_robust_step: null context");
    std::memset(ctx->robust_report, 0, sizeof ctx->robust_report);
    if (!G || !beta_out || !state_out || !counts_out) return fail(ctx, FOKL_ERR_ARG, "fokl_robust_step: null argument");
    int rc = robust_check_columns(ctx, nc, "fokl_robust_step");
    if (rc) return rc;
    if (!(astar >= 1.0) || !(atau_star >= 1.0))
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_step: the gamma sampler is Marsaglia-Tsang's for shapes >= 1 (astar and "
                    "atau + P / 2 must be at least 1)");
    if (attempt_cap < 0 || attempt_cap > 1024) return fail(ctx, FOKL_ERR_ARG, "fokl_robust_step: attempt cap in 1 .. 1024 (0: the default, 64)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RobustRun run;
    rc = robust_plan(ctx, run, nc, 1, 1, "fokl_robust_step");
    if (rc) return rc;
    RobustArgs &a = run.args;
    const size_t ld = (size_t)16 * a.nb, stride = (size_t)nc + 2;
    std::vector<double> full(ld * ld, 0.0);
    for (int i = 0; i < a.m; ++i)
        for (int j = 0; j < a.m; ++j) full[(size_t)i * ld + j] = G[(size_t)i * a.m + j];
    const int id = (int)chain;
    const long long counts0[4] = {-1, 0, 0, 0}, zeros[4] = {0, 0, 0, 0};
    std::vector<double> shift(nc, 0.0);
    int *d_ids = nullptr;
    double *d_shift = nullptr;
    HIP_TRY(ctx, run.buf.upload(&d_ids, &id, 1));
    HIP_TRY(ctx, run.buf.upload(&d_shift, shift.data(), (size_t)nc));
    HIP_TRY(ctx, run.buf.upload(&a.G, full.data(), ld * ld));
    HIP_TRY(ctx, run.buf.upload(&a.sig, &sigsqd, 1));
    HIP_TRY(ctx, run.buf.upload(&a.tau, &tausqd, 1));
    HIP_TRY(ctx, run.buf.upload(&a.counts, counts0, 4));
    HIP_TRY(ctx, run.buf.upload(&a.gcount, zeros, 4));
    HIP_TRY(ctx, run.buf.get(&a.beta, (size_t)RB_STATE_LD));
    HIP_TRY(ctx, run.buf.get(&a.run, 2 * stride));
    HIP_TRY(ctx, run.buf.get(&a.sums, (size_t)RS_SEGMENTS * 2 * stride));
    HIP_TRY(ctx, hipMemsetAsync(a.run, 0, 2 * stride * sizeof(double), ctx->stream));
    a.chain_ids = d_ids, a.shift = d_shift;
    robust_set_shapes(a, INFINITY, astar, atau_star, attempt_cap);
    a.seed = seed, a.b = b, a.btau = btau;
    a.burnin = (int)std::min<uint32_t>(iteration, (uint32_t)INT_MAX - 1) + 1;   // the step's iteration is before the rows: nothing is kept
    a.draws = 1, a.thin = 1, a.kept = 1;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess) e = robust_enqueue(ctx, run, iteration, 0, 4, ev);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[2], ev[3]);
    run.us[2] = ms * 1000.f, run.timed = 1;
    for (int i = 0; i < 4; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    long long cn[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(beta_out, a.beta, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&state_out[0], a.sig, sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&state_out[1], a.tau, sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cn, a.counts, sizeof cn, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_robust_step: ") + hipGetErrorString(e));
    for (int i = 0; i < 4; ++i) counts_out[i] = cn[i];
    a.groups = 0, run.partial_doubles = 0, run.pass_lds = 0;
    robust_fill_report(ctx, run, 1, 0, cn[2], cn[0] >= 0, ms);
    return FOKL_OK;
}

extern "C" int fokl_robust_chains(fokl_ctx *ctx, const int32_t *slots, int nc, const double *weights, int64_t n_weights, double nu,
                                  double astar, double atau_star, double b, double btau, const double *shift, int chains,
                                  const int32_t *chain_ids, const double *sigsqd0, const double *tausqd0, int burnin, int draws,
                                  int thin, uint32_t seed, int attempt_cap, double *betas_out, double *sig_out, double *tau_out,
                                  int64_t *attempts_out, double *sums_out, int64_t *counts_out, double *lam_sum_out)
{
    using namespace fokl;
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, "fokl_robust_chains: null context");
    std::memset(ctx->robust_report, 0, sizeof ctx->robust_report);
    if (!ctx->have_data) return fail(ctx, FOKL_ERR_STATE, "fokl_robust_chains: call fokl_upload first");
    if (!slots || !shift || !sigsqd0 || !tausqd0 || !sums_out || !counts_out)
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: null argument");
    int rc = robust_check_columns(ctx, nc, "fokl_robust_chains");
    if (rc) return rc;
    if (!(nu >= 1.0))
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: nu < 1 or NaN: the gamma sampler is Marsaglia-Tsang's for shapes (nu + 1) / 2 >= 1");
    if (!(astar >= 1.0) || !(atau_star >= 1.0))
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: the gamma sampler is Marsaglia-Tsang's for shapes >= 1 (astar and "
                    "atau + P / 2 must be at least 1)");
    if (chains < 1 || chains > 65535 || burnin < 0 || draws < 1 || thin < 1 || (int64_t)burnin + draws > (1 << 30))
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: chains in 1 .. 65 535, burnin >= 0, draws >= 1, thin >= 1, "
                    "burnin + draws <= 2^30");
    if (attempt_cap < 0 || attempt_cap > 1024) return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: attempt cap in 1 .. 1024 (0: the default, 64)");
    const bool rows = betas_out != nullptr;
    if (rows != (sig_out != nullptr) || rows != (tau_out != nullptr) || rows != (attempts_out != nullptr))
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: rows are kept (betas, sigsqd, tausqd, attempts) or not at all");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = check_slots(ctx, slots, nc, "fokl_robust_chains");
    if (rc) return rc;
    const int64_t n = ctx->n;
    if (n <= 0 || n >= ((int64_t)1 << 32)) return fail(ctx, FOKL_ERR_STATE, "fokl_robust_chains: the dataset has no rows, or 2^32 and more");
    if (weights && n_weights != n)
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: " + std::to_string(n_weights) + " weights for " + std::to_string(n) + " rows");

    RobustRun run;
    rc = robust_plan(ctx, run, nc, n, chains, "fokl_robust_chains");
    if (rc) return rc;
    RobustArgs &a = run.args;
    const int kept = (draws + thin - 1) / thin;
    const size_t ld = (size_t)16 * a.nb, stride = (size_t)nc + 2, n_rows = rows ? (size_t)chains * kept : 0;
    const size_t n_sums = (size_t)chains * RS_SEGMENTS * 2 * stride;
    const size_t row_bytes = n_rows * ((size_t)nc + 3) * sizeof(double);
    const size_t lam_bytes = lam_sum_out ? (size_t)chains * n * sizeof(double) : 0;
    const size_t partial_bytes = (size_t)chains * a.groups * run.partial_doubles * sizeof(double);
    const size_t other = (size_t)chains * (ld * ld + RB_STATE_LD + 8 * stride + 64) * sizeof(double) + (size_t)n * sizeof(double);
    size_t free_bytes = 0;
    HIP_TRY(ctx, capped_free_bytes("FOKL_ROBUST_FREE_BYTES", &free_bytes));
    if (row_bytes + lam_bytes + partial_bytes + other + (64 << 20) > free_bytes)
        return fail(ctx, FOKL_ERR_ARG, "fokl_robust_chains: the call wants " + std::to_string(row_bytes) + " bytes of rows (chains x "
                    "kept x (P + 4) x 8), " + std::to_string(lam_bytes) + " of row weights (chains x rows x 8) and " +
                    std::to_string(partial_bytes) + " of partial Grams on the device and 64 MiB to spare, the device has " +
                    std::to_string(free_bytes) + " free (thin, keep no rows, or fewer chains)");

    rc = robust_workspaces(ctx, run, slots, weights, chain_ids);
    if (rc) return rc;
    robust_set_shapes(a, nu, astar, atau_star, attempt_cap);
    a.seed = seed, a.b = b, a.btau = btau, a.burnin = burnin, a.draws = draws, a.thin = thin, a.kept = kept;
    double *d_shift = nullptr;
    HIP_TRY(ctx, run.buf.upload(&d_shift, shift, (size_t)nc));
    a.shift = d_shift;
    HIP_TRY(ctx, hipMemcpy(a.sig, sigsqd0, (size_t)chains * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(a.tau, tausqd0, (size_t)chains * sizeof(double), hipMemcpyHostToDevice));
    std::vector<long long> counts0((size_t)chains * 4, 0);
    for (int c = 0; c < chains; ++c) counts0[(size_t)c * 4] = -1;
    HIP_TRY(ctx, run.buf.upload(&a.counts, counts0.data(), counts0.size()));
    HIP_TRY(ctx, run.buf.get(&a.run, (size_t)chains * 2 * stride));
    HIP_TRY(ctx, run.buf.get(&a.sums, n_sums));
    HIP_TRY(ctx, hipMemsetAsync(a.run, 0, (size_t)chains * 2 * stride * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.sums, 0, n_sums * sizeof(double), ctx->stream));   // (a segment without iterations stays 0)
    if (lam_sum_out && a.draw) {
        HIP_TRY(ctx, run.buf.get(&a.lam_sum, (size_t)chains * n));
        HIP_TRY(ctx, hipMemsetAsync(a.lam_sum, 0, lam_bytes, ctx->stream));
    }
    if (rows) {
        HIP_TRY(ctx, run.buf.get(&a.betas_out, n_rows * (size_t)nc));
        HIP_TRY(ctx, run.buf.get(&a.sig_out, n_rows));
        HIP_TRY(ctx, run.buf.get(&a.tau_out, n_rows));
        HIP_TRY(ctx, run.buf.get(&a.attempts_out, n_rows));
    }

    const int total = burnin + draws, timed = std::min(total, RB_TIMED);
    std::vector<hipEvent_t> ev((size_t)timed * 4 + 2, nullptr);
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < ev.size() && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    hipEvent_t *whole = ev.data() + (size_t)timed * 4;
    if (e == hipSuccess) e = hipEventRecord(whole[0], ctx->stream);
    for (int k = 0; k < total && e == hipSuccess; ++k)
        e = robust_enqueue(ctx, run, (uint32_t)k, k >= burnin, a.draw || k == 0 ? 7 : 4,
                           k >= total - timed ? ev.data() + (size_t)(k - (total - timed)) * 4 : nullptr);
    if (e == hipSuccess) e = hipEventRecord(whole[1], ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    float total_ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&total_ms, whole[0], whole[1]);
    for (int i = 0; i < timed && e == hipSuccess; ++i)
        for (int s = 0; s < 3 && e == hipSuccess; ++s) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, ev[(size_t)i * 4 + s], ev[(size_t)i * 4 + s + 1]);
            run.us[s] += ms * 1000.f;
        }
    run.timed = timed;
    for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    std::vector<long long> cn((size_t)chains * 4, 0);
    if (e == hipSuccess) e = hipMemcpy(sums_out, a.sums, n_sums * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cn.data(), a.counts, cn.size() * sizeof(long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess && lam_sum_out && a.draw) e = hipMemcpy(lam_sum_out, a.lam_sum, lam_bytes, hipMemcpyDeviceToHost);
    if (lam_sum_out && !a.draw) std::fill(lam_sum_out, lam_sum_out + (size_t)chains * n, (double)draws);   // lam = 1, no pass after the first
    if (e == hipSuccess && rows) e = hipMemcpy(betas_out, a.betas_out, n_rows * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows) e = hipMemcpy(sig_out, a.sig_out, n_rows * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows) e = hipMemcpy(tau_out, a.tau_out, n_rows * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows) e = hipMemcpy(attempts_out, a.attempts_out, n_rows * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, FOKL_ERR_HIP, std::string("fokl_robust_chains: ") + hipGetErrorString(e));
    int64_t attempts = 0, flagged = 0;
    for (int c = 0; c < chains; ++c) {
        for (int i = 0; i < 4; ++i) counts_out[(size_t)c * 4 + i] = cn[(size_t)c * 4 + i];
        flagged += cn[(size_t)c * 4] >= 0;
        attempts += cn[(size_t)c * 4 + 2];
    }
    robust_fill_report(ctx, run, total, kept, attempts, flagged, total_ms);
    return FOKL_OK;
}

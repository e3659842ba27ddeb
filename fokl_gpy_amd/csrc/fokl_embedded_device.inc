// Embedded GPs (fokl_gpy_amd/embedded.py): K BSS-ANOVA GPs inside a traced user equation, sampled by Hamiltonian Monte
// Carlo.  Textually included by fokl_hip.hip.
//
// hmc_chain_kernel: ONE WORKGROUP PER CHAIN, the whole chain -- step search, `draws` transitions, the 50-draw step
// adaptation and the one mass update -- in one launch.  No communication between workgroups, no grid-wide barrier, every
// loop bounded by an argument or a constant; a chain's numbers depend on (seed, chain) only, never on the grid.
//
// A potential-and-gradient pass (emb_pass) at the parameters in LDS:
//   A. the threads stride the rows.  g_k = X beta_k: the basis columns are slots of `ld` fp64 (coalesced over the rows),
//      beta is read from LDS (one address per wave: a broadcast), the K accumulators are a statically indexed register
//      array.  The tape runs forward, then backward, over value / adjoint slots laid out [slot][thread] in LDS: the tape
//      is uniform over the workgroup, so the opcode switch does not diverge, and no register array is indexed by a
//      runtime slot.  Columns and constants are read where an operation uses them.  e = y - r, the thread's sum of e^2,
//      and w_k = e dr/dg_k written to the chain's scratch rows W[k][i] (read back by the same thread only).
//   B. dU/dbeta_k[t] = -exp(-s) sum_i X[i][t] w_k[i] + beta_k[t] / 1000: column by column, K accumulators per thread, a
//      wave reduction by shuffles, the per-wave partials in LDS and one fixed-order sum over the waves.
// The statement of the whole algorithm is embedded.full_sample_host; the kernel is tested against it.

#include "fokl_philox.h"

namespace fokl {

constexpr int EMB_MAX_GPS = 8;
constexpr int EMB_MAX_COLS = 16;
constexpr int EMB_MAX_OPS = 32;
constexpr int EMB_MAX_CONSTS = 64;
constexpr int EMB_MAX_PARAMS = 257;
constexpr int64_t EMB_MAX_VALUES = 4194304;        // N (T + 1): 32 MB of basis values, what the last-level cache keeps
constexpr int EMB_MAX_CHAINS = 4096;
constexpr int EMB_MAX_DRAWS = 1000000;
constexpr int EMB_MAX_LEAPFROG = 1000;
constexpr int EMB_SEARCH_CAP = 60;                 // halvings, and doublings / halvings, of the step search
constexpr int EMB_WINDOW = 50;                     // draws per step-size window
constexpr int EMB_MASS_DRAW = 500;                 // the mass update runs once, after this draw ...
constexpr int EMB_MASS_STATES = 100;               // ... from the last 100 states, if at least ...
constexpr int EMB_MASS_MOVED = 5;                  // ... 5 of those draws were accepted
constexpr size_t EMB_LDS_BUDGET = 160 * 1024;

enum { EMB_ADD = 0, EMB_SUB, EMB_MUL, EMB_DIV, EMB_NEG, EMB_EXP, EMB_LOG, EMB_SQRT, EMB_SQUARE, EMB_RECIP, EMB_POWC,
       EMB_OP_COUNT };
enum { EMB_KIND_SLOT = 0, EMB_KIND_COLUMN = 1, EMB_KIND_CONST = 2 };
enum { EMB_STATUS_OK = 0, EMB_STATUS_NO_STEP = 1 };

struct EmbProblem {
    int n_gps, n_coef, n_params;       // K, P = T + 1, D = K P + 1
    int n_ops, n_consts, n_cols, result;
    int draws, leapfrog, adapt, n_windows;
    uint32_t seed;
    int64_t n, ld;
    double eps0;
};

struct EmbLds {
    double *q, *grad, *qn, *pn, *gn, *inv_mass, *red, *consts, *val, *adj;
    int *ops;
};

__device__ __forceinline__ double emb_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum of one value per thread, the same in every thread and every run: waves in order
template <int THREADS>
__device__ __forceinline__ double emb_block_sum(double v, double *red)
{
    v = emb_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) total += red[w];
    return total;
}

__device__ __forceinline__ double emb_operand(int code, const double *val, const double *consts, const double *cols,
                                              int64_t ld, int64_t i, int threads)
{
    const int kind = code >> 8, idx = code & 255;
    if (kind == EMB_KIND_SLOT) return val[idx * threads + threadIdx.x];
    if (kind == EMB_KIND_COLUMN) return cols[(size_t)idx * ld + i];
    return consts[idx];
}

// U and dU/dq at the parameters `at` (LDS) -> returns U, the gradient in `grad` (LDS).  Every thread returns the same U.
template <int THREADS>
__device__ double emb_pass(const EmbProblem &p, const EmbLds &s, const double *at, double *grad,
                           const double *const *__restrict__ xcols, const double *__restrict__ y,
                           const double *__restrict__ cols, double *__restrict__ w)
{
    const int K = p.n_gps, P = p.n_coef, n_slots = K + p.n_ops, tid = threadIdx.x;
    double *val = s.val, *adj = s.adj;
    __syncthreads();                                   // `at` is complete; the previous pass's readers are done
    double sse = 0.0;
    for (int64_t i = tid; i < p.n; i += THREADS) {
        double g[EMB_MAX_GPS];
#pragma unroll
        for (int k = 0; k < EMB_MAX_GPS; ++k) g[k] = 0.0;
        for (int t = 0; t < P; ++t) {
            const double x = xcols[t][i];
#pragma unroll
            for (int k = 0; k < EMB_MAX_GPS; ++k)
                if (k < K) g[k] += x * at[k * P + t];
        }
#pragma unroll
        for (int k = 0; k < EMB_MAX_GPS; ++k)
            if (k < K) val[k * THREADS + tid] = g[k];
        for (int o = 0; o < p.n_ops; ++o) {
            const int code = s.ops[3 * o], ca = s.ops[3 * o + 1], cb = s.ops[3 * o + 2];
            const double a = emb_operand(ca, val, s.consts, cols, p.ld, i, THREADS);
            double r;
            if (code <= EMB_DIV) {
                const double b = emb_operand(cb, val, s.consts, cols, p.ld, i, THREADS);
                r = code == EMB_ADD ? a + b : code == EMB_SUB ? a - b : code == EMB_MUL ? a * b : a / b;
            } else if (code == EMB_NEG) r = -a;
            else if (code == EMB_EXP) r = exp(a);
            else if (code == EMB_LOG) r = log(a);
            else if (code == EMB_SQRT) r = sqrt(a);
            else if (code == EMB_SQUARE) r = a * a;
            else if (code == EMB_RECIP) r = 1.0 / a;
            else r = pow(a, s.consts[cb & 255]);
            val[(K + o) * THREADS + tid] = r;
        }
        for (int v = 0; v < n_slots; ++v) adj[v * THREADS + tid] = 0.0;
        adj[p.result * THREADS + tid] = 1.0;
        for (int o = p.n_ops - 1; o >= 0; --o) {
            const double bar = adj[(K + o) * THREADS + tid];
            const int code = s.ops[3 * o], ca = s.ops[3 * o + 1], cb = s.ops[3 * o + 2];
            const bool slot_a = (ca >> 8) == EMB_KIND_SLOT, slot_b = code <= EMB_DIV && (cb >> 8) == EMB_KIND_SLOT;
            if (!slot_a && !slot_b) continue;
            const double r = val[(K + o) * THREADS + tid];
            double da = 1.0, db = 1.0;
            if (code <= EMB_DIV) {
                if (code == EMB_SUB) db = -1.0;
                else if (code == EMB_MUL) {
                    da = emb_operand(cb, val, s.consts, cols, p.ld, i, THREADS);
                    db = emb_operand(ca, val, s.consts, cols, p.ld, i, THREADS);
                } else if (code == EMB_DIV) {
                    const double b = emb_operand(cb, val, s.consts, cols, p.ld, i, THREADS);
                    da = 1.0 / b;
                    db = -r / b;
                }
            } else {
                const double a = emb_operand(ca, val, s.consts, cols, p.ld, i, THREADS);
                if (code == EMB_NEG) da = -1.0;
                else if (code == EMB_EXP) da = r;
                else if (code == EMB_LOG) da = 1.0 / a;
                else if (code == EMB_SQRT) da = 0.5 / r;
                else if (code == EMB_SQUARE) da = 2.0 * a;
                else if (code == EMB_RECIP) da = -(r * r);
                else {
                    const double c = s.consts[cb & 255];
                    da = c * pow(a, c - 1.0);
                }
            }
            if (slot_a) adj[(ca & 255) * THREADS + tid] += bar * da;
            if (slot_b) adj[(cb & 255) * THREADS + tid] += bar * db;
        }
        const double e = y[i] - val[p.result * THREADS + tid];
        sse += e * e;
#pragma unroll
        for (int k = 0; k < EMB_MAX_GPS; ++k)
            if (k < K) w[(size_t)k * p.ld + i] = e * adj[k * THREADS + tid];
    }
    // B: the columns' dot products with w_k; partials per wave at red[THREADS / 64 + j * (THREADS / 64) + wave]
    constexpr int WAVES = THREADS / 64;
    double *part = s.red + WAVES;
    const int wave = tid >> 6, lane = tid & 63;
    for (int t = 0; t < P; ++t) {
        double acc[EMB_MAX_GPS];
#pragma unroll
        for (int k = 0; k < EMB_MAX_GPS; ++k) acc[k] = 0.0;
        const double *xc = xcols[t];
        for (int64_t i = tid; i < p.n; i += THREADS) {
            const double x = xc[i];
#pragma unroll
            for (int k = 0; k < EMB_MAX_GPS; ++k)
                if (k < K) acc[k] += x * w[(size_t)k * p.ld + i];
        }
#pragma unroll
        for (int k = 0; k < EMB_MAX_GPS; ++k)
            if (k < K) {
                const double v = emb_wave_sum(acc[k]);
                if (lane == 0) part[(k * P + t) * WAVES + wave] = v;
            }
    }
    {
        const double v = emb_wave_sum(sse);
        if (lane == 0) part[(K * P) * WAVES + wave] = v;
    }
    __syncthreads();
    double total_sse = 0.0;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) total_sse += part[(K * P) * WAVES + wv];
    const double sln = at[K * P], prec = exp(-sln);
    double norm2 = 0.0;
    for (int j = 0; j < K * P; ++j) norm2 += at[j] * at[j];           // D - 1 <= 256 LDS broadcasts, the same in every thread
    for (int j = tid; j < K * P; j += THREADS) {
        double dot = 0.0;
#pragma unroll
        for (int wv = 0; wv < WAVES; ++wv) dot += part[j * WAVES + wv];
        grad[j] = -prec * dot + at[j] / 1000.0;
    }
    if (tid == 0) grad[K * P] = 0.5 * (double)p.n - 0.5 * prec * total_sse;
    const double U = 0.5 * (double)p.n * (1.8378770664093453 + sln) + 0.5 * prec * total_sse + norm2 / 2000.0 +
                     0.5 * (double)(p.n_params - 1) * 8.745632345391483;
    __syncthreads();                                   // grad is complete; `part` may be written again
    return U;
}

// sum_j v_j^2 inv_mass_j / 2 over the parameters, uniform
template <int THREADS>
__device__ __forceinline__ double emb_kinetic(const EmbProblem &p, const EmbLds &s, const double *v)
{
    double k = 0.0;
    for (int j = threadIdx.x; j < p.n_params; j += THREADS) k += v[j] * v[j] * s.inv_mass[j];
    return 0.5 * emb_block_sum<THREADS>(k, s.red);
}

// sum_j |g_j|: finite exactly when the gradient is usable
template <int THREADS>
__device__ __forceinline__ double emb_abs_sum(const EmbProblem &p, const EmbLds &s, const double *v)
{
    double k = 0.0;
    for (int j = threadIdx.x; j < p.n_params; j += THREADS) k += fabs(v[j]);
    return emb_block_sum<THREADS>(k, s.red);
}

// find_reasonable_epsilon at the state q (potential U, gradient s.grad) -> the step, or 0 when none is found
template <int THREADS>
__device__ double emb_step_search(const EmbProblem &p, const EmbLds &s, double U, uint32_t chain, uint32_t draw,
                                  const double *const *xcols, const double *y, const double *cols, double *w)
{
    const int tid = threadIdx.x, D = p.n_params;
    double *r0 = s.gn + EMB_MAX_PARAMS;                // a row of its own behind gn
    for (int j = tid; j < D; j += THREADS) r0[j] = emb_normal(p.seed, chain, draw, EMB_PURPOSE_SEARCH, j) / sqrt(s.inv_mass[j]);
    __syncthreads();
    const double K0 = emb_kinetic<THREADS>(p, s, r0);
    // one loop for both phases: 0 halves the step until the trial point is finite (at most 60 times), 1 doubles or halves
    // it until the acceptance probability crosses 1/2 (at most 60 times)
    double eps = 1.0, a = 1.0;
    int phase = 0, halvings = 0, moves = 0;
    for (int it = 0; it < 2 * EMB_SEARCH_CAP + 2; ++it) {
        for (int j = tid; j < D; j += THREADS) {
            const double half = r0[j] - 0.5 * eps * s.grad[j];
            s.pn[j] = half;
            s.qn[j] = s.q[j] + eps * s.inv_mass[j] * half;
        }
        const double Un = emb_pass<THREADS>(p, s, s.qn, s.gn, xcols, y, cols, w);
        for (int j = tid; j < D; j += THREADS) s.pn[j] -= 0.5 * eps * s.gn[j];
        const double K1 = emb_kinetic<THREADS>(p, s, s.pn);
        const double gsum = emb_abs_sum<THREADS>(p, s, s.gn);
        const bool finite = isfinite(Un) && isfinite(gsum);
        const double log_accept = U - Un - (K1 - K0);
        if (phase == 0) {
            if (!finite) {
                if (++halvings > EMB_SEARCH_CAP) return 0.0;
                eps *= 0.5;
                continue;
            }
            a = log_accept > -0.6931471805599453 ? 1.0 : -1.0;
            eps *= 0.5;
            phase = 1;
        }
        if (!(a * log_accept > -a * 0.6931471805599453) || moves == EMB_SEARCH_CAP) break;
        ++moves;
        eps = a > 0.0 ? eps * 2.0 : eps * 0.5;
    }
    return isfinite(eps) && eps > 0.0 ? eps : 0.0;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void hmc_chain_kernel(EmbProblem p, const double *const *__restrict__ xcols,
                                                            const double *__restrict__ y, const double *__restrict__ cols,
                                                            const int *__restrict__ ops, const double *__restrict__ consts,
                                                            const double *__restrict__ q0, double *__restrict__ wall,
                                                            double *__restrict__ states, double *__restrict__ Uout,
                                                            int *__restrict__ accepted, double *__restrict__ eps_hist,
                                                            double *__restrict__ inv_mass_out, double *__restrict__ eps_final,
                                                            int *__restrict__ status, double *__restrict__ grad0,
                                                            double *__restrict__ proposal)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int WAVES = THREADS / 64;
    const int tid = threadIdx.x, D = p.n_params, n_slots = p.n_gps + p.n_ops;
    const uint32_t chain = blockIdx.x;
    EmbLds s;
    s.q = lds;
    s.grad = s.q + EMB_MAX_PARAMS;
    s.qn = s.grad + EMB_MAX_PARAMS;
    s.pn = s.qn + EMB_MAX_PARAMS;
    s.gn = s.pn + EMB_MAX_PARAMS;                      // two rows: gn, and the step search's momentum
    s.inv_mass = s.gn + 2 * EMB_MAX_PARAMS;
    s.red = s.inv_mass + EMB_MAX_PARAMS;               // WAVES + EMB_MAX_PARAMS * WAVES
    s.consts = s.red + WAVES + EMB_MAX_PARAMS * WAVES;
    s.val = s.consts + EMB_MAX_CONSTS;
    s.adj = s.val + (size_t)n_slots * THREADS;
    s.ops = reinterpret_cast<int *>(s.adj + (size_t)n_slots * THREADS);
    for (int j = tid; j < 3 * p.n_ops; j += THREADS) s.ops[j] = ops[j];
    for (int j = tid; j < p.n_consts; j += THREADS) s.consts[j] = consts[j];
    for (int j = tid; j < D; j += THREADS) {
        s.q[j] = q0 ? q0[(size_t)chain * D + j] : 1.0;
        s.inv_mass[j] = 1.0;
    }
    double *w = wall + (size_t)chain * p.n_gps * p.ld;
    double *st = states + (size_t)chain * (p.draws + 1) * D;
    double *Uc = Uout + (size_t)chain * (p.draws + 1);
    int *ac = accepted + (size_t)chain * (p.draws + 1);

    double U = emb_pass<THREADS>(p, s, s.q, s.grad, xcols, y, cols, w);
    for (int j = tid; j < D; j += THREADS) {
        st[j] = s.q[j];
        if (grad0) grad0[(size_t)chain * D + j] = s.grad[j];
    }
    if (tid == 0) {
        Uc[0] = U;
        ac[0] = 0;
    }
    int mass_updated = 0;
    double eps = p.eps0;
    if (!(eps > 0.0)) eps = emb_step_search<THREADS>(p, s, U, chain, 0u, xcols, y, cols, w);
    bool alive = eps > 0.0;
    int window = 0, moved = 0;
    for (int d = 1; d <= p.draws && alive; ++d) {
        for (int j = tid; j < D; j += THREADS) {
            const double mom = emb_normal(p.seed, chain, (uint32_t)d, EMB_PURPOSE_MOMENTUM, j) / sqrt(s.inv_mass[j]);
            s.gn[EMB_MAX_PARAMS + j] = mom;
            s.pn[j] = mom - 0.5 * eps * s.grad[j];
            s.qn[j] = s.q[j];
        }
        __syncthreads();
        const double K0 = emb_kinetic<THREADS>(p, s, s.gn + EMB_MAX_PARAMS);
        double Un = U;
        for (int l = 0; l < p.leapfrog; ++l) {
            for (int j = tid; j < D; j += THREADS) s.qn[j] += eps * s.inv_mass[j] * s.pn[j];
            Un = emb_pass<THREADS>(p, s, s.qn, s.gn, xcols, y, cols, w);
            const double scale = l == p.leapfrog - 1 ? 0.5 * eps : eps;
            for (int j = tid; j < D; j += THREADS) s.pn[j] -= scale * s.gn[j];
        }
        __syncthreads();
        const double K1 = emb_kinetic<THREADS>(p, s, s.pn);
        const double u = emb_uniform(p.seed, chain, (uint32_t)d, EMB_PURPOSE_ACCEPT, 0u);
        const bool accept = u < exp(U - Un + K0 - K1);
        if (proposal && d == p.draws)
            for (int j = tid; j < D + 1; j += THREADS) proposal[(size_t)chain * (D + 1) + j] = j < D ? s.qn[j] : Un;
        if (accept) {
            U = Un;
            for (int j = tid; j < D; j += THREADS) {
                s.q[j] = s.qn[j];
                s.grad[j] = s.gn[j];
            }
        }
        for (int j = tid; j < D; j += THREADS) st[(size_t)d * D + j] = s.q[j];      // (thread j reads back its own writes below)
        if (tid == 0) {
            Uc[d] = U;
            ac[d] = accept ? 1 : 0;
        }
        window += accept ? 1 : 0;
        if (d > EMB_MASS_DRAW - EMB_MASS_STATES && d <= EMB_MASS_DRAW) moved += accept ? 1 : 0;
        if (d % EMB_WINDOW == 0) {
            if (p.adapt) {
                if (window < 15) eps *= 0.5;
                else if (window < 30) eps *= 0.8;
                else if (window > 45) eps *= 1.5;
                else if (window > 30) eps *= 1.2;
            }
            window = 0;
            if (p.adapt && d == EMB_MASS_DRAW && moved >= EMB_MASS_MOVED) {
                // per-parameter variance of the last 100 states (n - 1 in the denominator); used only if every one is
                // finite and positive
                double bad = 0.0;
                for (int j = tid; j < D; j += THREADS) {
                    double mean = 0.0, var = 0.0;
                    for (int r = d - EMB_MASS_STATES + 1; r <= d; ++r) mean += st[(size_t)r * D + j];
                    mean /= (double)EMB_MASS_STATES;
                    for (int r = d - EMB_MASS_STATES + 1; r <= d; ++r) {
                        const double c = st[(size_t)r * D + j] - mean;
                        var += c * c;
                    }
                    var /= (double)(EMB_MASS_STATES - 1);
                    s.pn[j] = var;
                    if (!(isfinite(var) && var > 0.0)) bad += 1.0;
                }
                __syncthreads();
                if (emb_block_sum<THREADS>(bad, s.red) == 0.0) {
                    for (int j = tid; j < D; j += THREADS) s.inv_mass[j] = s.pn[j];
                    __syncthreads();
                    mass_updated = 1;
                    eps = emb_step_search<THREADS>(p, s, U, chain, (uint32_t)d, xcols, y, cols, w);
                    alive = eps > 0.0;
                }
            }
            if (tid == 0) eps_hist[(size_t)chain * p.n_windows + d / EMB_WINDOW - 1] = alive ? eps : __builtin_nan("");
            if (!alive) {
                // the rest of the chain is not sampled, and neither is its last proposal
                const double nan = __builtin_nan("");
                if (proposal)
                    for (int j = tid; j < D + 1; j += THREADS) proposal[(size_t)chain * (D + 1) + j] = nan;
                for (int r = d + 1; r <= p.draws; ++r) {
                    for (int j = tid; j < D; j += THREADS) st[(size_t)r * D + j] = nan;
                    if (tid == 0) {
                        Uc[r] = nan;
                        ac[r] = 0;
                    }
                }
                for (int r = d / EMB_WINDOW + tid; r < p.n_windows; r += THREADS) eps_hist[(size_t)chain * p.n_windows + r] = nan;
            }
        }
    }
    if (!alive && !mass_updated) {
        // no step at the start: nothing after the start state is sampled
        const double nan = __builtin_nan("");
        for (int r = 1; r <= p.draws; ++r) {
            for (int j = tid; j < D; j += THREADS) st[(size_t)r * D + j] = nan;
            if (tid == 0) {
                Uc[r] = nan;
                ac[r] = 0;
            }
        }
        for (int r = tid; r < p.n_windows; r += THREADS) eps_hist[(size_t)chain * p.n_windows + r] = nan;
        if (proposal)
            for (int j = tid; j < D + 1; j += THREADS) proposal[(size_t)chain * (D + 1) + j] = nan;
    }
    for (int j = tid; j < D; j += THREADS) inv_mass_out[(size_t)chain * D + j] = s.inv_mass[j];
    if (tid == 0) {
        eps_final[chain] = alive ? eps : __builtin_nan("");
        status[2 * chain] = alive ? EMB_STATUS_OK : EMB_STATUS_NO_STEP;
        status[2 * chain + 1] = mass_updated;
    }
}

static size_t emb_lds_bytes(int n_slots, int n_ops, int threads)
{
    const size_t waves = threads / 64;
    const size_t doubles = (size_t)7 * EMB_MAX_PARAMS + waves + (size_t)EMB_MAX_PARAMS * waves + EMB_MAX_CONSTS +
                           (size_t)2 * n_slots * threads;
    return doubles * sizeof(double) + (size_t)3 * std::max(n_ops, 1) * sizeof(int);
}

// the launch plan of a tape: 256 threads where values and adjoints fit beside the rest, 128 for the largest tapes
static size_t emb_plan(int n_gps, int n_ops, int *threads)
{
    const int n_slots = n_gps + n_ops;
    *threads = emb_lds_bytes(n_slots, n_ops, 256) <= EMB_LDS_BUDGET ? 256 : 128;
    return emb_lds_bytes(n_slots, n_ops, *threads);
}

// "" or why the tape cannot run
static std::string emb_tape_refusal(int n_gps, int n_cols, int n_ops, const int32_t *ops, int n_consts, int result)
{
    auto operand = [&](int code, int o, const char *which) -> std::string {
        const int kind = code >> 8, idx = code & 255;
        const std::string at = "operation " + std::to_string(o) + ": " + which + " operand ";
        if (code < 0 || kind > EMB_KIND_CONST) return at + "of an unknown kind";
        if (kind == EMB_KIND_SLOT && idx >= n_gps + o) return at + "is a value that is not computed before it";
        if (kind == EMB_KIND_COLUMN && idx >= n_cols) return at + "names column " + std::to_string(idx) + " of " + std::to_string(n_cols);
        if (kind == EMB_KIND_CONST && idx >= n_consts) return at + "names constant " + std::to_string(idx) + " of " + std::to_string(n_consts);
        return "";
    };
    for (int o = 0; o < n_ops; ++o) {
        const int code = ops[3 * o];
        if (code < 0 || code >= EMB_OP_COUNT) return "operation " + std::to_string(o) + " has the unknown opcode " + std::to_string(code);
        std::string r = operand(ops[3 * o + 1], o, "first");
        if (r.empty() && code <= EMB_DIV) r = operand(ops[3 * o + 2], o, "second");
        if (r.empty() && code == EMB_POWC) {
            r = operand(ops[3 * o + 2], o, "second");
            if (r.empty() && (ops[3 * o + 2] >> 8) != EMB_KIND_CONST) r = "operation " + std::to_string(o) + ": the exponent of a power must be a constant";
        }
        if (!r.empty()) return r;
    }
    if (result < 0 || (result >> 8) != EMB_KIND_SLOT || (result & 255) >= n_gps + n_ops)
        return "the result is not a value of the tape (an equation must depend on a GP)";
    return "";
}

}  // namespace fokl

extern "C" int fokl_embedded_plan(int n_gps, int n_ops, int *threads, size_t *lds_bytes)
{
    using namespace fokl;
    if (!threads || !lds_bytes) return fail(nullptr, FOKL_ERR_ARG, "fokl_embedded_plan: null pointer");
    if (n_gps < 1 || n_gps > EMB_MAX_GPS || n_ops < 0 || n_ops > EMB_MAX_OPS)
        return fail(nullptr, FOKL_ERR_ARG, "fokl_embedded_plan: " + std::to_string(n_gps) + " GPs and " + std::to_string(n_ops) +
                                               " operations, 1 to " + std::to_string(EMB_MAX_GPS) + " and at most " +
                                               std::to_string(EMB_MAX_OPS) + " expected");
    *lds_bytes = emb_plan(n_gps, n_ops, threads);
    return FOKL_OK;
}

extern "C" int fokl_embedded_hmc(fokl_ctx *ctx, int n_gps, int n_coef, const int32_t *term_slots, int n_cols,
                                 const int32_t *col_slots, int n_ops, const int32_t *ops, int n_consts, const double *consts,
                                 int32_t result, int n_chains, int draws, int leapfrog, uint32_t seed, const double *q0,
                                 double eps0, int adapt, double *states, double *potential, int32_t *accepted,
                                 double *eps_hist, double *inv_mass, double *eps_final, int32_t *status, double *grad0,
                                 double *proposal)
{
    using namespace fokl;
    const std::string who = "fokl_embedded_hmc: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    if (ctx->n <= 0) return fail(ctx, FOKL_ERR_STATE, who + "no dataset uploaded");
    if (!term_slots || (n_cols > 0 && !col_slots) || (n_ops > 0 && !ops) || (n_consts > 0 && !consts) || !states ||
        !potential || !accepted || !eps_hist || !inv_mass || !eps_final || !status)
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer");
    if (n_gps < 1 || n_gps > EMB_MAX_GPS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_gps) + " GPs, the kernel is built for 1 to " + std::to_string(EMB_MAX_GPS));
    if (n_cols < 0 || n_cols > EMB_MAX_COLS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_cols) + " columns, at most " + std::to_string(EMB_MAX_COLS));
    if (n_ops < 0 || n_ops > EMB_MAX_OPS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_ops) + " operations, at most " + std::to_string(EMB_MAX_OPS));
    if (n_consts < 0 || n_consts > EMB_MAX_CONSTS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_consts) + " constants, at most " + std::to_string(EMB_MAX_CONSTS));
    if (n_coef < 1 || (int64_t)n_gps * n_coef + 1 > EMB_MAX_PARAMS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_gps) + " GPs of " + std::to_string(n_coef) +
                                           " coefficients and ln sigma^2 are more than " + std::to_string(EMB_MAX_PARAMS) + " parameters");
    if ((int64_t)ctx->n * n_coef > EMB_MAX_VALUES)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(ctx->n) + " rows x " + std::to_string(n_coef) +
                                           " basis columns are more than the 4 194 304 values (32 MB) every chain can stream "
                                           "from the last-level cache; a row-parallel chain is not built");
    if (n_chains < 1 || n_chains > EMB_MAX_CHAINS || draws < 0 || draws > EMB_MAX_DRAWS || leapfrog < 1 ||
        leapfrog > EMB_MAX_LEAPFROG || !(eps0 >= 0.0) || !std::isfinite(eps0))
        return fail(ctx, FOKL_ERR_ARG, who + "chains in 1 .. 4096, draws in 0 .. 1 000 000, leapfrog in 1 .. 1000 and a finite "
                                           "eps0 >= 0 expected");
    const std::string refusal = emb_tape_refusal(n_gps, n_cols, n_ops, ops, n_consts, result);
    if (!refusal.empty()) return fail(ctx, FOKL_ERR_ARG, who + refusal);
    if (int rc = check_slots(ctx, term_slots, n_coef, "fokl_embedded_hmc")) return rc;
    if (n_cols > 0)
        if (int rc = check_slots(ctx, col_slots, n_cols, "fokl_embedded_hmc")) return rc;

    EmbProblem p{};
    p.n_gps = n_gps;
    p.n_coef = n_coef;
    p.n_params = n_gps * n_coef + 1;
    p.n_ops = n_ops;
    p.n_consts = n_consts;
    p.n_cols = n_cols;
    p.result = result & 255;
    p.draws = draws;
    p.leapfrog = leapfrog;
    p.adapt = adapt ? 1 : 0;
    p.n_windows = draws / EMB_WINDOW;
    p.seed = seed;
    p.n = ctx->n;
    p.ld = ctx->ld;
    p.eps0 = eps0;
    const int D = p.n_params;
    int threads = 0;
    const size_t lds_bytes = emb_plan(n_gps, n_ops, &threads);
    if (lds_bytes > EMB_LDS_BUDGET) return fail(ctx, FOKL_ERR_ARG, who + "the tape's values do not fit the LDS of a compute unit");

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    // the columns of the equation are gathered behind one base pointer: [n_cols][ld], device to device
    std::vector<const double *> xcols(n_coef);
    for (int t = 0; t < n_coef; ++t) xcols[t] = ctx->slot_ptr[term_slots[t]];
    const double **d_xcols = nullptr;
    double *d_cols = nullptr, *d_consts = nullptr, *d_q0 = nullptr, *d_w = nullptr, *d_states = nullptr, *d_U = nullptr,
           *d_hist = nullptr, *d_mass = nullptr, *d_eps = nullptr, *d_grad0 = nullptr, *d_prop = nullptr;
    int *d_ops = nullptr, *d_acc = nullptr, *d_status = nullptr;
    const size_t C = (size_t)n_chains, S = C * (draws + 1);
    HIP_TRY(ctx, buf.upload(&d_xcols, xcols.data(), xcols.size()));
    HIP_TRY(ctx, buf.get(&d_cols, (size_t)n_cols * p.ld));
    for (int c = 0; c < n_cols; ++c)
        HIP_TRY(ctx, hipMemcpyAsync(d_cols + (size_t)c * p.ld, ctx->slot_ptr[col_slots[c]], (size_t)p.n * sizeof(double),
                                    hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, buf.upload(&d_ops, ops, (size_t)3 * n_ops));
    HIP_TRY(ctx, buf.upload(&d_consts, consts, (size_t)n_consts));
    if (q0) HIP_TRY(ctx, buf.upload(&d_q0, q0, C * D));
    HIP_TRY(ctx, buf.get(&d_w, C * n_gps * p.ld));
    HIP_TRY(ctx, buf.get(&d_states, S * D));
    HIP_TRY(ctx, buf.get(&d_U, S));
    HIP_TRY(ctx, buf.get(&d_acc, S));
    HIP_TRY(ctx, buf.get(&d_hist, C * std::max(p.n_windows, 1)));
    HIP_TRY(ctx, buf.get(&d_mass, C * D));
    HIP_TRY(ctx, buf.get(&d_eps, C));
    HIP_TRY(ctx, buf.get(&d_status, 2 * C));
    if (grad0) HIP_TRY(ctx, buf.get(&d_grad0, C * D));
    if (proposal) HIP_TRY(ctx, buf.get(&d_prop, C * (D + 1)));

    auto kernel = threads == 256 ? hmc_chain_kernel<256> : hmc_chain_kernel<128>;
    if (lds_bytes > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)EMB_LDS_BUDGET));
    hipLaunchKernelGGL(kernel, dim3(n_chains), dim3(threads), lds_bytes, ctx->stream, p,
                       (const double *const *)d_xcols, (const double *)ctx->slot_ptr[FOKL_SLOT_Y], (const double *)d_cols,
                       (const int *)d_ops, (const double *)d_consts, (const double *)d_q0, d_w, d_states, d_U, d_acc, d_hist,
                       d_mass, d_eps, d_status, d_grad0, d_prop);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(states, d_states, S * D * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(potential, d_U, S * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(accepted, d_acc, S * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (p.n_windows > 0)
        HIP_TRY(ctx, hipMemcpy(eps_hist, d_hist, C * p.n_windows * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(inv_mass, d_mass, C * D * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(eps_final, d_eps, C * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(status, d_status, 2 * C * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (grad0) HIP_TRY(ctx, hipMemcpy(grad0, d_grad0, C * D * sizeof(double), hipMemcpyDeviceToHost));
    if (proposal) HIP_TRY(ctx, hipMemcpy(proposal, d_prop, C * (D + 1) * sizeof(double), hipMemcpyDeviceToHost));
    return FOKL_OK;
}

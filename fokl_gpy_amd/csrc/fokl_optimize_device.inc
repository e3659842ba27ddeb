// Multistart box-constrained optimisation of a Bernoulli-polynomial model over its posterior (textually included by
// fokl_hip.hip): one projected Newton solve per (draw, start), all solves at once.  The algorithm is stated in numpy
// by fokl_gpy_amd/optimize.py (solve_host: the module docstring lists the steps); this file is that statement, one lane
// per solve.  Compiled under the tree's -ffp-contract=off: nothing is fused.
//
// model_optimize_kernel: 64 solves per wavefront, one wavefront per workgroup -- what binds is the latency of a solve's
// dependent chain (a few dozen value / gradient / Hessian evaluations one after the other), so the wavefronts are spread
// over the CUs.  Solve n = draw n / S, start n % S: starts are the fast axis.  What is the same for every solve -- the
// term entries, the factors' (input, order), the polynomial coefficients, the box -- is wave-uniform: scalar loads.  A
// draw's coefficients are read where they were uploaded, [draw][coefficient]: with S a multiple of 64 a wavefront belongs
// to one draw and they are scalar loads too (the UNIFORM instantiation), otherwise each lane reads its draw's row (two
// rows per wavefront at S = 32, consecutive terms on one cache line).  What is a solve's own sits in LDS as [item][lane],
// touched by its own lane only (no barriers): phi, phi', phi'' of every distinct (input, order) factor -- evaluated once
// per iterate by Horner and shared by all terms --, the Hessian's lower triangle, which the Cholesky factor overwrites,
// and the iterate, the gradient and the direction.  All of them are indexed by wave-uniform run-time values; as register
// arrays they would live in scratch.  3 n_slots + m (m + 1) / 2 + 3 m rows of 512 bytes: 140 KB for 16 inputs with two
// orders each.
//
// A term is one 16-byte entry {slot, slot, slot, coefficient} (unused slots -1, slots in ascending input order): value,
// gradient and Hessian contributions of up to three factors are formed in registers from nine LDS reads.  A term with
// more factors (or none) is {-1 - k, offset, -, coefficient} and walks its k slots from a side list: the same sums by
// loops over factor pairs.  Control flow is wave-uniform throughout (the factorisation is modified in place instead of
// retried, the steepest-descent fall-back is a select); a solve that has stopped keeps its results in registers and
// idles until its wavefront is done.  No scratch.

#include <cfloat>

namespace fokl {

constexpr int OP_LANES = 64;
constexpr int OP_MAX_INPUTS = 16;
constexpr int OP_MAX_HALVINGS = 30;
constexpr size_t OP_LDS_BUDGET = 144 * 1024;
constexpr int64_t OP_MAX_SOLVES = (int64_t)1 << 20;
constexpr double OP_ARMIJO = 1e-4, OP_NOISE = 1e-13, OP_PIVOT_FLOOR = 1e-8;
constexpr int OP_CONVERGED = 0, OP_ITERATION_LIMIT = 1, OP_NON_FINITE = 2, OP_STALLED = 3;

struct OpProblem {
    int m, n_slots, n_entries, n_coef, n_hess, width, max_iter, n_starts;
    int64_t n_solves;
    double sign, tol;
};

// phi (and with LEVEL 2 phi', phi'') of every factor at the iterate, or with LEVEL 0 at the trial point
// P(x + alpha d): fac [3 n_slots][64]
template <int LEVEL>
__device__ __forceinline__ void op_factors(const OpProblem &p, const int *__restrict__ slot_src,
                                           const int *__restrict__ slot_ord, const double *__restrict__ table,
                                           const double *__restrict__ box, const double *xs, const double *dv,
                                           double alpha, double *fac)
{
    for (int s = 0; s < p.n_slots; ++s) {
        const int j = slot_src[s], order = slot_ord[s];
        const double *c = table + (size_t)(order - 1) * p.width;
        double x = xs[j * OP_LANES];
        if (LEVEL == 0) x = fmin(fmax(x + alpha * dv[j * OP_LANES], box[j]), box[p.m + j]);
        double value = c[order], slope = 0.0, bend = 0.0;
        for (int k = order - 1; k >= 0; --k) {
            if (LEVEL == 2) {
                bend = bend * x + slope;
                slope = slope * x + value;
            }
            value = value * x + c[k];
        }
        fac[(3 * s) * OP_LANES] = value;
        if (LEVEL == 2) {
            fac[(3 * s + 1) * OP_LANES] = slope;
            fac[(3 * s + 2) * OP_LANES] = 2.0 * bend;
        }
    }
}

// F = sign * model and the sum of its terms' magnitudes from the factor values; with LEVEL 2 also the gradient g [m][64]
// and the Hessian's lower triangle H [m (m + 1) / 2][64] (entry i (i + 1) / 2 + j, j <= i)
template <int LEVEL>
__device__ __forceinline__ void op_terms(const OpProblem &p, const int *__restrict__ slot_src,
                                         const int4 *__restrict__ entries, const int *__restrict__ long_slots,
                                         const double *__restrict__ coef, const double *fac, double *g, double *H,
                                         double &F, double &noise)
{
    if (LEVEL == 2) {
        for (int j = 0; j < p.m; ++j) g[j * OP_LANES] = 0.0;
        for (int h = 0; h < p.n_hess; ++h) H[h * OP_LANES] = 0.0;
    }
    F = p.sign * coef[0];
    noise = fabs(F);
#pragma unroll 2
    for (int t = 0; t < p.n_entries; ++t) {
        const int4 d = entries[t];
        const double w = p.sign * coef[d.w];
        if (d.x >= 0) {
            const double a0 = fac[(3 * d.x) * OP_LANES];
            const double a1 = d.y >= 0 ? fac[(3 * d.y) * OP_LANES] : 1.0;
            const double a2 = d.z >= 0 ? fac[(3 * d.z) * OP_LANES] : 1.0;
            const double term = w * (a0 * a1 * a2);
            F += term;
            noise += fabs(term);
            if (LEVEL == 2) {
                const int j0 = slot_src[d.x], h0 = j0 * (j0 + 1) / 2;
                const double b0 = fac[(3 * d.x + 1) * OP_LANES], c0 = fac[(3 * d.x + 2) * OP_LANES];
                const double r0 = w * (a1 * a2);
                g[j0 * OP_LANES] += r0 * b0;
                H[(h0 + j0) * OP_LANES] += r0 * c0;
                if (d.y >= 0) {
                    const int j1 = slot_src[d.y], h1 = j1 * (j1 + 1) / 2;
                    const double b1 = fac[(3 * d.y + 1) * OP_LANES], c1 = fac[(3 * d.y + 2) * OP_LANES];
                    const double r1 = w * (a0 * a2);
                    g[j1 * OP_LANES] += r1 * b1;
                    H[(h1 + j1) * OP_LANES] += r1 * c1;
                    H[(h1 + j0) * OP_LANES] += w * a2 * b1 * b0;
                    if (d.z >= 0) {
                        const int j2 = slot_src[d.z], h2 = j2 * (j2 + 1) / 2;
                        const double b2 = fac[(3 * d.z + 1) * OP_LANES], c2 = fac[(3 * d.z + 2) * OP_LANES];
                        const double r2 = w * (a0 * a1);
                        g[j2 * OP_LANES] += r2 * b2;
                        H[(h2 + j2) * OP_LANES] += r2 * c2;
                        H[(h2 + j0) * OP_LANES] += w * a1 * b2 * b0;
                        H[(h2 + j1) * OP_LANES] += w * a0 * b2 * b1;
                    }
                }
            }
        } else {
            const int k = -1 - d.x;
            const int *list = long_slots + d.y;
            double product = 1.0;
            for (int i = 0; i < k; ++i) product *= fac[(3 * list[i]) * OP_LANES];
            const double term = w * product;
            F += term;
            noise += fabs(term);
            if (LEVEL == 2) {
                for (int a = 0; a < k; ++a) {
                    const int sa = list[a], ja = slot_src[sa], ha = ja * (ja + 1) / 2;
                    double rest = 1.0;
                    for (int i = 0; i < k; ++i)
                        if (i != a) rest *= fac[(3 * list[i]) * OP_LANES];
                    rest = w * rest;
                    const double ba = fac[(3 * sa + 1) * OP_LANES];
                    g[ja * OP_LANES] += rest * ba;
                    H[(ha + ja) * OP_LANES] += rest * fac[(3 * sa + 2) * OP_LANES];
                    for (int b = 0; b < a; ++b) {
                        const int sb = list[b], jb = slot_src[sb];
                        double both = 1.0;
                        for (int i = 0; i < k; ++i)
                            if (i != a && i != b) both *= fac[(3 * list[i]) * OP_LANES];
                        H[(ha + jb) * OP_LANES] += w * both * ba * fac[(3 * sb + 1) * OP_LANES];
                    }
                }
            }
        }
    }
}

// The Newton direction into dv [m][64]: modified Cholesky of H (rows / columns of the `active` coordinates replaced by
// the unit ones) in place, then the two triangular solves with -g (0 where active)
__device__ __forceinline__ void op_newton(int m, unsigned active, double *H, const double *g, double *dv)
{
    double free_diag = 0.0;
    for (int j = 0; j < m; ++j)
        if (!((active >> j) & 1u)) free_diag = fmax(free_diag, fabs(H[(j * (j + 1) / 2 + j) * OP_LANES]));
    const double floor_ = OP_PIVOT_FLOOR * fmax(1.0, free_diag);
    for (int i = 0; i < m; ++i) {
        double *Hi = H + (size_t)(i * (i + 1) / 2) * OP_LANES;
        for (int j = 0; j <= i; ++j) {
            const double *Hj = H + (size_t)(j * (j + 1) / 2) * OP_LANES;
            double s = (((active >> i) | (active >> j)) & 1u) ? (i == j ? 1.0 : 0.0) : Hi[j * OP_LANES];
            for (int k = 0; k < j; ++k) s = s - Hi[k * OP_LANES] * Hj[k * OP_LANES];
            if (j < i) {
                Hi[j * OP_LANES] = s / Hj[j * OP_LANES];
            } else {
                if (!(s > floor_)) s = fmax(fabs(s), floor_);
                Hi[i * OP_LANES] = sqrt(s);
            }
        }
    }
    for (int i = 0; i < m; ++i) {
        const double *Hi = H + (size_t)(i * (i + 1) / 2) * OP_LANES;
        double s = ((active >> i) & 1u) ? 0.0 : -g[i * OP_LANES];
        for (int k = 0; k < i; ++k) s = s - Hi[k * OP_LANES] * dv[k * OP_LANES];
        dv[i * OP_LANES] = s / Hi[i * OP_LANES];
    }
    for (int i = m - 1; i >= 0; --i) {
        double s = dv[i * OP_LANES];
        for (int k = i + 1; k < m; ++k) s = s - H[(k * (k + 1) / 2 + i) * OP_LANES] * dv[k * OP_LANES];
        dv[i * OP_LANES] = s / H[(i * (i + 1) / 2 + i) * OP_LANES];
    }
}

// box [2][m] (lower bounds, upper bounds), starts [n_starts][m], betas [draws][n_coef]; x_out [n_solves][m], the others
// [n_solves].  Lanes beyond n_solves (the last wavefront) solve nothing and write nothing.
template <bool UNIFORM>
__global__ __launch_bounds__(OP_LANES) void model_optimize_kernel(OpProblem p, const int *__restrict__ slot_src,
                                                                  const int *__restrict__ slot_ord,
                                                                  const int4 *__restrict__ entries,
                                                                  const int *__restrict__ long_slots,
                                                                  const double *__restrict__ table,
                                                                  const double *__restrict__ box,
                                                                  const double *__restrict__ starts,
                                                                  const double *__restrict__ betas,
                                                                  double *__restrict__ x_out, double *__restrict__ f_out,
                                                                  int *__restrict__ it_out, int *__restrict__ st_out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * OP_LANES + lane;
    const bool real = n < p.n_solves;
    const int draw = real ? (int)(n / p.n_starts) : 0, start = real ? (int)(n % p.n_starts) : 0;
    const double *coef = betas + (size_t)(UNIFORM ? __builtin_amdgcn_readfirstlane(draw) : draw) * p.n_coef;
    const int m = p.m;
    double *fac = lds + lane;                                          // [3 n_slots][64]
    double *H = fac + (size_t)3 * p.n_slots * OP_LANES;                // [n_hess][64]
    double *xs = H + (size_t)p.n_hess * OP_LANES;                      // [m][64] each: iterate, gradient, direction
    double *g = xs + m * OP_LANES;
    double *dv = g + m * OP_LANES;
    unsigned fixed = 0;
    for (int j = 0; j < m; ++j) {
        xs[j * OP_LANES] = fmin(fmax(starts[(size_t)start * m + j], box[j]), box[m + j]);
        if (box[j] == box[m + j]) fixed |= 1u << j;
    }
    int status = real ? -1 : OP_CONVERGED, iterations = 0;             // -1: running
    double f_end = NAN;
    bool steepest = false;
    for (int it = 0; __any(status < 0); ++it) {
        double F, noise;
        op_factors<2>(p, slot_src, slot_ord, table, box, xs, dv, 0.0, fac);
        op_terms<2>(p, slot_src, entries, long_slots, coef, fac, g, H, F, noise);
        double pg = 0.0;
        unsigned active = fixed;
        bool finite = fabs(F) <= DBL_MAX;
        for (int j = 0; j < m; ++j) {
            const double x = xs[j * OP_LANES], gj = g[j * OP_LANES], lo = box[j], hi = box[m + j];
            finite = finite && fabs(gj) <= DBL_MAX;
            pg = fmax(pg, fabs(fmin(fmax(x - gj, lo), hi) - x));
            if ((x <= lo && gj > 0.0) || (x >= hi && gj < 0.0)) active |= 1u << j;
        }
        if (status < 0 && (!finite || pg <= p.tol || it == p.max_iter)) {
            status = !finite ? OP_NON_FINITE : pg <= p.tol ? OP_CONVERGED : OP_ITERATION_LIMIT;
            iterations = it;
            f_end = F;
        }
        if (!__any(status < 0)) break;
        op_newton(m, active, H, g, dv);
        double reach = 0.0;
        bool use_steepest = steepest;
        for (int j = 0; j < m; ++j) {
            const double dj = fabs(dv[j * OP_LANES]);
            use_steepest = use_steepest || !(dj <= DBL_MAX);
            reach = fmax(reach, dj);
        }
        if (use_steepest) {
            reach = 0.0;
            for (int j = 0; j < m; ++j) {
                const double dj = ((active >> j) & 1u) ? 0.0 : -g[j * OP_LANES];
                dv[j * OP_LANES] = dj;
                reach = fmax(reach, fabs(dj));
            }
        }
        if (reach > 1.0)
            for (int j = 0; j < m; ++j) dv[j * OP_LANES] = dv[j * OP_LANES] / reach;
        double alpha = 1.0;
        bool searching = status < 0;
        for (int h = 0; h <= OP_MAX_HALVINGS && __any(searching); ++h) {
            double Ft, noise_t;
            op_factors<0>(p, slot_src, slot_ord, table, box, xs, dv, alpha, fac);
            op_terms<0>(p, slot_src, entries, long_slots, coef, fac, g, H, Ft, noise_t);
            double slope = 0.0, moved = 0.0;
            for (int j = 0; j < m; ++j) {
                const double x = xs[j * OP_LANES];
                const double step = fmin(fmax(x + alpha * dv[j * OP_LANES], box[j]), box[m + j]) - x;
                slope = slope + g[j * OP_LANES] * step;
                moved = fmax(moved, fabs(step));
            }
            const bool ok = Ft <= F + OP_ARMIJO * fmin(slope, 0.0) + OP_NOISE * noise && moved > 0.0;
            if (searching && !ok) alpha = alpha * 0.5;
            searching = searching && !ok;
        }
        const bool failed = searching;                                 // no trial point passed
        if (status < 0 && !failed)
            for (int j = 0; j < m; ++j)
                xs[j * OP_LANES] = fmin(fmax(xs[j * OP_LANES] + alpha * dv[j * OP_LANES], box[j]), box[m + j]);
        if (failed && use_steepest) {
            status = OP_STALLED;
            iterations = it;
            f_end = F;
        }
        steepest = failed && !use_steepest;
    }
    if (real) {
        for (int j = 0; j < m; ++j) x_out[(size_t)n * m + j] = xs[j * OP_LANES];
        f_out[n] = p.sign * f_end;
        it_out[n] = iterations;
        st_out[n] = status;
    }
}

}  // namespace fokl

extern "C" int fokl_model_optimize(fokl_ctx *ctx, int n_inputs, int n_terms, const int32_t *mtx, int n_draws,
                                   const double *betas, const double *table, int n_basis, int width, const double *lo,
                                   const double *hi, int n_starts, const double *starts, double sign, int max_iter,
                                   double tol, double *x, double *f, int32_t *iterations, int32_t *status)
{
    const char *who = "fokl_model_optimize: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, std::string(who) + "null context");
    if (n_inputs <= 0 || n_terms < 0 || n_draws <= 0 || n_starts <= 0 || n_basis <= 0 || width <= 0 ||
        (n_terms > 0 && !mtx) || !betas || !table || !lo || !hi || !starts || !x || !f || !iterations || !status)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + "null pointer or empty problem");
    if (n_inputs > OP_MAX_INPUTS)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + std::to_string(n_inputs) + " inputs, the kernel is built for at most " +
                                           std::to_string(OP_MAX_INPUTS));
    if (!(sign == 1.0 || sign == -1.0) || max_iter < 0 || !(tol >= 0.0))
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + "sign must be +1 or -1, max_iter and tol not negative");
    for (int j = 0; j < n_inputs; ++j)
        if (!(lo[j] <= hi[j]) || !(std::fabs(lo[j]) <= DBL_MAX) || !(std::fabs(hi[j]) <= DBL_MAX))
            return fail(ctx, FOKL_ERR_ARG, std::string(who) + "empty or inverted box at input " + std::to_string(j));
    if ((int64_t)n_draws * n_starts > OP_MAX_SOLVES)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + std::to_string((int64_t)n_draws * n_starts) +
                                           " solves, one call runs at most " + std::to_string(OP_MAX_SOLVES));

    // ---- the model as the kernel reads it: distinct (input, order) factors, 16-byte term entries ----
    std::map<std::pair<int, int>, int> slot_of;
    std::vector<int32_t> slot_src, slot_ord, entries, long_slots;
    for (int t = 0; t < n_terms; ++t) {
        std::vector<int32_t> row;
        for (int j = 0; j < n_inputs; ++j) {
            const int order = mtx[(size_t)t * n_inputs + j];
            if (order < 0 || order > n_basis || order >= width)
                return fail(ctx, FOKL_ERR_ARG, std::string(who) + "basis order outside the coefficient table");
            if (order == 0) continue;
            const auto found = slot_of.emplace(std::make_pair(j, order), (int)slot_src.size());
            if (found.second) {
                slot_src.push_back(j);
                slot_ord.push_back(order);
            }
            row.push_back(found.first->second);
        }
        int32_t ent[4] = {-1, -1, -1, t + 1};
        if (row.empty() || row.size() > 3) {
            ent[0] = -1 - (int32_t)row.size();
            ent[1] = (int32_t)long_slots.size();
            long_slots.insert(long_slots.end(), row.begin(), row.end());
        } else {
            std::copy(row.begin(), row.end(), ent);
        }
        entries.insert(entries.end(), ent, ent + 4);
    }
    fokl::OpProblem p{};
    p.m = n_inputs;
    p.n_slots = (int)slot_src.size();
    p.n_entries = n_terms;
    p.n_coef = n_terms + 1;
    p.n_hess = n_inputs * (n_inputs + 1) / 2;
    p.width = width;
    p.max_iter = max_iter;
    p.n_starts = n_starts;
    p.n_solves = (int64_t)n_draws * n_starts;
    p.sign = sign;
    p.tol = tol;
    const size_t lds_rows = (size_t)3 * p.n_slots + p.n_hess + (size_t)3 * n_inputs;
    const size_t lds_bytes = lds_rows * OP_LANES * sizeof(double);
    if (lds_bytes > OP_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + std::to_string(p.n_slots) + " distinct (input, order) factors and " +
                                           std::to_string(p.n_hess) + " Hessian entries need " + std::to_string(lds_rows) +
                                           " values per solve, a wavefront's LDS holds " +
                                           std::to_string(OP_LDS_BUDGET / (OP_LANES * sizeof(double))));

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GiBuffers buf;                                                     // fokl_integrate_device.inc: freed on every way out
    const size_t N = (size_t)p.n_solves, m = (size_t)n_inputs;
    int *d_src = nullptr, *d_ord = nullptr, *d_long = nullptr, *d_it = nullptr, *d_st = nullptr;
    int4 *d_entries = nullptr;
    double *d_table = nullptr, *d_box = nullptr, *d_starts = nullptr, *d_betas = nullptr, *d_x = nullptr, *d_f = nullptr;
    HIP_TRY(ctx, buf.get(&d_src, slot_src.size()));
    HIP_TRY(ctx, buf.get(&d_ord, slot_ord.size()));
    HIP_TRY(ctx, buf.get(&d_long, long_slots.size()));
    HIP_TRY(ctx, buf.get(&d_entries, (size_t)n_terms));
    HIP_TRY(ctx, buf.get(&d_table, (size_t)n_basis * width));
    HIP_TRY(ctx, buf.get(&d_box, 2 * m));
    HIP_TRY(ctx, buf.get(&d_starts, (size_t)n_starts * m));
    HIP_TRY(ctx, buf.get(&d_betas, (size_t)n_draws * p.n_coef));
    HIP_TRY(ctx, buf.get(&d_x, N * m));
    HIP_TRY(ctx, buf.get(&d_f, N));
    HIP_TRY(ctx, buf.get(&d_it, N));
    HIP_TRY(ctx, buf.get(&d_st, N));
    if (!slot_src.empty()) {
        HIP_TRY(ctx, hipMemcpy(d_src, slot_src.data(), slot_src.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(d_ord, slot_ord.data(), slot_ord.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    if (!long_slots.empty())
        HIP_TRY(ctx, hipMemcpy(d_long, long_slots.data(), long_slots.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!entries.empty())
        HIP_TRY(ctx, hipMemcpy(d_entries, entries.data(), entries.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_table, table, (size_t)n_basis * width * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_box, lo, m * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_box + m, hi, m * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_starts, starts, (size_t)n_starts * m * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_betas, betas, (size_t)n_draws * p.n_coef * sizeof(double), hipMemcpyHostToDevice));

    const bool uniform = n_starts % OP_LANES == 0;                     // a wavefront belongs to one draw
    const void *kernel = uniform ? reinterpret_cast<const void *>(fokl::model_optimize_kernel<true>)
                                 : reinterpret_cast<const void *>(fokl::model_optimize_kernel<false>);
    if (lds_bytes > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OP_LDS_BUDGET));
    const int grid = (int)((N + OP_LANES - 1) / OP_LANES);
    {
        // per iterate and solve roughly: 40 flops and 9 + 18 LDS accesses per term, 6 flops per factor and degree
        TimedRegion timed(ctx, FOKL_K_OPTIMIZE, 8.0 * (double)N * (m + 3.0) + 8.0 * (double)n_draws * p.n_coef,
                          (double)N * 40.0 * std::max(1, n_terms));
        if (uniform)
            hipLaunchKernelGGL(fokl::model_optimize_kernel<true>, dim3(grid), dim3(OP_LANES), lds_bytes, ctx->stream, p,
                               d_src, d_ord, d_entries, d_long, d_table, d_box, d_starts, d_betas, d_x, d_f, d_it, d_st);
        else
            hipLaunchKernelGGL(fokl::model_optimize_kernel<false>, dim3(grid), dim3(OP_LANES), lds_bytes, ctx->stream, p,
                               d_src, d_ord, d_entries, d_long, d_table, d_box, d_starts, d_betas, d_x, d_f, d_it, d_st);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(x, d_x, N * m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(f, d_f, N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(iterations, d_it, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(status, d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FOKL_OK;
}

// What the two posterior optimisers share (textually included by fokl_hip.hip ahead of fokl_optimize_device.inc and
// fokl_optimize_system_device.inc): the evaluation of a Bernoulli-polynomial model from its term entries and ONE projected
// Newton step -- tests, active set, modified Cholesky, arc search, stall rule -- on the device, and on the host side of
// the entry points the packing of a model into those entries, the checks and the pick of an instantiation.  The step is
// stated in numpy by fokl_gpy_amd/optimize.py (_model_parts, _newton_step; the module docstring lists the steps 1-5).
// Compiled under the tree's -ffp-contract=off: nothing is fused.
//
// One lane per solve, 64 solves per wavefront, one wavefront per workgroup.  What is a solve's own sits in LDS as
// [item][lane], touched by its own lane only (no barriers), indexed by wave-uniform run-time values (as register arrays
// they would live in scratch): phi, phi', phi'' of every distinct (variable, order) factor of a model -- evaluated once per
// point by Horner and shared by all of its terms --, the Hessian's lower triangle (entry i (i + 1) / 2 + j, j <= i), which
// the Cholesky factor overwrites, and the iterate, the gradient and the direction.  What the problem is -- term entries,
// the factors' (variable, order), the polynomial coefficients, the box -- is wave-uniform: scalar loads.
//
// A term is one 16-byte entry {slot, slot, slot, coefficient} (unused slots -1, slots in ascending variable order): value,
// gradient and Hessian contributions of up to three factors are formed in registers from nine LDS reads.  A term with
// more factors (or none) is {-1 - k, offset, -, coefficient} and walks its k slots from a side list: the same sums by
// loops over factor pairs.  Control flow is wave-uniform throughout (the factorisation is modified in place instead of
// retried, the steepest-descent fall-back is a select).  No scratch.

#include <cfloat>

namespace fokl {

constexpr int OP_LANES = 64;
constexpr int OP_MAX_INPUTS = 16;
constexpr int OP_MAX_HALVINGS = 30;
constexpr size_t OP_LDS_BUDGET = 144 * 1024;
constexpr int64_t OP_MAX_SOLVES = (int64_t)1 << 20;
constexpr double OP_ARMIJO = 1e-4, OP_NOISE = 1e-13, OP_PIVOT_FLOOR = 1e-8;
constexpr int OP_CONVERGED = 0, OP_ITERATION_LIMIT = 1, OP_NON_FINITE = 2, OP_STALLED = 3;

// The trace of ONE iteration of every solve (fokl_model_optimize_trace, fokl_system_optimize_trace): a row of doubles per
// solve, written by the product kernels' TRACE instantiations.  Flags and counts are stored as doubles too (exact).
//   head    running (1: the solve was running when iteration k began; 0: it had stopped before, or its wavefront had),
//           F, noise, pg, active (the mask as a number), status after the tests of iteration k (-1: still running),
//           stepping, use_steepest, trial points, alpha, failed, steepest for the next iteration, status at the exit
//   x_in [m], g [m], H [m (m + 1) / 2] before the factorisation, factor [m (m + 1) / 2], d [m] after the select and the
//   scaling, trial [31] (NaN where the lane evaluated none), x_out [m]; the system kernel appends its own (SysTraceAt).
// The host fills every row with NaN and running = 0.  x_in and x_out are written for every real lane whose wavefront
// reaches iteration k, running or not.
constexpr int OP_TR_RUNNING = 0, OP_TR_F = 1, OP_TR_NOISE = 2, OP_TR_PG = 3, OP_TR_ACTIVE = 4, OP_TR_STATUS_TESTS = 5,
              OP_TR_STEPPING = 6, OP_TR_USE_STEEPEST = 7, OP_TR_TRIALS = 8, OP_TR_ALPHA = 9, OP_TR_FAILED = 10,
              OP_TR_STEEPEST_NEXT = 11, OP_TR_STATUS = 12, OP_TR_HEAD = 13;

struct OpTraceAt {                                                    // offsets into a row
    int flags, x_in, g, H, factor, d, trial, x_out, end;
    __host__ __device__ static OpTraceAt of(int m)
    {
        const int nh = m * (m + 1) / 2;
        OpTraceAt a;
        a.flags = 0;
        a.x_in = OP_TR_HEAD;
        a.g = a.x_in + m;
        a.H = a.g + m;
        a.factor = a.H + nh;
        a.d = a.factor + nh;
        a.trial = a.d + m;
        a.x_out = a.trial + OP_MAX_HALVINGS + 1;
        a.end = a.x_out + m;
        return a;
    }
};

struct OpTrace {
    double *row = nullptr;                                            // this lane's row while iteration k runs, else nullptr
    OpTraceAt at = {};
};

// What a TRACE kernel writes of iteration k before the step: the entry values and the status after the tests
__device__ __forceinline__ void op_trace_entry(const OpTrace &tr, int m, bool running, double F, double noise, double pg,
                                               unsigned active, int status, const double *xs, const double *g,
                                               const double *H)
{
    if (!tr.row) return;
    for (int j = 0; j < m; ++j) tr.row[tr.at.x_in + j] = tr.row[tr.at.x_out + j] = xs[j * OP_LANES];
    tr.row[OP_TR_RUNNING] = running;
    tr.row[OP_TR_STATUS_TESTS] = tr.row[OP_TR_STATUS] = status;
    if (!running) return;
    tr.row[OP_TR_F] = F;
    tr.row[OP_TR_NOISE] = noise;
    tr.row[OP_TR_PG] = pg;
    tr.row[OP_TR_ACTIVE] = active;
    for (int j = 0; j < m; ++j) tr.row[tr.at.g + j] = g[j * OP_LANES];
    for (int h = 0; h < m * (m + 1) / 2; ++h) tr.row[tr.at.H + h] = H[h * OP_LANES];
}

// ... and after it: where the solve is now, what it carries to the next iteration, its status
__device__ __forceinline__ void op_trace_exit(const OpTrace &tr, int m, const double *xs, bool steepest, int status)
{
    if (!tr.row) return;
    for (int j = 0; j < m; ++j) tr.row[tr.at.x_out + j] = xs[j * OP_LANES];
    tr.row[OP_TR_STEEPEST_NEXT] = steepest;
    tr.row[OP_TR_STATUS] = status;
}

// coordinate j of the iterate, or of the trial point P(x + alpha d); box [2][m] (lower bounds, upper bounds)
template <bool TRIAL>
__device__ __forceinline__ double op_point(int m, const double *box, const double *xs, const double *dv, double alpha, int j)
{
    const double x = xs[j * OP_LANES];
    return TRIAL ? fmin(fmax(x + alpha * dv[j * OP_LANES], box[j]), box[m + j]) : x;
}

// The polynomial c[0 .. order] at x by Horner: its value, with LEVEL 2 also its derivative and HALF its second derivative
template <int LEVEL>
__device__ __forceinline__ void op_horner(const double *__restrict__ c, int order, double x, double &value, double &slope,
                                          double &bend)
{
    value = c[order];
    slope = bend = 0.0;
    for (int k = order - 1; k >= 0; --k) {
        if (LEVEL == 2) {
            bend = bend * x + slope;
            slope = slope * x + value;
        }
        value = value * x + c[k];
    }
}

// phi (with LEVEL 2 also phi', phi'') of a model's factors into fac [3 n_slots][64], at the iterate or the trial point.
// MAPPED: factor s reads slot_map[2 s] + slot_map[2 s + 1] z and the derivatives are with respect to z; otherwise it
// reads the coordinate itself (no 0 + 1 * z: a -0.0 stays what it is).
template <int LEVEL, bool TRIAL, bool MAPPED>
__device__ __forceinline__ void op_factors(int n_slots, const int *__restrict__ slot_var, const int *__restrict__ slot_ord,
                                           const double *__restrict__ slot_map, const double *__restrict__ table, int width,
                                           int m, const double *box, const double *xs, const double *dv, double alpha,
                                           double *fac)
{
    for (int s = 0; s < n_slots; ++s) {
        const int order = slot_ord[s];
        double x = op_point<TRIAL>(m, box, xs, dv, alpha, slot_var[s]), b = 1.0;
        if (MAPPED) {
            b = slot_map[2 * s + 1];
            x = slot_map[2 * s] + b * x;
        }
        double value, slope, bend;
        op_horner<LEVEL>(table + (size_t)(order - 1) * width, order, x, value, slope, bend);
        fac[(3 * s) * OP_LANES] = value;
        if (LEVEL == 2) {
            fac[(3 * s + 1) * OP_LANES] = MAPPED ? slope * b : slope;
            fac[(3 * s + 2) * OP_LANES] = MAPPED ? 2.0 * bend * (b * b) : 2.0 * bend;
        }
    }
}

// One model from its factor values: e = scale x its value and the sum of its terms' magnitudes; with LEVEL 2 also scale x
// its gradient ADDED into g [m][64] and weight x its Hessian ADDED into H (the caller zeroes them).  scale is +-1 or 1:
// what is formed is the model's plain value and gradient, or their exact negatives.
template <int LEVEL>
__device__ __forceinline__ void op_terms(int n_entries, const int *__restrict__ slot_var, const int4 *__restrict__ entries,
                                         const int *__restrict__ long_slots, const double *__restrict__ coef, double scale,
                                         double weight, const double *fac, double *g, double *H, double &e, double &noise)
{
    e = scale * coef[0];
    noise = fabs(e);
#pragma unroll 2
    for (int t = 0; t < n_entries; ++t) {
        const int4 d = entries[t];
        const double w = scale * coef[d.w], wh = weight * coef[d.w];
        if (d.x >= 0) {
            const double a0 = fac[(3 * d.x) * OP_LANES];
            const double a1 = d.y >= 0 ? fac[(3 * d.y) * OP_LANES] : 1.0;
            const double a2 = d.z >= 0 ? fac[(3 * d.z) * OP_LANES] : 1.0;
            const double term = w * (a0 * a1 * a2);
            e += term;
            noise += fabs(term);
            if (LEVEL == 2) {
                const int j0 = slot_var[d.x], h0 = j0 * (j0 + 1) / 2;
                const double b0 = fac[(3 * d.x + 1) * OP_LANES], c0 = fac[(3 * d.x + 2) * OP_LANES];
                g[j0 * OP_LANES] += w * (a1 * a2) * b0;
                H[(h0 + j0) * OP_LANES] += wh * (a1 * a2) * c0;
                if (d.y >= 0) {
                    const int j1 = slot_var[d.y], h1 = j1 * (j1 + 1) / 2;
                    const double b1 = fac[(3 * d.y + 1) * OP_LANES], c1 = fac[(3 * d.y + 2) * OP_LANES];
                    g[j1 * OP_LANES] += w * (a0 * a2) * b1;
                    H[(h1 + j1) * OP_LANES] += wh * (a0 * a2) * c1;
                    H[(h1 + j0) * OP_LANES] += wh * a2 * b1 * b0;
                    if (d.z >= 0) {
                        const int j2 = slot_var[d.z], h2 = j2 * (j2 + 1) / 2;
                        const double b2 = fac[(3 * d.z + 1) * OP_LANES], c2 = fac[(3 * d.z + 2) * OP_LANES];
                        g[j2 * OP_LANES] += w * (a0 * a1) * b2;
                        H[(h2 + j2) * OP_LANES] += wh * (a0 * a1) * c2;
                        H[(h2 + j0) * OP_LANES] += wh * a1 * b2 * b0;
                        H[(h2 + j1) * OP_LANES] += wh * a0 * b2 * b1;
                    }
                }
            }
        } else {
            const int k = -1 - d.x;
            const int *list = long_slots + d.y;
            double product = 1.0;
            for (int i = 0; i < k; ++i) product *= fac[(3 * list[i]) * OP_LANES];
            const double term = w * product;
            e += term;
            noise += fabs(term);
            if (LEVEL == 2) {
                for (int a = 0; a < k; ++a) {
                    const int sa = list[a], ja = slot_var[sa], ha = ja * (ja + 1) / 2;
                    double rest = 1.0;
                    for (int i = 0; i < k; ++i)
                        if (i != a) rest *= fac[(3 * list[i]) * OP_LANES];
                    const double ba = fac[(3 * sa + 1) * OP_LANES];
                    g[ja * OP_LANES] += w * rest * ba;
                    H[(ha + ja) * OP_LANES] += wh * rest * fac[(3 * sa + 2) * OP_LANES];
                    for (int b = 0; b < a; ++b) {
                        const int sb = list[b], jb = slot_var[sb];
                        double both = 1.0;
                        for (int i = 0; i < k; ++i)
                            if (i != a && i != b) both *= fac[(3 * list[i]) * OP_LANES];
                        H[(ha + jb) * OP_LANES] += wh * both * ba * fac[(3 * sb + 1) * OP_LANES];
                    }
                }
            }
        }
    }
}

// What the tests and the step need from the merit F and its gradient g at the iterate: are they finite, the projected
// gradient max_j |P(x - g)_j - x_j|, and the active set -- the `fixed` coordinates and those on a bound whose descent
// direction points outwards
__device__ __forceinline__ void op_survey(int m, const double *box, const double *xs, const double *g, double F,
                                          unsigned fixed, bool &finite, double &pg, unsigned &active)
{
    pg = 0.0;
    active = fixed;
    finite = fabs(F) <= DBL_MAX;
    for (int j = 0; j < m; ++j) {
        const double x = xs[j * OP_LANES], gj = g[j * OP_LANES], lo = box[j], hi = box[m + j];
        finite = finite && fabs(gj) <= DBL_MAX;
        pg = fmax(pg, fabs(fmin(fmax(x - gj, lo), hi) - x));
        if ((x <= lo && gj > 0.0) || (x >= hi && gj < 0.0)) active |= 1u << j;
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

// One step of the solves that are `stepping`, from the iterate xs where the merit is F (sum of magnitudes `noise`) with
// gradient g and Hessian triangle H: the Newton direction -- projected steepest descent where `steepest` asks for it or
// the Newton direction is not finite --, scaled to at most one box width, then halving along the projection arc under the
// Armijo test with its rounding allowance.  merit_at(alpha) returns the merit at P(x + alpha d); it reads xs and dv and
// may overwrite whatever else the caller gives it.  A solve whose search passes moves to that point.  One whose search
// fails takes steepest descent from the same point next time (`steepest`); when this already was steepest descent the
// function returns true for it: stalled.  Every lane runs every loop; what a lane that is not stepping computes is dropped.
// TRACE (the *_trace entry points; compiled away otherwise): a lane whose `tr.row` is set writes what this step decided
// into its row of the trace -- see OpTrace.
template <bool TRACE = false, typename MeritAt>
__device__ __forceinline__ bool op_step(int m, const double *box, unsigned active, bool stepping, double F, double noise,
                                        double *H, const double *g, double *dv, double *xs, bool &steepest,
                                        MeritAt &&merit_at, const OpTrace &tr = OpTrace())
{
    op_newton(m, active, H, g, dv);
    if constexpr (TRACE)
        if (tr.row)
            for (int h = 0; h < m * (m + 1) / 2; ++h) tr.row[tr.at.factor + h] = H[h * OP_LANES];
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
    int trials = 0;                                                    // trial points this lane evaluated (TRACE only)
    (void)trials;
    if constexpr (TRACE)
        if (tr.row) {
            for (int j = 0; j < m; ++j) tr.row[tr.at.d + j] = dv[j * OP_LANES];
            tr.row[tr.at.flags + OP_TR_USE_STEEPEST] = use_steepest;
            tr.row[tr.at.flags + OP_TR_STEPPING] = stepping;
        }
    double alpha = 1.0;
    bool searching = stepping;
    for (int h = 0; h <= OP_MAX_HALVINGS && __any(searching); ++h) {
        const double Ft = merit_at(alpha);
        if constexpr (TRACE)
            if (tr.row && searching) {
                tr.row[tr.at.trial + h] = Ft;
                ++trials;
            }
        double slope = 0.0, moved = 0.0;
        for (int j = 0; j < m; ++j) {
            const double step = op_point<true>(m, box, xs, dv, alpha, j) - xs[j * OP_LANES];
            slope = slope + g[j * OP_LANES] * step;
            moved = fmax(moved, fabs(step));
        }
        const bool ok = Ft <= F + OP_ARMIJO * fmin(slope, 0.0) + OP_NOISE * noise && moved > 0.0;
        if (searching && !ok) alpha = alpha * 0.5;
        searching = searching && !ok;
    }
    const bool failed = searching;                                     // no trial point passed
    if (stepping && !failed)
        for (int j = 0; j < m; ++j) xs[j * OP_LANES] = op_point<true>(m, box, xs, dv, alpha, j);
    steepest = failed && !use_steepest;
    if constexpr (TRACE)
        if (tr.row) {
            tr.row[tr.at.flags + OP_TR_TRIALS] = trials;
            tr.row[tr.at.flags + OP_TR_ALPHA] = alpha;
            tr.row[tr.at.flags + OP_TR_FAILED] = failed;
        }
    return failed && use_steepest;
}

}  // namespace fokl

namespace {

// Models as the kernels read them, one after the other: the distinct (variable, order) factors of each (its SLOTS, counted
// from the model's first), a 16-byte entry per term, the slots of the longer terms
struct OpTables {
    std::vector<int32_t> slot_var, slot_ord, entries, long_slots;
    std::vector<double> slot_map;                                      // per slot (shift, slope); only when asked for
};

// Appends the model mtx [n_terms][n_inputs] whose input j reads variable var_of[j] (nullptr: variable j) through
// shift[j] + slope[j] z (nullptr: no map is kept).  False: a basis order outside the coefficient table.
bool op_pack_model(const int32_t *mtx, int n_inputs, int n_terms, const int32_t *var_of, const double *shift,
                   const double *slope, int n_basis, int width, OpTables &out)
{
    std::map<std::pair<int, int>, int> slot_of;                        // (variable, order) -> the model's slot
    const int slot0 = (int)out.slot_var.size();
    for (int t = 0; t < n_terms; ++t) {
        std::vector<std::pair<int, int>> row;                          // (variable, slot): ascending variable order
        for (int j = 0; j < n_inputs; ++j) {
            const int order = mtx[(size_t)t * n_inputs + j];
            if (order < 0 || order > n_basis || order >= width) return false;
            if (order == 0) continue;
            const int v = var_of ? var_of[j] : j;
            const auto found = slot_of.emplace(std::make_pair(v, order), (int)out.slot_var.size() - slot0);
            if (found.second) {
                out.slot_var.push_back(v);
                out.slot_ord.push_back(order);
                if (shift) out.slot_map.insert(out.slot_map.end(), {shift[j], slope[j]});
            }
            row.emplace_back(v, found.first->second);
        }
        std::sort(row.begin(), row.end());
        int32_t ent[4] = {-1, -1, -1, t + 1};
        if (row.empty() || row.size() > 3) {
            ent[0] = -1 - (int32_t)row.size();
            ent[1] = (int32_t)out.long_slots.size();
            for (const auto &r : row) out.long_slots.push_back(r.second);
        } else {
            for (size_t i = 0; i < row.size(); ++i) ent[i] = row[i].second;
        }
        out.entries.insert(out.entries.end(), ent, ent + 4);
    }
    return true;
}

// What both entry points refuse about the sense and the limits of a solve, the box and the number of solves ("": nothing).
// `limits` says which arguments `limits_ok` is about, `unit` what a coordinate of the box is called.
std::string op_refusal(double sign, bool limits_ok, const char *limits, int n, const double *lo, const double *hi,
                       const char *unit, int n_draws, int n_starts)
{
    if (!(sign == 1.0 || sign == -1.0) || !limits_ok) return std::string("sign must be +1 or -1, ") + limits + " not negative";
    for (int j = 0; j < n; ++j)
        if (!(lo[j] <= hi[j]) || !(std::fabs(lo[j]) <= DBL_MAX) || !(std::fabs(hi[j]) <= DBL_MAX))
            return std::string("empty or inverted box at ") + unit + " " + std::to_string(j);
    if ((int64_t)n_draws * n_starts > fokl::OP_MAX_SOLVES)
        return std::to_string((int64_t)n_draws * n_starts) + " solves, one call runs at most " +
               std::to_string(fokl::OP_MAX_SOLVES);
    return std::string();
}

// The instantiation for this number of starts -- UNIFORM when a wavefront belongs to one draw --, allowed its LDS
// (`raised`: the attribute that lifts the 64 KB default was set)
template <typename Kernel>
hipError_t op_pick(Kernel *uniform, Kernel *per_lane, int n_starts, size_t lds_bytes, Kernel **kernel, bool *raised)
{
    *kernel = n_starts % fokl::OP_LANES == 0 ? uniform : per_lane;
    *raised = lds_bytes > 64 * 1024;
    return lds_opt_in(*kernel, lds_bytes, fokl::OP_LDS_BUDGET);
}

}  // namespace

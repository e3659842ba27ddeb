// dynamics.simulate (textually included by fokl_hip.hip, after fokl_integrate_device.inc): a system of fitted models wired
// by variable names, one Runge-Kutta integration per posterior draw / initial state, all members at once.
//
// The statement of the arithmetic is dynamics.simulate_host (fokl_gpy_amd/dynamics.py, module docstring); this file
// follows it operation for operation and in its order, so a member's trajectory equals the host's bit for bit: only
// + - * /, ceil and comparisons, compiled under the tree's -ffp-contract=off (nothing is fused).
//
// simulate_ensemble_kernel<NS> has integrate_ensemble_kernel's layout: one lane per member, one wavefront per workgroup;
// what is a member's own sits in LDS as [item][lane] (slot 0 = 1.0, the values of the distinct factors, the stage's
// normalised states, the coefficients), read and written by its own lane only (no barriers); a term is one 16-byte entry
// {slot, slot, slot, coefficient} and a product of more than three factors continues in the next entry (coefficient -1).
// What is the same for every member is a kernel argument or a load at a wave-uniform address: the wiring, the term lists,
// each normalisation's (lo, hi - lo), the box, the forcing row, the Bernoulli coefficients of the used orders.
// New relative to that kernel:
//   * a normalised input is a (state or forcing column, lo, hi - lo) triple: every model normalises with its own minmax,
//     so two models that read one state with different ranges have two of them (forcing first, then ordered by state);
//   * a factor is (normalised input, kernel, order); the factors are ordered forcing splines, forcing Bernoulli, state
//     splines, state Bernoulli -- forcing factors are evaluated once per step, state factors once per stage, and the
//     kernel of a factor follows from its position (wave-uniform loop bounds, no per-lane branch);
//   * the spline gather on the fit's own 499 pieces (FR:570-589): the table holds the used orders only, as
//     [order][piece][4], one 32-byte run per evaluation; Bernoulli factors are Horner over a [row][21] table;
//   * a per-lane first_saturation register: the first step in which a normalised input was clamped or the slope rule
//     changed a slope; carried in device memory between launches, written once at the end of each.
// LDS bytes = (1 + factors + normalised states + coefficients) x 64 lanes x 8; SIM_LDS_BUDGET bounds them.
//
// The time axis is cut into launches of at most FOKL_SIMULATE_STEPS_PER_LAUNCH steps (default 512); a launch writes its
// points as [state][point][member], and ensemble_band_kernel / ensemble_transpose_kernel (fokl_integrate_device.inc) form
// the mean, the bounds and the members from them, unchanged.

namespace fokl {

constexpr int SIM_MAX_STATES = 8;
constexpr int SIM_LANES = 64;
constexpr int SIM_PIECES = 499;
constexpr int SIM_BERN_WIDTH = 21;           // coefficients of the highest Bernoulli order (20)
constexpr size_t SIM_LDS_BUDGET = 144 * 1024;

struct SimSystem {
    int n_norm_forcing, n_norm;              // normalised inputs [0, n_norm_forcing) read the forcing row, the others a state
    int norm_begin[SIM_MAX_STATES + 1];      // ... ordered by state: those of state j are [norm_begin[j], norm_begin[j + 1])
    int n_forcing_splines, n_forcing_factors, n_state_splines_end, n_factors;    // the four ranges of the factors
    int n_coef, n_forcing_cols;
    int entry_begin[SIM_MAX_STATES];         // model k: entries [entry_begin[k], entry_begin[k] + entry_count[k])
    int entry_count[SIM_MAX_STATES];
    int constant[SIM_MAX_STATES];            // index of betas[k][0] among the coefficients
    double box_lo[SIM_MAX_STATES], box_hi[SIM_MAX_STATES];
    double h;
};

// dynamics.spline_value: the fit's piece and local coordinate (FR:570-589).  v is in [0, 1] after the clamps, so the piece
// is in [0, 498]; anything else (a NaN) reads piece 0 and stays inside the table.
__device__ __forceinline__ double sim_cubic(const double *__restrict__ table, int row, double v)
{
    double p = ceil(v * 499.0);
    p = p + (p == 0.0 ? 1.0 : 0.0);
    p = p - 1.0;
    const double s = 499.0 * v - p;
    const int piece = (p >= 0.0 && p <= (double)(SIM_PIECES - 1)) ? (int)p : 0;
    const double2 *c = reinterpret_cast<const double2 *>(table + ((size_t)row * SIM_PIECES + piece) * 4);
    const double2 c01 = c[0], c23 = c[1];
    return c01.x + s * (c01.y + s * (c23.x + s * c23.y));
}

// dynamics.bernoulli_value: Horner, highest coefficient first (op_horner's value path); c is wave-uniform
__device__ __forceinline__ double sim_horner(const double *__restrict__ c, int degree, double v)
{
    double value = c[degree];
    for (int k = degree - 1; k >= 0; --k) value = value * v + c[k];
    return value;
}

__device__ __forceinline__ double sim_clamp(double v, bool &acted)
{
    acted = acted || v > 1.0 || v < 0.0;
    if (v > 1.0) v = 1.0;
    if (v < 0.0) v = 0.0;
    return v;
}

struct SimTables {
    const int *norm_src;                     // >= 0 a state, -(c + 1) forcing column c
    const double *norm_lo, *norm_span;
    const int *fac_norm, *fac_row, *fac_degree;
    const int4 *entries;
    const double *spline, *bern;
};

// h * model_k(at) for every state k after the slope rule; true if a clamp or the rule acted for this lane.  CS is the
// stride of the coefficients behind cf: SIM_LANES where every lane has its own ([coefficient][lane], cf offset by the lane),
// 1 where the wavefront shares one set (fokl_assimilate_device.inc: lane = particle of one draw).  OWN_STEP: the slope is
// scaled by the lane's own `step` in the place of the wave-uniform sys.h (fokl_simulate_adaptive_device.inc)
template <int NS, int CS = SIM_LANES, bool OWN_STEP = false>
__device__ __forceinline__ bool sim_stage(const SimSystem &sys, const SimTables &tab, double *xn, double *fac,
                                          const double *cf, const double (&at)[NS], double (&dy)[NS], double step = 0.0)
{
    bool acted = false;
    // the normalised inputs of state j are [norm_begin[j], norm_begin[j + 1]): j is a compile-time index into the registers
#pragma unroll
    for (int j = 0; j < NS; ++j)
        for (int n = sys.norm_begin[j]; n < sys.norm_begin[j + 1]; ++n)
            xn[(n - sys.n_norm_forcing) * SIM_LANES] = sim_clamp((at[j] - tab.norm_lo[n]) / tab.norm_span[n], acted);
    // four cubics at a time, their inputs read before and their values stored after: four table gathers in flight
    int f = sys.n_forcing_factors;
    for (; f + 4 <= sys.n_state_splines_end; f += 4) {
        double x[4], v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = xn[(tab.fac_norm[f + q] - sys.n_norm_forcing) * SIM_LANES];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = sim_cubic(tab.spline, tab.fac_row[f + q], x[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) fac[(f + 1 + q) * SIM_LANES] = v[q];
    }
    for (; f < sys.n_state_splines_end; ++f)
        fac[(f + 1) * SIM_LANES] = sim_cubic(tab.spline, tab.fac_row[f], xn[(tab.fac_norm[f] - sys.n_norm_forcing) * SIM_LANES]);
    for (; f < sys.n_factors; ++f)
        fac[(f + 1) * SIM_LANES] = sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f],
                                              xn[(tab.fac_norm[f] - sys.n_norm_forcing) * SIM_LANES]);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int4 *ent = tab.entries + sys.entry_begin[k];
        double delta = 0.0, phi = 1.0;
#pragma unroll 4
        for (int t = 0; t < sys.entry_count[k]; ++t) {
            const int4 d = ent[t];
            phi = phi * fac[d.x * SIM_LANES];
            phi = phi * fac[d.y * SIM_LANES];
            phi = phi * fac[d.z * SIM_LANES];
            const bool ends = d.w >= 0;                                 // wave-uniform
            const double with = delta + cf[max(d.w, 0) * CS] * phi;
            delta = ends ? with : delta;
            phi = ends ? 1.0 : phi;
        }
        double s = (delta + cf[sys.constant[k] * CS]) * (OWN_STEP ? step : sys.h);
        const bool outwards = (at[k] >= sys.box_hi[k] && s > 0) || (at[k] <= sys.box_lo[k] && s < 0);
        if (outwards) s = 0;
        acted = acted || outwards;
        dy[k] = s;
    }
    return acted;
}

// Steps [t0, t0 + steps) of every member.  state [NS][ld] and saturation [ld] in / out; points [NS][chunk_points][ld]: with
// write_first the state before the first step goes to point 0 and step s to point s + 1, otherwise step s to point s.
// ld = members rounded up to 64 = 64 * gridDim.x: every lane owns a column of every buffer (the padding members
// integrate zeros).
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void simulate_ensemble_kernel(
    SimSystem sys, const int *__restrict__ norm_src, const double *__restrict__ norm_lo, const double *__restrict__ norm_span,
    const int *__restrict__ fac_norm, const int *__restrict__ fac_row, const int *__restrict__ fac_degree,
    const int4 *__restrict__ entries, const double *__restrict__ spline, const double *__restrict__ bern,
    const double *__restrict__ coef, const double *__restrict__ forcing, double *__restrict__ state,
    int *__restrict__ saturation, double *__restrict__ points, int64_t ld, int64_t t0, int steps, int chunk_points,
    int write_first)
{
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * SIM_LANES + lane;
    double *fac = lds + lane;                                          // [1 + n_factors][64]: slot 0 is 1.0
    double *xn = lds + (size_t)(1 + sys.n_factors) * SIM_LANES + lane; // [n_norm - n_norm_forcing][64]
    double *cf = xn + (sys.n_norm - sys.n_norm_forcing) * SIM_LANES;   // [n_coef][64]
    fac[0] = 1.0;
    for (int c = 0; c < sys.n_coef; ++c) cf[c * SIM_LANES] = coef[(size_t)c * ld + e];
    double y[NS], at[NS], dy[NS] = {}, sum[NS] = {};
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = state[(size_t)j * ld + e];
    int first = saturation[e];
    if (write_first) {
#pragma unroll
        for (int j = 0; j < NS; ++j) points[(size_t)j * chunk_points * ld + e] = y[j];
    }
    double *out = points + (write_first ? ld : 0) + e;
    for (int s = 0; s < steps; ++s) {
        const double *row = forcing + (size_t)(t0 + s) * sys.n_forcing_cols;    // the same row serves the four stages
        bool acted = false;
        for (int f = 0; f < sys.n_forcing_factors; ++f) {
            const int n = tab.fac_norm[f];
            const double v = sim_clamp((row[-(tab.norm_src[n] + 1)] - tab.norm_lo[n]) / tab.norm_span[n], acted);
            fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                           ? sim_cubic(tab.spline, tab.fac_row[f], v)
                                           : sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v);
        }
        // the four stages as one loop body: y, y + dy1 / 2, y + dy2 / 2, y + dy3, and dy1 + 2 dy2 + 2 dy3 + dy4 summed
        // left to right -- dy * 0.5 is dy / 2 and 1.0 * dy is dy, bit for bit
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            const double reach = st == 3 ? 1.0 : 0.5, weight = (st == 1 || st == 2) ? 2.0 : 1.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) at[j] = st == 0 ? y[j] : y[j] + dy[j] * reach;
            const bool stage_acted = sim_stage<NS>(sys, tab, xn, fac, cf, at, dy);
            acted = acted || stage_acted;
#pragma unroll
            for (int j = 0; j < NS; ++j) sum[j] = st == 0 ? dy[j] : sum[j] + weight * dy[j];
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            y[j] += sum[j] / 6;
            out[((size_t)j * chunk_points + s) * ld] = y[j];
        }
        if (first < 0 && acted) first = (int)(t0 + s);
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) state[(size_t)j * ld + e] = y[j];
    saturation[e] = first;
}

}  // namespace fokl

namespace {

// The kernel instance of a system: f(std::integral_constant<int, NS>) with NS = n_states, 1 .. SIM_MAX_STATES
template <class F>
hipError_t sim_dispatch(int n_states, F &&f)
{
    switch (n_states) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
    }
    return hipErrorInvalidValue;
}

// What the simulate calls and the filter refuse of n_steps (sim_check's steps_test; control has its own)
int sim_steps_fit(fokl_ctx *ctx, const std::string &who, const fokl_system &s)
{
    if (s.n_steps + 1 > (int64_t)1 << 30) return fail(ctx, FOKL_ERR_ARG, who + "too many steps");
    return FOKL_OK;
}

// What every entry point refuses first, in this order: a null pointer or a size that cannot be (own_ok: the caller's own
// pointers, the same refusal), too many states, the caller's test of n_steps, h.  0, or the refusal's code.
int sim_check(fokl_ctx *ctx, const std::string &who, const fokl_system *system, bool own_ok,
              int (*steps_test)(fokl_ctx *, const std::string &, const fokl_system &))
{
    if (!system || !own_ok) return fail(ctx, FOKL_ERR_ARG, who + "null pointer, negative size or empty system");
    const fokl_system &s = *system;
    if (s.n_members <= 0 || s.n_states <= 0 || s.n_steps < 0 || s.n_forcing_cols < 0 || s.n_norm_forcing < 0 ||
        s.n_norm < s.n_norm_forcing || s.n_forcing_factors < 0 || s.n_factors < s.n_forcing_factors || s.n_spline_rows < 0 ||
        s.n_bern_rows < 0 || s.n_entries < 0 || s.n_coef < s.n_states || !s.entry_begin || !s.entry_count || !s.constant ||
        !s.coef || !s.y0 || !s.box || (s.n_norm > 0 && (!s.norm_src || !s.norm_lo || !s.norm_span)) ||
        (s.n_factors > 0 && (!s.fac_norm || !s.fac_kind || !s.fac_row || !s.fac_degree)) || (s.n_entries > 0 && !s.entries) ||
        (s.n_spline_rows > 0 && !s.spline_table) || (s.n_bern_rows > 0 && !s.bern_table) ||
        (s.n_forcing_cols > 0 && s.n_steps > 0 && !s.forcing))
        return fail(ctx, FOKL_ERR_ARG, who + "null pointer, negative size or empty system");
    if (s.n_states > SIM_MAX_STATES)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(s.n_states) + " states, the kernel is built for at most " +
                                           std::to_string(SIM_MAX_STATES));
    if (const int refused = steps_test(ctx, who, s)) return refused;
    if (!(s.h > 0) || !std::isfinite(s.h)) return fail(ctx, FOKL_ERR_ARG, who + "h must be positive and finite");
    return FOKL_OK;
}

// Every index simulate_ensemble_kernel / assimilate_kernel follow, checked on the host (they read nothing outside their
// tables), and the system as the kernels take it.  0, or the refusal's code with its text in the context.
int sim_plan(fokl_ctx *ctx, const std::string &who, const fokl_system &s, SimSystem &sys, int &n_bern_factors)
{
    // ---- every index the kernel follows, checked here: it reads nothing outside its tables ----
    for (int n = 0; n < s.n_norm; ++n) {
        const int src = s.norm_src[n];
        const bool ok = n < s.n_norm_forcing ? (src < 0 && -(int64_t)src - 1 < s.n_forcing_cols) : (src >= 0 && src < s.n_states);
        if (!ok) return fail(ctx, FOKL_ERR_ARG, who + "a normalised input reads outside the states / the forcing columns");
        if (n > s.n_norm_forcing && src < s.norm_src[n - 1])
            return fail(ctx, FOKL_ERR_ARG, who + "the normalised inputs of the states must be ordered by state");
        if (!(s.norm_span[n] > 0) || !std::isfinite(s.norm_span[n]) || !std::isfinite(s.norm_lo[n]))
            return fail(ctx, FOKL_ERR_ARG, who + "a normalisation needs a finite lower end and a positive finite span");
    }
    int n_forcing_splines = 0, n_state_splines = 0;
    n_bern_factors = 0;
    for (int f = 0; f < s.n_factors; ++f) {
        const bool is_forcing = f < s.n_forcing_factors, spline = s.fac_kind[f] == 0;
        if (s.fac_kind[f] != 0 && s.fac_kind[f] != 1)
            return fail(ctx, FOKL_ERR_ARG, who + "a factor's kernel is neither 0 (splines) nor 1 (Bernoulli)");
        if (spline && f > 0 && s.fac_kind[f - 1] == 1 && f != s.n_forcing_factors)
            return fail(ctx, FOKL_ERR_ARG, who + "the factors must be ordered splines before Bernoulli, forcing before states");
        const int n = s.fac_norm[f];
        if (is_forcing ? (n < 0 || n >= s.n_norm_forcing) : (n < s.n_norm_forcing || n >= s.n_norm))
            return fail(ctx, FOKL_ERR_ARG, who + "a factor reads outside the normalised inputs of its kind");
        if (s.fac_row[f] < 0 || s.fac_row[f] >= (spline ? s.n_spline_rows : s.n_bern_rows))
            return fail(ctx, FOKL_ERR_ARG, who + "a factor's order lies outside its coefficient table");
        if (!spline && (s.fac_degree[f] < 0 || s.fac_degree[f] >= SIM_BERN_WIDTH))
            return fail(ctx, FOKL_ERR_ARG, who + "Bernoulli orders above " + std::to_string(SIM_BERN_WIDTH - 1) + " are not handled");
        n_forcing_splines += is_forcing && spline;
        n_state_splines += !is_forcing && spline;
        n_bern_factors += !spline;
    }
    for (int t = 0; t < s.n_entries; ++t) {
        const int32_t *d = s.entries + 4 * (size_t)t;
        if (d[0] < 0 || d[0] > s.n_factors || d[1] < 0 || d[1] > s.n_factors || d[2] < 0 || d[2] > s.n_factors || d[3] < -1 ||
            d[3] >= s.n_coef)
            return fail(ctx, FOKL_ERR_ARG, who + "a term entry points outside the factors / the coefficients");
    }
    sys = SimSystem{};
    for (int k = 0; k < s.n_states; ++k) {
        if (s.entry_begin[k] < 0 || s.entry_count[k] < 0 || (int64_t)s.entry_begin[k] + s.entry_count[k] > s.n_entries ||
            s.constant[k] < 0 || s.constant[k] >= s.n_coef)
            return fail(ctx, FOKL_ERR_ARG, who + "a model's term list or constant lies outside the tables");
        if (!(s.box[2 * k] < s.box[2 * k + 1])) return fail(ctx, FOKL_ERR_ARG, who + "a state's box is empty");
        sys.entry_begin[k] = s.entry_begin[k];
        sys.entry_count[k] = s.entry_count[k];
        sys.constant[k] = s.constant[k];
        sys.box_lo[k] = s.box[2 * k];
        sys.box_hi[k] = s.box[2 * k + 1];
    }
    sys.n_norm_forcing = s.n_norm_forcing;
    sys.n_norm = s.n_norm;
    for (int j = 0, n = s.n_norm_forcing; j <= SIM_MAX_STATES; ++j) {
        while (n < s.n_norm && s.norm_src[n] < j) ++n;
        sys.norm_begin[j] = n;
    }
    sys.n_forcing_splines = n_forcing_splines;
    sys.n_forcing_factors = s.n_forcing_factors;
    sys.n_state_splines_end = s.n_forcing_factors + n_state_splines;
    sys.n_factors = s.n_factors;
    sys.n_coef = s.n_coef;
    sys.n_forcing_cols = s.n_forcing_cols;
    sys.h = s.h;
    return FOKL_OK;
}

// The term entries of every state over one stage, for the kernel timers' work estimates
double sim_terms_per_stage(const SimSystem &sys, int n_states)
{
    double terms = 0.0;
    for (int k = 0; k < n_states; ++k) terms += sys.entry_count[k];
    return terms;
}

// The system's nine tables and its forcing on the device
hipError_t sim_upload(DeviceBuffers &buf, const fokl_system &s, SimTables &tab, double *&forcing)
{
    int *norm_src = nullptr, *fac_norm = nullptr, *fac_row = nullptr, *fac_degree = nullptr;
    int4 *entries = nullptr;
    double *norm_lo = nullptr, *norm_span = nullptr, *spline = nullptr, *bern = nullptr;
    hipError_t e;
    if ((e = buf.upload(&norm_src, s.norm_src, (size_t)s.n_norm)) || (e = buf.upload(&norm_lo, s.norm_lo, (size_t)s.n_norm)) ||
        (e = buf.upload(&norm_span, s.norm_span, (size_t)s.n_norm)) || (e = buf.upload(&fac_norm, s.fac_norm, (size_t)s.n_factors)) ||
        (e = buf.upload(&fac_row, s.fac_row, (size_t)s.n_factors)) || (e = buf.upload(&fac_degree, s.fac_degree, (size_t)s.n_factors)) ||
        (e = buf.upload(&entries, s.entries, (size_t)s.n_entries)) ||
        (e = buf.upload(&spline, s.spline_table, (size_t)s.n_spline_rows * SIM_PIECES * 4)) ||
        (e = buf.upload(&bern, s.bern_table, (size_t)s.n_bern_rows * SIM_BERN_WIDTH)) ||
        (e = buf.upload(&forcing, s.forcing, (size_t)s.n_steps * s.n_forcing_cols)))
        return e;
    tab = SimTables{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    return hipSuccess;
}

// host [rows][members] -> device [rows][ld], ld = the members rounded up to whole wavefronts; the padding members hold zeros
hipError_t sim_upload_padded(DeviceBuffers &buf, double **out, const double *host, size_t rows, size_t members, size_t ld)
{
    std::vector<double> padded(rows * ld, 0.0);
    for (size_t r = 0; r < rows; ++r) std::memcpy(padded.data() + r * ld, host + r * members, members * sizeof(double));
    return buf.upload(out, padded.data(), padded.size());
}

// The outputs the three simulate calls share, and what they refuse of them after sim_check
struct SimOutputs {
    int cut;
    double *mean, *bounds, *members;
};

int sim_outputs_check(fokl_ctx *ctx, const std::string &who, const fokl_system &s, const SimOutputs &out)
{
    if (out.bounds && (out.cut < 1 || out.cut >= s.n_members)) return fail(ctx, FOKL_ERR_ARG, who + "bounds need 1 <= cut < n_members");
    if (out.bounds && s.n_members > GI_BAND_MAX_MEMBERS)
        return fail(ctx, FOKL_ERR_ARG, who + "bounds are formed over at most " + std::to_string(GI_BAND_MAX_MEMBERS) +
                                           " members (mean and members have no limit)");
    return FOKL_OK;
}

// The time axis of a simulate call: launches of at most `bound` steps (and of what stays resident: the points of one launch),
// each followed by the band and, where the members are wanted, the transpose with its strided copy; then mean and bounds.
// launch(points, t0, steps, chunk_points, write_first) queues the caller's integration kernel for one chunk;
// flops_per_step: its work per member and step for the kernel timer (0: not known beforehand).
template <class Launch>
int sim_run(fokl_ctx *ctx, const fokl_system &s, size_t ld, int64_t bound, const SimOutputs &out, double flops_per_step,
            DeviceBuffers &buf, Launch launch, int64_t &per_launch, int64_t &launches)
{
    const int n_states = s.n_states, n_members = s.n_members;
    const int64_t n_steps = s.n_steps, n_points = n_steps + 1;
    const size_t E = (size_t)n_members;
    const int64_t resident = ((int64_t)256 << 20) / (int64_t)((size_t)n_states * ld * sizeof(double));
    per_launch = std::max<int64_t>(1, std::min(bound, resident - 1));
    const int chunk_cap = (int)std::min<int64_t>(per_launch + 1, n_points);

    double *d_points = nullptr, *d_mean = nullptr, *d_bounds = nullptr, *d_members = nullptr;
    HIP_TRY(ctx, buf.get(&d_points, (size_t)n_states * chunk_cap * ld));
    HIP_TRY(ctx, buf.get(&d_mean, (size_t)n_states * n_points));
    if (out.bounds) HIP_TRY(ctx, buf.get(&d_bounds, (size_t)n_states * n_points * 2));
    if (out.members) HIP_TRY(ctx, buf.get(&d_members, E * n_states * chunk_cap));

    int npow2 = 2;
    while (npow2 < n_members) npow2 <<= 1;
    const size_t band_lds = out.bounds ? (size_t)npow2 * sizeof(double) : 0;
    HIP_TRY(ctx, lds_opt_in(ensemble_band_kernel, band_lds, GI_BAND_MAX_MEMBERS * sizeof(double)));

    launches = 0;
    for (int64_t t0 = 0, p_first = 0; p_first < n_points;) {
        const int write_first = t0 == 0;
        const int steps = (int)std::min<int64_t>(per_launch, n_steps - t0);
        const int chunk_points = steps + write_first;
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)ld * n_states * (chunk_points + 2.0),
                              (double)ld * steps * flops_per_step);
            HIP_TRY(ctx, launch(d_points, t0, steps, chunk_points, write_first));
            ++launches;
        }
        {
            const int rows = n_states * chunk_points;
            const int band_grid = std::min(rows, cu_count(ctx) * (band_lds > 32 * 1024 ? 1 : 4));
            TimedRegion timed(ctx, FOKL_K_BAND, 8.0 * (double)rows * (E + 3.0), (double)rows * E);
            hipLaunchKernelGGL(ensemble_band_kernel, dim3(band_grid), dim3(GI_BAND_THREADS), band_lds, ctx->stream,
                               d_points, (int64_t)ld, n_members, n_states, chunk_points, n_points, p_first, npow2, out.cut,
                               d_mean, d_bounds);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (out.members) {
            hipLaunchKernelGGL(ensemble_transpose_kernel, dim3((n_members + 31) / 32, (chunk_points + 31) / 32, n_states),
                               dim3(256), 0, ctx->stream, d_points, (int64_t)ld, n_members, n_states, chunk_points,
                               d_members);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy2D(out.members + p_first, (size_t)n_points * sizeof(double), d_members,
                                     (size_t)chunk_points * sizeof(double), (size_t)chunk_points * sizeof(double),
                                     E * n_states, hipMemcpyDeviceToHost));
        }
        t0 += steps;
        p_first += chunk_points;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out.mean, d_mean, (size_t)n_states * n_points * sizeof(double), hipMemcpyDeviceToHost));
    if (out.bounds)
        HIP_TRY(ctx, hipMemcpy(out.bounds, d_bounds, (size_t)n_states * n_points * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return FOKL_OK;
}

}  // namespace

extern "C" int fokl_simulate_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_simulate_report: null argument");
    std::memcpy(out, ctx->simulate_report, sizeof ctx->simulate_report);
    return FOKL_OK;
}

extern "C" int fokl_simulate_ensemble(fokl_ctx *ctx, const fokl_system *system, int cut, double *mean, double *bounds,
                                      double *members, int32_t *first_saturation)
{
    const std::string who = "fokl_simulate_ensemble: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->simulate_report, 0, sizeof ctx->simulate_report);
    if (const int refused = sim_check(ctx, who, system, mean && first_saturation, sim_steps_fit)) return refused;
    const fokl_system &s = *system;
    const SimOutputs out{cut, mean, bounds, members};
    if (const int refused = sim_outputs_check(ctx, who, s, out)) return refused;

    SimSystem sys{};
    int n_bern_factors = 0;
    if (const int refused = sim_plan(ctx, who, s, sys, n_bern_factors)) return refused;
    const size_t lds_rows = (size_t)1 + s.n_factors + (s.n_norm - s.n_norm_forcing) + s.n_coef;
    const size_t lds_bytes = lds_rows * SIM_LANES * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_rows) + " values per member in LDS (1 + factors + "
                                           "normalised states + coefficients), a wavefront's " + std::to_string(SIM_LDS_BUDGET / 1024) +
                                           " KB hold " + std::to_string(SIM_LDS_BUDGET / (SIM_LANES * sizeof(double))));

    const size_t E = (size_t)s.n_members, ld = (E + SIM_LANES - 1) / SIM_LANES * SIM_LANES;
    const std::vector<int32_t> never(ld, -1);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    SimTables tab{};
    int *d_sat = nullptr;
    double *d_coef = nullptr, *d_forcing = nullptr, *d_state = nullptr;
    HIP_TRY(ctx, sim_upload(buf, s, tab, d_forcing));
    HIP_TRY(ctx, sim_upload_padded(buf, &d_coef, s.coef, (size_t)s.n_coef, E, ld));
    HIP_TRY(ctx, sim_upload_padded(buf, &d_state, s.y0, (size_t)s.n_states, E, ld));
    HIP_TRY(ctx, buf.upload(&d_sat, never.data(), never.size()));

    // steps per launch: bounded (no launch of this call runs long); FOKL_SIMULATE_STEPS_PER_LAUNCH overrides (tests: the cut
    // changes no bit of the result)
    const int grid = (int)(ld / SIM_LANES);
    const double flops_per_step = 4.0 * (8.0 * sim_terms_per_stage(sys, s.n_states) + 20.0 * (s.n_factors - s.n_forcing_factors));
    int64_t per_launch = 0, launches = 0;
    const auto launch = [&](double *points, int64_t t0, int steps, int chunk_points, int write_first) {
        return sim_dispatch(s.n_states, [&](auto ns) {
            const auto kernel = simulate_ensemble_kernel<decltype(ns)::value>;
            if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, tab.norm_src, tab.norm_lo,
                               tab.norm_span, tab.fac_norm, tab.fac_row, tab.fac_degree, tab.entries, tab.spline, tab.bern,
                               (const double *)d_coef, (const double *)d_forcing, d_state, d_sat, points, (int64_t)ld, t0, steps,
                               chunk_points, write_first);
            return hipGetLastError();
        });
    };
    if (const int failed = sim_run(ctx, s, ld, env_int("FOKL_SIMULATE_STEPS_PER_LAUNCH", 512), out, flops_per_step, buf, launch,
                                   per_launch, launches))
        return failed;
    HIP_TRY(ctx, hipMemcpy(first_saturation, d_sat, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t *rep = ctx->simulate_report;
    rep[0] = s.n_states;
    rep[1] = s.n_members;
    rep[2] = grid;
    rep[3] = (int64_t)lds_bytes;
    rep[4] = launches;
    rep[5] = s.n_factors - n_bern_factors;
    rep[6] = n_bern_factors;
    rep[7] = per_launch;
    return FOKL_OK;
}

// GP_Integrate over an ensemble (textually included by fokl_hip.hip): one Runge-Kutta integration per posterior draw /
// initial state, all members at once, and per (state, time point) the mean and the order-statistic bounds over members.
//
// The arithmetic of one member is fokl_integrate.cpp's, operation for operation and in its order (input routing, the
// 498-interval evaluation of the 499-piece table, the clamp of normalised states to [0, 1], the saturation rule of the
// four stages, one forcing row per step, terms summed left to right) except that a cubic's X**2 and X**3 are products
// here and libm pow there (<= 1 ulp per cubic).  Compiled under the tree's -ffp-contract=off: nothing is fused.
//
// integrate_ensemble_kernel: one lane per member, one wavefront per workgroup (1 000 members are 16 wavefronts: what binds
// is the latency of a member's dependent chain, so the wavefronts are spread over CUs, not packed).  What is the same for
// every member -- routing, term lists, bounds, forcing -- is wave-uniform: kernel arguments and scalar loads.  What is a
// member's own sits in LDS as [item][lane], read and written by its own lane only (no barriers): the coefficients
// (uploaded as [coefficient][member], one coalesced run each, staged once per launch) and the values of the distinct
// (input, order) cubics, evaluated once per stage and shared by every term of every state's model.  A term is one
// 16-byte entry {slot, slot, slot, coefficient}: slot 0 holds 1.0, so a term with fewer than three factors multiplies by
// exact ones and a term with more continues in the next entry (coefficient -1) -- the term loop has no inner loop and
// no data-dependent branch.  The spline table holds only the orders some model uses, as [order][piece][4]: one 32-byte
// run per evaluation, gathered through L2.  Stage vectors are registers: the kernel is unrolled over the number of
// states (GI_MAX_STATES instantiations; more states are refused).
//
// The time axis is cut into launches of a bounded number of steps; the state is carried in device memory in between and
// a launch writes its points as [state][point][member] (coalesced here, and a (state, point) row is contiguous for
// the band kernel).
//
// ensemble_band_kernel: one workgroup per (state, point) row: the mean as 256 strided partial sums combined by a fixed
// tree (bitwise reproducible), and for the bounds the row sorted in LDS (bitonic network over the next power of two,
// padded with +inf) in numpy's order, in which a NaN member counts as the largest value, above +inf.  A `>` is no order
// once a NaN is in the row -- the network then leaves even the finite values out of place -- so a NaN enters the list as
// +inf and is counted: with n of them, sorted[k] is NaN for k >= E - n and the list's value below (the values that stand
// in for the NaN sit at the top, level with a member's own +inf).  sorted[cut] and sorted[E - cut] are then order
// statistics of the stored values, equal to np.sort's on the returned members: the upper bound is NaN once `cut` members
// are NaN, the lower one once E - cut are, and the mean is NaN with the first NaN member.  A row without NaN is sorted as
// it always was.  E <= GI_BAND_MAX_MEMBERS (16 384 values = 128 KB of LDS); bounds over more are refused.

namespace fokl {

constexpr int GI_MAX_STATES = 4;
constexpr int GI_LANES = 64;
constexpr int GI_PIECES = 499;               // pieces per order in the table; 498 intervals are evaluated (GI:103-131)
constexpr int GI_BAND_THREADS = 256;
constexpr int GI_BAND_MAX_MEMBERS = 16384;
constexpr size_t GI_LDS_BUDGET = 144 * 1024;

struct GiSystem {
    int n_forcing_factors;                   // factors [0, n_forcing_factors) read the forcing row: once per step
    int n_factors;                           // the others read a state: once per stage
    int n_coef;
    int n_other;
    int entry_begin[GI_MAX_STATES];          // model k: entries [entry_begin[k], entry_begin[k] + entry_count[k])
    int entry_count[GI_MAX_STATES];
    int constant[GI_MAX_STATES];             // index of betas[k][0] among the coefficients
    double lo[GI_MAX_STATES], hi[GI_MAX_STATES];
    double h;
};

// spline_value() of fokl_integrate.cpp.  The piece is clamped on both sides: for x in [0, 1] that is the reference's
// "498 -> 497"; beyond (a forcing value outside its normalisation, a NaN) the host clamps the same way: the outermost cubic
// is extended, a NaN takes piece 0 and gives NaN.
__device__ __forceinline__ double gi_cubic(const double *__restrict__ table, int order_slot, double x)
{
    int piece = (int)floor(x * 498.0);
    piece = min(max(piece, 0), 497);
    const double r = 1.0 / 498.0;
    const double xmin = r * (double)piece;
    const double X = (x - xmin) / r;
    const double2 *c = reinterpret_cast<const double2 *>(table + ((size_t)order_slot * GI_PIECES + piece) * 4);
    const double2 c01 = c[0], c23 = c[1];
    return c01.x + c01.y * X + c23.x * (X * X) + c23.y * (X * X * X);
}

// h * model_k(at) for every state k, zeroed where `at` sits on a bound and the slope points outwards
template <int NS>
__device__ __forceinline__ void gi_stage(const GiSystem &sys, const int *__restrict__ fac_src,
                                         const int *__restrict__ fac_ord, const int4 *__restrict__ entries,
                                         const double *__restrict__ table, double *xn, double *fac, const double *cf,
                                         const double (&at)[NS], double (&dy)[NS])
{
    // the normalised states go through LDS: a factor picks its input by a run-time (wave-uniform) index, and a register
    // array indexed that way would live in scratch
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double v = (at[j] - sys.lo[j]) / (sys.hi[j] - sys.lo[j]);
        if (v > 1.0) v = 1.0;
        if (v < 0.0) v = 0.0;
        xn[j * GI_LANES] = v;
    }
    // four cubics at a time, their inputs read before and their values stored after: four table gathers in flight
    int f = sys.n_forcing_factors;
    for (; f + 4 <= sys.n_factors; f += 4) {
        double x[4], v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = xn[fac_src[f + q] * GI_LANES];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = gi_cubic(table, fac_ord[f + q], x[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) fac[(f + 1 + q) * GI_LANES] = v[q];
    }
    for (; f < sys.n_factors; ++f) fac[(f + 1) * GI_LANES] = gi_cubic(table, fac_ord[f], xn[fac_src[f] * GI_LANES]);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int4 *ent = entries + sys.entry_begin[k];
        double delta = 0.0, phi = 1.0;
#pragma unroll 4
        for (int t = 0; t < sys.entry_count[k]; ++t) {
            const int4 d = ent[t];
            phi = phi * fac[d.x * GI_LANES];
            phi = phi * fac[d.y * GI_LANES];
            phi = phi * fac[d.z * GI_LANES];
            const bool ends = d.w >= 0;                                // wave-uniform
            const double with = delta + cf[max(d.w, 0) * GI_LANES] * phi;
            delta = ends ? with : delta;
            phi = ends ? 1.0 : phi;
        }
        double s = (delta + cf[sys.constant[k] * GI_LANES]) * sys.h;
        if (at[k] >= sys.hi[k] && s > 0) s = 0;
        if (at[k] <= sys.lo[k] && s < 0) s = 0;
        dy[k] = s;
    }
}

// Steps [t0, t0 + steps) of every member.  state [NS][ld] in / out; points [NS][chunk_points][ld]: with write_first the
// state before the first step goes to point 0 and step s to point s + 1, otherwise step s to point s.  ld = members
// rounded up to 64 = 64 * gridDim.x: every lane owns a column of every buffer (the padding members integrate zeros).
template <int NS>
__global__ __launch_bounds__(GI_LANES) void integrate_ensemble_kernel(GiSystem sys, const int *__restrict__ fac_src,
                                                                      const int *__restrict__ fac_ord,
                                                                      const int4 *__restrict__ entries,
                                                                      const double *__restrict__ table,
                                                                      const double *__restrict__ coef,
                                                                      const double *__restrict__ forcing,
                                                                      double *__restrict__ state,
                                                                      double *__restrict__ points, int64_t ld,
                                                                      int64_t t0, int steps, int chunk_points,
                                                                      int write_first)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * GI_LANES + lane;
    double *fac = lds + lane;                                          // [1 + n_factors][64]: slot 0 is 1.0
    double *xn = lds + (size_t)(1 + sys.n_factors) * GI_LANES + lane;  // [NS][64]: the stage's normalised states
    double *cf = xn + NS * GI_LANES;                                   // [n_coef][64]
    fac[0] = 1.0;
    for (int c = 0; c < sys.n_coef; ++c) cf[c * GI_LANES] = coef[(size_t)c * ld + e];
    double y[NS], at[NS], dy[NS] = {}, sum[NS] = {};
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = state[(size_t)j * ld + e];
    if (write_first) {
#pragma unroll
        for (int j = 0; j < NS; ++j) points[(size_t)j * chunk_points * ld + e] = y[j];
    }
    double *out = points + (write_first ? ld : 0) + e;
    for (int s = 0; s < steps; ++s) {
        const double *row = forcing + (size_t)(t0 + s) * sys.n_other;  // the same row serves the four stages
        for (int f = 0; f < sys.n_forcing_factors; ++f)
            fac[(f + 1) * GI_LANES] = gi_cubic(table, fac_ord[f], row[-(fac_src[f] + 1)]);
        // the four stages as one loop body (a quarter of the code): y, y + dy1 / 2, y + dy2 / 2, y + dy3, and
        // dy1 + 2 dy2 + 2 dy3 + dy4 summed left to right -- dy * 0.5 is dy / 2 and 1.0 * dy is dy, bit for bit
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            const double reach = st == 3 ? 1.0 : 0.5, weight = (st == 1 || st == 2) ? 2.0 : 1.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) at[j] = st == 0 ? y[j] : y[j] + dy[j] * reach;
            gi_stage<NS>(sys, fac_src, fac_ord, entries, table, xn, fac, cf, at, dy);
#pragma unroll
            for (int j = 0; j < NS; ++j) sum[j] = st == 0 ? dy[j] : sum[j] + weight * dy[j];
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            y[j] += sum[j] / 6;
            out[((size_t)j * chunk_points + s) * ld] = y[j];
        }
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) state[(size_t)j * ld + e] = y[j];
}

// Rows of `points` ([n_states][chunk_points][ld], the first `members` values of a row count): row (s, q) -> time point
// p_first + q of state s.  mean [n_states][n_points]; bounds [n_states][n_points][2] or nullptr (then no LDS is used
// beyond the 256 partial sums).  npow2 = members rounded up to a power of two (>= 2).
__global__ __launch_bounds__(GI_BAND_THREADS) void ensemble_band_kernel(const double *__restrict__ points, int64_t ld,
                                                                        int members, int n_states, int chunk_points,
                                                                        int64_t n_points, int64_t p_first, int npow2,
                                                                        int cut, double *__restrict__ mean,
                                                                        double *__restrict__ bounds)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double partial[GI_BAND_THREADS];
    __shared__ int nan_count[GI_BAND_THREADS];
    const int tid = threadIdx.x;
    const int n_rows = n_states * chunk_points;
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const double *src = points + (size_t)r * ld;
        const int64_t dst = (int64_t)(r / chunk_points) * n_points + p_first + r % chunk_points;
        double sum = 0.0;
        for (int i = tid; i < members; i += GI_BAND_THREADS) sum += src[i];
        partial[tid] = sum;
        if (bounds) {
            int nans = 0;                                              // a NaN member enters the list as +inf and is counted
            for (int i = tid; i < npow2; i += GI_BAND_THREADS) {
                const double v = i < members ? src[i] : INFINITY;
                nans += v != v;
                lds[i] = v != v ? INFINITY : v;
            }
            nan_count[tid] = nans;
        }
        __syncthreads();
        for (int half = GI_BAND_THREADS / 2; half > 0; half >>= 1) {
            if (tid < half) {
                partial[tid] += partial[tid + half];
                if (bounds) nan_count[tid] += nan_count[tid + half];
            }
            __syncthreads();
        }
        if (tid == 0) mean[dst] = partial[0] / (double)members;
        if (bounds) {
            for (int size = 2; size <= npow2; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int i = tid; i < (npow2 >> 1); i += GI_BAND_THREADS) {
                        const int a = 2 * i - (i & (stride - 1)), b = a + stride;    // a has bit `stride` clear
                        const bool up = (a & size) == 0;
                        const double va = lds[a], vb = lds[b];
                        if ((va > vb) == up) {
                            lds[a] = vb;
                            lds[b] = va;
                        }
                    }
                    __syncthreads();
                }
            if (tid == 0) {                                            // sorted[k] is NaN from k = members - (NaN members) on
                const int first_nan = members - nan_count[0];
                bounds[2 * dst] = cut < first_nan ? lds[cut] : NAN;
                bounds[2 * dst + 1] = members - cut < first_nan ? lds[members - cut] : NAN;
            }
        }
        __syncthreads();
    }
}

// points [n_states][chunk_points][ld] -> out [members][n_states][chunk_points]: the public layout of `members`, for the
// points of one launch (32 x 32 tiles through LDS: reads run along members, writes along points).
__global__ __launch_bounds__(256) void ensemble_transpose_kernel(const double *__restrict__ points, int64_t ld, int members,
                                                                 int n_states, int chunk_points, double *__restrict__ out)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // 32 x 8
    const int s = blockIdx.z;
    const int q0 = blockIdx.y * 32, e0 = blockIdx.x * 32;
    for (int i = ty; i < 32; i += 8) {
        const int q = q0 + i, e = e0 + tx;
        tile[i][tx] = (q < chunk_points && e < members) ? points[((size_t)s * chunk_points + q) * ld + e] : 0.0;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int e = e0 + i, q = q0 + tx;
        if (e < members && q < chunk_points) out[((size_t)e * n_states + s) * chunk_points + q] = tile[tx][i];
    }
}

}  // namespace fokl

namespace {

template <int NS>
void gi_launch(fokl_ctx *ctx, int grid, size_t lds_bytes, const GiSystem &sys, const int *fac_src, const int *fac_ord,
               const int4 *entries, const double *table, const double *coef, const double *forcing, double *state,
               double *points, int64_t ld, int64_t t0, int steps, int chunk_points, int write_first)
{
    hipLaunchKernelGGL(integrate_ensemble_kernel<NS>, dim3(grid), dim3(GI_LANES), lds_bytes, ctx->stream, sys, fac_src,
                       fac_ord, entries, table, coef, forcing, state, points, ld, t0, steps, chunk_points, write_first);
}

template <int NS>
hipError_t gi_allow_lds(size_t lds_bytes)
{
    if (lds_bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(integrate_ensemble_kernel<NS>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)GI_LDS_BUDGET);
}

}  // namespace

extern "C" int fokl_gp_integrate_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_gp_integrate_report: null argument");
    std::memcpy(out, ctx->integrate_report, sizeof ctx->integrate_report);
    return FOKL_OK;
}

extern "C" int fokl_gp_integrate_ensemble(fokl_ctx *ctx, int n_members, int n_states, int n_other, int64_t n_steps,
                                          const double *const *betas, const int32_t *betas_per_member,
                                          const int32_t *const *mtx, const int32_t *mtx_rows, const int32_t *mtx_cols,
                                          const int32_t *const *source, const int32_t *n_source, const double *forcing,
                                          const double *norms, const double *spline_table, int n_basis, int width,
                                          double h, const double *y0, int y0_per_member, int cut, double *mean,
                                          double *bounds, double *members)
{
    const char *who = "fokl_gp_integrate_ensemble: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, std::string(who) + "null context");
    std::memset(ctx->integrate_report, 0, sizeof ctx->integrate_report);
    if (n_members <= 0 || n_states <= 0 || n_other < 0 || n_steps < 0 || !betas || !betas_per_member || !mtx ||
        !mtx_rows || !mtx_cols || !source || !n_source || !norms || !spline_table || !y0 || !mean ||
        (n_other > 0 && !forcing))
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + "null pointer or empty system");
    if (width != GI_PIECES)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + "the spline table must be 499 pieces wide");
    if (n_states > GI_MAX_STATES)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + std::to_string(n_states) + " states, the kernel is built for at most " +
                                           std::to_string(GI_MAX_STATES));
    if (n_steps + 1 > (int64_t)1 << 30) return fail(ctx, FOKL_ERR_ARG, std::string(who) + "too many steps");
    if (bounds && (cut < 1 || cut >= n_members))
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + "bounds need 1 <= cut < n_members");
    if (bounds && n_members > GI_BAND_MAX_MEMBERS)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + "bounds are formed over at most " +
                                           std::to_string(GI_BAND_MAX_MEMBERS) + " members (mean and members have no limit)");

    // ---- the system as the kernel reads it: distinct (input, order) factors, packed orders, 16-byte term entries ----
    GiSystem sys{};
    std::vector<int32_t> order_slot((size_t)n_basis + 1, -1), used_orders;
    std::map<std::pair<int, int>, int> factor_of;                  // (source, order) -> provisional index
    std::vector<std::pair<int, int>> factors;
    size_t n_coef = 0;
    for (int k = 0; k < n_states; ++k) {
        if (mtx_rows[k] < 0 || mtx_cols[k] < 0 || (mtx_rows[k] > 0 && mtx_cols[k] > 0 && !mtx[k]) || !betas[k] ||
            (n_source[k] > 0 && !source[k]))
            return fail(ctx, FOKL_ERR_ARG, std::string(who) + "null pointer or negative size in a model");
        if (n_source[k] < mtx_cols[k])
            return fail(ctx, FOKL_ERR_ARG, std::string(who) + "a model has more input columns than inputs are routed to it");
        for (int i = 0; i < n_source[k]; ++i) {
            const int s = source[k][i];
            if (s >= n_states || (s < 0 && -(s + 1) >= n_other))
                return fail(ctx, FOKL_ERR_ARG, std::string(who) + "input routing out of range");
        }
        for (int i = 0; i < mtx_rows[k] * mtx_cols[k]; ++i) {
            const int order = mtx[k][i];
            if (order < 0 || order > n_basis)
                return fail(ctx, FOKL_ERR_ARG, std::string(who) + "basis order outside the spline table");
            if (order == 0) continue;
            if (order_slot[order] < 0) {
                order_slot[order] = (int)used_orders.size();
                used_orders.push_back(order);
            }
            const auto key = std::make_pair((int)source[k][i % mtx_cols[k]], order);
            if (factor_of.emplace(key, (int)factors.size()).second) factors.push_back(key);
        }
        n_coef += (size_t)mtx_rows[k] + 1;
    }
    // forcing factors first (they are evaluated once per step), first-seen order otherwise
    std::vector<int> slot_of(factors.size());
    std::vector<int32_t> fac_src, fac_ord;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t f = 0; f < factors.size(); ++f)
            if ((factors[f].first < 0) == (pass == 0)) {
                slot_of[f] = (int)fac_src.size() + 1;              // slot 0 holds 1.0
                fac_src.push_back(factors[f].first);
                fac_ord.push_back(order_slot[factors[f].second]);
            }
    sys.n_factors = (int)factors.size();
    sys.n_forcing_factors = 0;
    for (const auto &f : factors) sys.n_forcing_factors += f.first < 0;
    sys.n_coef = (int)n_coef;
    sys.n_other = n_other;
    sys.h = h;
    std::vector<int32_t> entries;                                  // int4 each: three slots, coefficient index or -1
    int coef_at = 0;
    for (int k = 0; k < n_states; ++k) {
        sys.lo[k] = norms[k];
        sys.hi[k] = norms[n_states + k];
        sys.constant[k] = coef_at;
        sys.entry_begin[k] = (int)(entries.size() / 4);
        for (int i = 0; i < mtx_rows[k]; ++i) {
            int filled = 0;
            int32_t ent[4] = {0, 0, 0, -1};
            for (int j = 0; j < mtx_cols[k]; ++j) {
                const int order = mtx[k][i * mtx_cols[k] + j];
                if (order == 0) continue;
                if (filled == 3) {                                 // a fourth factor: the product continues in the next entry
                    entries.insert(entries.end(), ent, ent + 4);
                    ent[0] = ent[1] = ent[2] = 0;
                    filled = 0;
                }
                ent[filled++] = slot_of[factor_of[std::make_pair((int)source[k][j], order)]];
            }
            ent[3] = coef_at + 1 + i;
            entries.insert(entries.end(), ent, ent + 4);
        }
        sys.entry_count[k] = (int)(entries.size() / 4) - sys.entry_begin[k];
        coef_at += mtx_rows[k] + 1;
    }
    const size_t lds_bytes = (size_t)(1 + sys.n_factors + n_states + sys.n_coef) * GI_LANES * sizeof(double);
    if (lds_bytes > GI_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, std::string(who) + "the models' coefficients and factors (" +
                                           std::to_string(sys.n_coef + sys.n_factors) + ") do not fit a wavefront's LDS (" +
                                           std::to_string(GI_LDS_BUDGET / (GI_LANES * sizeof(double)) - 1 - n_states) + ")");

    const int64_t n_points = n_steps + 1;
    const size_t E = (size_t)n_members, ld = (E + GI_LANES - 1) / GI_LANES * GI_LANES;
    std::vector<double> table(used_orders.size() * GI_PIECES * 4);
    for (size_t o = 0; o < used_orders.size(); ++o) {
        const double *c = spline_table + (size_t)(used_orders[o] - 1) * 4 * width;
        for (int p = 0; p < GI_PIECES; ++p)
            for (int q = 0; q < 4; ++q) table[(o * GI_PIECES + p) * 4 + q] = c[(size_t)q * width + p];
    }
    std::vector<double> coef(n_coef * ld, 0.0), state((size_t)n_states * ld, 0.0);
    coef_at = 0;
    for (int k = 0; k < n_states; ++k) {
        const size_t nb = (size_t)mtx_rows[k] + 1;
        for (size_t c = 0; c < nb; ++c) {
            double *dst = coef.data() + (coef_at + c) * ld;
            if (betas_per_member[k])
                for (size_t e = 0; e < E; ++e) dst[e] = betas[k][e * nb + c];
            else
                std::fill(dst, dst + E, betas[k][c]);
        }
        coef_at += (int)nb;
        for (size_t e = 0; e < E; ++e) state[(size_t)k * ld + e] = y0[(y0_per_member ? e * n_states : 0) + k];
    }

    // steps per launch: bounded (no launch of this call runs long, the points of one launch are what is resident);
    // FOKL_INTEGRATE_STEPS_PER_LAUNCH overrides (tests: the cut changes no bit of the result)
    int64_t per_launch = env_int("FOKL_INTEGRATE_STEPS_PER_LAUNCH", 512);
    const int64_t resident = ((int64_t)256 << 20) / (int64_t)((size_t)n_states * ld * sizeof(double));
    per_launch = std::max<int64_t>(1, std::min(per_launch, resident - 1));
    const int chunk_cap = (int)std::min<int64_t>(per_launch + 1, n_points);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    int *d_src = nullptr, *d_ord = nullptr;
    int4 *d_entries = nullptr;
    double *d_table = nullptr, *d_coef = nullptr, *d_forcing = nullptr, *d_state = nullptr, *d_points = nullptr,
           *d_mean = nullptr, *d_bounds = nullptr, *d_members = nullptr;
    HIP_TRY(ctx, buf.upload(&d_src, fac_src.data(), fac_src.size()));
    HIP_TRY(ctx, buf.upload(&d_ord, fac_ord.data(), fac_ord.size()));
    HIP_TRY(ctx, buf.upload(&d_entries, entries.data(), entries.size() / 4));
    HIP_TRY(ctx, buf.upload(&d_table, table.data(), table.size()));
    HIP_TRY(ctx, buf.upload(&d_coef, coef.data(), coef.size()));
    HIP_TRY(ctx, buf.upload(&d_forcing, forcing, (size_t)n_steps * n_other));
    HIP_TRY(ctx, buf.upload(&d_state, state.data(), state.size()));
    HIP_TRY(ctx, buf.get(&d_points, (size_t)n_states * chunk_cap * ld));
    HIP_TRY(ctx, buf.get(&d_mean, (size_t)n_states * n_points));
    if (bounds) HIP_TRY(ctx, buf.get(&d_bounds, (size_t)n_states * n_points * 2));
    if (members) HIP_TRY(ctx, buf.get(&d_members, E * n_states * chunk_cap));

    hipError_t lds_ok = hipSuccess;
    switch (n_states) {
    case 1: lds_ok = gi_allow_lds<1>(lds_bytes); break;
    case 2: lds_ok = gi_allow_lds<2>(lds_bytes); break;
    case 3: lds_ok = gi_allow_lds<3>(lds_bytes); break;
    default: lds_ok = gi_allow_lds<4>(lds_bytes); break;
    }
    HIP_TRY(ctx, lds_ok);
    int npow2 = 2;
    while (npow2 < n_members) npow2 <<= 1;
    const size_t band_lds = bounds ? (size_t)npow2 * sizeof(double) : 0;
    if (band_lds > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(ensemble_band_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, GI_BAND_MAX_MEMBERS * (int)sizeof(double)));

    const int grid = (int)(ld / GI_LANES);
    double terms_per_stage = 0.0;
    for (int k = 0; k < n_states; ++k) terms_per_stage += sys.entry_count[k];
    int64_t launches = 0, first_rows = 0, first_band_grid = 0;
    for (int64_t t0 = 0, p_first = 0; p_first < n_points;) {
        const int write_first = t0 == 0;
        const int steps = (int)std::min<int64_t>(per_launch, n_steps - t0);
        const int chunk_points = steps + write_first;
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)ld * n_states * (chunk_points + 2.0),
                              (double)ld * steps * 4.0 * (8.0 * terms_per_stage + 20.0 * (sys.n_factors - sys.n_forcing_factors)));
            switch (n_states) {
            case 1: gi_launch<1>(ctx, grid, lds_bytes, sys, d_src, d_ord, d_entries, d_table, d_coef, d_forcing, d_state, d_points, (int64_t)ld, t0, steps, chunk_points, write_first); break;
            case 2: gi_launch<2>(ctx, grid, lds_bytes, sys, d_src, d_ord, d_entries, d_table, d_coef, d_forcing, d_state, d_points, (int64_t)ld, t0, steps, chunk_points, write_first); break;
            case 3: gi_launch<3>(ctx, grid, lds_bytes, sys, d_src, d_ord, d_entries, d_table, d_coef, d_forcing, d_state, d_points, (int64_t)ld, t0, steps, chunk_points, write_first); break;
            default: gi_launch<4>(ctx, grid, lds_bytes, sys, d_src, d_ord, d_entries, d_table, d_coef, d_forcing, d_state, d_points, (int64_t)ld, t0, steps, chunk_points, write_first); break;
            }
            HIP_TRY(ctx, hipGetLastError());
        }
        {
            const int rows = n_states * chunk_points;
            const int band_grid = std::min(rows, cu_count(ctx) * (band_lds > 32 * 1024 ? 1 : 4));
            TimedRegion timed(ctx, FOKL_K_BAND, 8.0 * (double)rows * (E + 3.0), (double)rows * E);
            hipLaunchKernelGGL(ensemble_band_kernel, dim3(band_grid), dim3(GI_BAND_THREADS), band_lds, ctx->stream,
                               d_points, (int64_t)ld, n_members, n_states, chunk_points, n_points, p_first, npow2, cut,
                               d_mean, d_bounds);
            HIP_TRY(ctx, hipGetLastError());
            if (launches++ == 0) {
                first_rows = rows;
                first_band_grid = band_grid;
            }
        }
        if (members) {
            hipLaunchKernelGGL(ensemble_transpose_kernel, dim3((n_members + 31) / 32, (chunk_points + 31) / 32, n_states),
                               dim3(256), 0, ctx->stream, d_points, (int64_t)ld, n_members, n_states, chunk_points,
                               d_members);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy2D(members + p_first, (size_t)n_points * sizeof(double), d_members,
                                     (size_t)chunk_points * sizeof(double), (size_t)chunk_points * sizeof(double),
                                     E * n_states, hipMemcpyDeviceToHost));
        }
        t0 += steps;
        p_first += chunk_points;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(mean, d_mean, (size_t)n_states * n_points * sizeof(double), hipMemcpyDeviceToHost));
    if (bounds)
        HIP_TRY(ctx, hipMemcpy(bounds, d_bounds, (size_t)n_states * n_points * 2 * sizeof(double), hipMemcpyDeviceToHost));
    int64_t *rep = ctx->integrate_report;
    rep[0] = n_states;
    rep[1] = n_members;
    rep[2] = grid;
    rep[3] = (int64_t)lds_bytes;
    rep[4] = launches;
    rep[5] = per_launch;
    rep[6] = (int64_t)band_lds;
    rep[7] = first_rows;
    rep[8] = first_band_grid;
    rep[9] = cu_count(ctx);
    return FOKL_OK;
}

// dynamics.control (textually included by fokl_hip.hip, after fokl_assimilate_device.inc): which inputs make the states of a
// system of fitted models do what is wanted -- one bounded least-squares solve per (posterior draw, start), projected
// Gauss-Newton with the Jacobian from forward sensitivities of the Runge-Kutta scheme as executed.
//
// The statement of the arithmetic is dynamics.control_host (fokl_gpy_amd/dynamics.py, module docstring); this file follows it
// operation for operation and in its order: only + - * /, sqrt and comparisons, compiled under the tree's
// -ffp-contract=off.  The values of a step are simulate_ensemble_kernel's (sim_clamp / sim_cubic / sim_horner / sim_stage of
// fokl_simulate_device.inc; ctl_cubic / ctl_horner / ctl_stage are their twins that carry a tangent and form the value by
// the same operations), so a trajectory under the returned controls is dynamics.simulate_host's bit for bit.
//
// control_iterate_kernel<NS>: one wavefront per workgroup and solve; one launch is one iteration of every solve that is
// still running (a finished solve returns at once).  Iterate, status and counters live in device memory between launches.
//   tangent pass   lane d < D carries the nominal trajectory (wave-uniform, computed in every lane) and direction d's
//                  tangent; states and tangents are registers.  Per residual g_d += 2 w r t_d needs no other lane, and
//                  H[d][d'] += (2 w t_d) t_d' reads the 64 tangents from the exchange row
//   stop test      the projected-gradient maximum is the xor butterfly (asm_max)
//   Cholesky       lane = row, in place in H; column entries and pivots are read from LDS at wave-uniform addresses
//   trial pass     lane i < 31 tries P(z + 2^-i d), lane 32 + i tries P(z - 2^-i g): simulate's step (sim_stage with the
//                  draw's coefficients once) with the controlled columns' forcing factors from the lane's own trial point;
//                  each lane accumulates its own F; the first passing lane comes from a ballot
// control_trajectory_kernel<NS> is the trial pass with every lane at the accepted point and lane 0 storing.
// The parts of an iteration are __device__ functions (ctl_tangent_pass, ctl_stop_code, ctl_newton_direction, ctl_trial_points,
// ctl_first_passing) that the kernels of dynamics.control_pooled (fokl_control_pooled_device.inc) call as well.
// LDS, as [item][lane] unless noted: values of slot 0 (1.0), the factors and the stage's normalised states; their tangents;
// four rows of 64 (exchange, z, g, direction); row d of H as [D][64] (after the factorisation: the trial points, lane =
// trial); the draw's coefficients ONCE ([coefficient]).  bytes = (2 (1 + factors + normalised states) + 4 + D) x 64 x 8 +
// n_coef x 8.  No atomics, plain stores: the same arguments give the same bits, and draw e alone is draw e of the full run.

namespace fokl {

constexpr int CTL_MAX_D = 32;
constexpr int CTL_MAX_STEPS = 4096;
constexpr int CTL_TRIALS = 31;                 // alpha = 1, 1/2, ..., 2^-30
constexpr int CTL_MAX_SOLVES = 1 << 20;
constexpr double CTL_ARMIJO = 1e-4, CTL_NOISE = 1e-13, CTL_PIVOT_FLOOR = 1e-8;
enum { CTL_CONVERGED = 0, CTL_ITERATION_LIMIT = 1, CTL_NON_FINITE = 2, CTL_STALLED = 3 };

struct CtlProblem {
    int D, n_controls, segments, n_starts, n_draws, n_steps, has_previous, max_iter;
    double lo[CTL_MAX_D], width[CTL_MAX_D], move[CTL_MAX_D], prev[CTL_MAX_D];
    double wt[SIM_MAX_STATES], term[SIM_MAX_STATES], lim_lo[SIM_MAX_STATES], lim_hi[SIM_MAX_STATES];
    double hl, tol;
};

struct CtlTables {
    const int *norm_control;                   // [n_norm_forcing]: the control a forcing input reads, -1 a forcing column
    const int *seg_first;                      // [segments]: the first step of every hold
    const double *ref;                         // [NS][n_steps + 1], NaN: not tracked
};

// sim_cubic with d value / d v: the value by the same operations (dynamics._factor_dual)
__device__ __forceinline__ double ctl_cubic(const double *__restrict__ table, int row, double v, double &slope)
{
    double p = ceil(v * 499.0);
    p = p + (p == 0.0 ? 1.0 : 0.0);
    p = p - 1.0;
    const double s = 499.0 * v - p;
    const int piece = (p >= 0.0 && p <= (double)(SIM_PIECES - 1)) ? (int)p : 0;
    const double2 *c = reinterpret_cast<const double2 *>(table + ((size_t)row * SIM_PIECES + piece) * 4);
    const double2 c01 = c[0], c23 = c[1];
    const double q2 = c23.x + s * c23.y;
    const double q1 = c01.y + s * q2;
    const double d1 = q2 + s * c23.y;
    const double d0 = q1 + s * d1;
    slope = 499.0 * d0;
    return c01.x + s * q1;
}

__device__ __forceinline__ double ctl_horner(const double *__restrict__ c, int degree, double v, double &slope)
{
    double value = c[degree], d = 0.0;
    for (int k = degree - 1; k >= 0; --k) {
        d = d * v + value;
        value = value * v + c[k];
    }
    slope = d;
    return value;
}

__device__ __forceinline__ double ctl_clip01(double x)
{
    x = x < 0.0 ? 0.0 : x;
    return x > 1.0 ? 1.0 : x;
}

// sim_stage<NS, 1> with tangents: txn / tfac are laid out as xn / fac
template <int NS>
__device__ __forceinline__ void ctl_stage(const SimSystem &sys, const SimTables &tab, double *xn, double *fac, double *txn,
                                          double *tfac, const double *cf, const double (&at)[NS], const double (&tat)[NS],
                                          double (&dy)[NS], double (&tdy)[NS])
{
#pragma unroll
    for (int j = 0; j < NS; ++j)
        for (int n = sys.norm_begin[j]; n < sys.norm_begin[j + 1]; ++n) {
            bool clamped = false;
            const double v = sim_clamp((at[j] - tab.norm_lo[n]) / tab.norm_span[n], clamped);
            xn[(n - sys.n_norm_forcing) * SIM_LANES] = v;
            txn[(n - sys.n_norm_forcing) * SIM_LANES] = clamped ? 0.0 : tat[j] / tab.norm_span[n];
        }
    for (int f = sys.n_forcing_factors; f < sys.n_factors; ++f) {
        const int n = (tab.fac_norm[f] - sys.n_norm_forcing) * SIM_LANES;
        double slope;
        fac[(f + 1) * SIM_LANES] = f < sys.n_state_splines_end
                                       ? ctl_cubic(tab.spline, tab.fac_row[f], xn[n], slope)
                                       : ctl_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], xn[n], slope);
        tfac[(f + 1) * SIM_LANES] = slope * txn[n];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int4 *ent = tab.entries + sys.entry_begin[k];
        double delta = 0.0, phi = 1.0, tdelta = 0.0, tphi = 0.0;
        for (int t = 0; t < sys.entry_count[k]; ++t) {
            const int4 d = ent[t];
            tphi = tphi * fac[d.x * SIM_LANES] + phi * tfac[d.x * SIM_LANES];
            phi = phi * fac[d.x * SIM_LANES];
            tphi = tphi * fac[d.y * SIM_LANES] + phi * tfac[d.y * SIM_LANES];
            phi = phi * fac[d.y * SIM_LANES];
            tphi = tphi * fac[d.z * SIM_LANES] + phi * tfac[d.z * SIM_LANES];
            phi = phi * fac[d.z * SIM_LANES];
            const bool ends = d.w >= 0;                                 // wave-uniform
            const double c = cf[max(d.w, 0)];
            const double with = delta + c * phi, twith = tdelta + c * tphi;
            delta = ends ? with : delta;
            tdelta = ends ? twith : tdelta;
            phi = ends ? 1.0 : phi;
            tphi = ends ? 0.0 : tphi;
        }
        double s = (delta + cf[sys.constant[k]]) * sys.h, ts = tdelta * sys.h;
        const bool outwards = (at[k] >= sys.box_hi[k] && s > 0) || (at[k] <= sys.box_lo[k] && s < 0);
        if (outwards) {
            s = 0;
            ts = 0;
        }
        dy[k] = s;
        tdy[k] = ts;
    }
}

// One residual a - b of weight w with tangent t in this lane (`act`: wave-uniform; an idle limit adds nothing)
__device__ __forceinline__ void ctl_residual(double weight, double a, double b, double t, bool act, int D, int lane, double *ex,
                                             double *Hl, double &F, double &noise, double &g)
{
    if (!act) return;
    const double r = a - b, mag = fabs(a) + fabs(b);
    const double q = weight * r;
    F = F + q * r;
    noise = noise + weight * (mag * mag);
    g = g + (2.0 * q) * t;
    ex[lane] = t;
    __syncthreads();
    const double wt2 = (2.0 * weight) * t;
    for (int d2 = 0; d2 < D; ++d2) Hl[d2 * SIM_LANES] = Hl[d2 * SIM_LANES] + wt2 * ex[d2];
    __syncthreads();
}

// The cost of the lane's own point zt[d * 64] (zt is offset by the lane): simulate's step with the controlled columns read
// from the point.  With `traj` (every lane at the same point) lane 0 stores the trajectory [NS][n_steps + 1]; `first` is
// the first step in which a clamp or the slope rule acted.
template <int NS>
__device__ __forceinline__ double ctl_value_pass(const SimSystem &sys, const CtlProblem &cp, const SimTables &tab,
                                                 const CtlTables &ct, const double *__restrict__ forcing, double *xn, double *fac,
                                                 const double *cf, const double *zt, const double (&y0)[NS], int lane,
                                                 double *__restrict__ traj, int &first)
{
    double y[NS], at[NS], dy[NS] = {}, sum[NS] = {};
    const int P = cp.n_steps + 1;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        y[j] = y0[j];
        if (traj && lane == 0) traj[(size_t)j * P] = y[j];
    }
    double F = 0.0;
    int k = 0;
    for (int s = 0; s < cp.n_steps; ++s) {
        if (k + 1 < cp.segments && s >= ct.seg_first[k + 1]) ++k;
        const double *row = forcing + (size_t)s * sys.n_forcing_cols;
        bool acted = false;
        for (int f = 0; f < sys.n_forcing_factors; ++f) {
            const int n = tab.fac_norm[f];
            const int c = ct.norm_control[n];
            const double x = c < 0 ? row[-(tab.norm_src[n] + 1)] : cp.lo[c] + zt[(c * cp.segments + k) * SIM_LANES] * cp.width[c];
            const double v = sim_clamp((x - tab.norm_lo[n]) / tab.norm_span[n], acted);
            fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                           ? sim_cubic(tab.spline, tab.fac_row[f], v)
                                           : sim_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v);
        }
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            const double reach = st == 3 ? 1.0 : 0.5, weight = (st == 1 || st == 2) ? 2.0 : 1.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) at[j] = st == 0 ? y[j] : y[j] + dy[j] * reach;
            const bool stage_acted = sim_stage<NS, 1>(sys, tab, xn, fac, cf, at, dy);
            acted = acted || stage_acted;
#pragma unroll
            for (int j = 0; j < NS; ++j) sum[j] = st == 0 ? dy[j] : sum[j] + weight * dy[j];
        }
        const int point = s + 1;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            y[j] = y[j] + sum[j] / 6;
            if (traj && lane == 0) traj[(size_t)j * P + point] = y[j];
            const double target = ct.ref[(size_t)j * P + point];
            if (cp.wt[j] > 0 && target == target) {
                const double r = y[j] - target, q = cp.wt[j] * r;
                F = F + q * r;
            }
            if (point == cp.n_steps && cp.term[j] > 0) {
                const double r = y[j] - target, q = cp.term[j] * r;
                F = F + q * r;
            }
            if (cp.hl > 0 && cp.lim_hi[j] < INFINITY && y[j] > cp.lim_hi[j]) {
                const double r = y[j] - cp.lim_hi[j], q = cp.hl * r;
                F = F + q * r;
            }
            if (cp.hl > 0 && cp.lim_lo[j] > -INFINITY && y[j] < cp.lim_lo[j]) {
                const double r = cp.lim_lo[j] - y[j], q = cp.hl * r;
                F = F + q * r;
            }
        }
        if (first < 0 && acted) first = s;
    }
    for (int c = 0; c < cp.n_controls; ++c) {
        if (!(cp.move[c] > 0)) continue;
        for (int m = 0; m < cp.segments; ++m) {
            if (m == 0 && !cp.has_previous) continue;
            const int d = c * cp.segments + m;
            const double now = cp.lo[c] + zt[d * SIM_LANES] * cp.width[c];
            const double before = m == 0 ? cp.prev[c] : cp.lo[c] + zt[(d - 1) * SIM_LANES] * cp.width[c];
            const double r = now - before, q = cp.move[c] * r;
            F = F + q * r;
        }
    }
    return F;
}

struct CtlLds {
    double *fac, *xn, *tfac, *txn, *ex, *zs, *gs, *ds, *H, *cf;    // fac .. txn are offset by the lane; H is not
};

__device__ __forceinline__ CtlLds ctl_lds(double *lds, const SimSystem &sys, int D, int lane)
{
    const size_t n_state = (size_t)(sys.n_norm - sys.n_norm_forcing), n_fac = (size_t)1 + sys.n_factors;
    CtlLds l;
    l.fac = lds + lane;
    l.xn = lds + n_fac * SIM_LANES + lane;
    l.tfac = lds + (n_fac + n_state) * SIM_LANES + lane;
    l.txn = lds + (2 * n_fac + n_state) * SIM_LANES + lane;
    l.ex = lds + 2 * (n_fac + n_state) * SIM_LANES;
    l.zs = l.ex + SIM_LANES;
    l.gs = l.zs + SIM_LANES;
    l.ds = l.gs + SIM_LANES;
    l.H = l.ds + SIM_LANES;
    l.cf = l.H + (size_t)D * SIM_LANES;
    return l;
}

// ---- what control_iterate_kernel and the pooled kernels (fokl_control_pooled_device.inc) share: one text, inlined ----

// Before a tangent pass: slot 0, the draw's coefficients `coef` [n_coef], the iterate `z` [D] into the z row, H = 0
__device__ __forceinline__ void ctl_tangent_load(const SimSystem &sys, const CtlLds &l, double *Hl, int D, int lane,
                                                 const double *__restrict__ coef, const double *__restrict__ z)
{
    l.fac[0] = 1.0;
    l.tfac[0] = 0.0;
    for (int c = lane; c < sys.n_coef; c += SIM_LANES) l.cf[c] = coef[c];
    l.zs[lane] = lane < D ? z[lane] : 0.0;
    for (int d2 = 0; d2 < D; ++d2) Hl[d2 * SIM_LANES] = 0.0;
    __syncthreads();
}

// The tangent pass at the z row: F, noise (wave-uniform), g of this lane's direction (0 for lane >= D), row `lane` of H in Hl
template <int NS>
__device__ __forceinline__ void ctl_tangent_pass(const SimSystem &sys, const CtlProblem &cp, const SimTables &tab,
                                                 const CtlTables &ct, const double *__restrict__ forcing, const CtlLds &l,
                                                 double *Hl, const double (&y0r)[NS], int lane, double &F, double &noise,
                                                 double &g)
{
    const int D = cp.D, P = cp.n_steps + 1;
    double y[NS], at[NS], dy[NS] = {}, sum[NS] = {}, ty[NS] = {}, tat[NS], tdy[NS] = {}, tsum[NS] = {};
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = y0r[j];
    F = 0.0;
    noise = 0.0;
    g = 0.0;
    int k = 0;
    for (int s = 0; s < cp.n_steps; ++s) {
        if (k + 1 < cp.segments && s >= ct.seg_first[k + 1]) ++k;
        const double *row = forcing + (size_t)s * sys.n_forcing_cols;
        for (int f = 0; f < sys.n_forcing_factors; ++f) {
            const int n = tab.fac_norm[f];
            const int c = ct.norm_control[n];
            const double x = c < 0 ? row[-(tab.norm_src[n] + 1)] : cp.lo[c] + l.zs[c * cp.segments + k] * cp.width[c];
            bool clamped = false;
            const double v = sim_clamp((x - tab.norm_lo[n]) / tab.norm_span[n], clamped);
            const double tv = (c >= 0 && lane == c * cp.segments + k && !clamped) ? cp.width[c] / tab.norm_span[n] : 0.0;
            double slope;
            l.fac[(f + 1) * SIM_LANES] = f < sys.n_forcing_splines
                                             ? ctl_cubic(tab.spline, tab.fac_row[f], v, slope)
                                             : ctl_horner(tab.bern + tab.fac_row[f] * SIM_BERN_WIDTH, tab.fac_degree[f], v, slope);
            l.tfac[(f + 1) * SIM_LANES] = slope * tv;
        }
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            const double reach = st == 3 ? 1.0 : 0.5, weight = (st == 1 || st == 2) ? 2.0 : 1.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                at[j] = st == 0 ? y[j] : y[j] + dy[j] * reach;
                tat[j] = st == 0 ? ty[j] : ty[j] + tdy[j] * reach;
            }
            ctl_stage<NS>(sys, tab, l.xn, l.fac, l.txn, l.tfac, l.cf, at, tat, dy, tdy);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                sum[j] = st == 0 ? dy[j] : sum[j] + weight * dy[j];
                tsum[j] = st == 0 ? tdy[j] : tsum[j] + weight * tdy[j];
            }
        }
        const int point = s + 1;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            y[j] = y[j] + sum[j] / 6;
            ty[j] = ty[j] + tsum[j] / 6;
            const double target = ct.ref[(size_t)j * P + point];
            if (cp.wt[j] > 0 && target == target) ctl_residual(cp.wt[j], y[j], target, ty[j], true, D, lane, l.ex, Hl, F, noise, g);
            if (point == cp.n_steps && cp.term[j] > 0)
                ctl_residual(cp.term[j], y[j], target, ty[j], true, D, lane, l.ex, Hl, F, noise, g);
            if (cp.hl > 0 && cp.lim_hi[j] < INFINITY)
                ctl_residual(cp.hl, y[j], cp.lim_hi[j], ty[j], y[j] > cp.lim_hi[j], D, lane, l.ex, Hl, F, noise, g);
            if (cp.hl > 0 && cp.lim_lo[j] > -INFINITY)
                ctl_residual(cp.hl, cp.lim_lo[j], y[j], -ty[j], y[j] < cp.lim_lo[j], D, lane, l.ex, Hl, F, noise, g);
        }
    }
    for (int c = 0; c < cp.n_controls; ++c) {
        if (!(cp.move[c] > 0)) continue;
        for (int m = 0; m < cp.segments; ++m) {
            if (m == 0 && !cp.has_previous) continue;
            const int d = c * cp.segments + m;
            const double now = cp.lo[c] + l.zs[d] * cp.width[c];
            const double before = m == 0 ? cp.prev[c] : cp.lo[c] + l.zs[d - 1] * cp.width[c];
            const double t = lane == d ? cp.width[c] : (m > 0 && lane == d - 1) ? -cp.width[c] : 0.0;
            ctl_residual(cp.move[c], now, before, t, true, D, lane, l.ex, Hl, F, noise, g);
        }
    }
    if (lane >= D) g = 0.0;
}

// The stop test of iteration `it` at z_lane = zl: a status, or -1 to go on (wave-uniform)
__device__ __forceinline__ int ctl_stop_code(const CtlProblem &cp, double F, double g, double zl, int lane, int it)
{
    const bool finite = F - F == 0.0 && __all((int)(g - g == 0.0));
    const double pg = asm_max(lane < cp.D ? fabs(ctl_clip01(zl - g) - zl) : 0.0);
    return !finite ? CTL_NON_FINITE : pg <= cp.tol ? CTL_CONVERGED : it == cp.max_iter ? CTL_ITERATION_LIMIT : -1;
}

// Active set, the modified Cholesky factor in place (L[i][k] = H[k * 64 + i], H[d' * 64 + d] = H[d][d'] on entry) and the two
// solves: the Newton direction is left in ds [D] and g in gs [64].  Uses ex.
__device__ __forceinline__ void ctl_newton_direction(double *H, double *ex, double *gs, double *ds, int D, int lane, double zl,
                                                     double g)
{
    const bool active = lane < D && ((zl <= 0.0 && g > 0) || (zl >= 1.0 && g < 0));
    const unsigned long long active_mask = __ballot((int)active);
    const double free_diag = asm_max((lane < D && !active) ? fabs(H[lane * SIM_LANES + lane]) : 0.0);
    const double floor_ = CTL_PIVOT_FLOOR * fmax(1.0, free_diag);
    for (int j = 0; j < D; ++j) {
        double s = 0.0;
        if (lane >= j && lane < D) {
            const bool either = active || ((active_mask >> j) & 1ull);
            s = either ? (lane == j ? 1.0 : 0.0) : H[j * SIM_LANES + lane];
            for (int q = 0; q < j; ++q) s = s - H[q * SIM_LANES + lane] * H[q * SIM_LANES + j];
            if (lane == j) {
                s = s > floor_ ? s : fmax(fabs(s), floor_);
                H[j * SIM_LANES + j] = sqrt(s);
            }
        }
        __syncthreads();
        if (lane > j && lane < D) H[j * SIM_LANES + lane] = s / H[j * SIM_LANES + j];
        __syncthreads();
    }
    double s = active ? 0.0 : -g;
    for (int q = 0; q < D; ++q) {                                      // forward
        if (lane == q) {
            s = s / H[q * SIM_LANES + q];
            ex[q] = s;
        }
        __syncthreads();
        if (lane > q && lane < D) s = s - H[q * SIM_LANES + lane] * ex[q];
    }
    for (int q = D - 1; q >= 0; --q) {                                 // back
        if (lane == q) {
            s = s / H[q * SIM_LANES + q];
            ds[q] = s;
        }
        __syncthreads();
        if (lane < q) s = s - H[lane * SIM_LANES + q] * ds[q];
    }
    gs[lane] = g;
    __syncthreads();
}

// Every trial point at once, the lane's own in column `lane` of the H rows (Hl[d * 64]); its slope and whether it moves z.
// Returns whether the lane is a trial at all (lanes 31 and 63 are not).
__device__ __forceinline__ bool ctl_trial_points(const double *zs, const double *gs, const double *ds, double *Hl, int D, int lane,
                                                 double &slope, bool &moved)
{
    const int halving = lane & 31;
    const bool newton = lane < 32, valid = halving < CTL_TRIALS;
    const double alpha = __longlong_as_double((long long)(1023 - halving) << 52);      // 2^-halving
    slope = 0.0;
    moved = false;
    for (int d = 0; d < D; ++d) {
        const double base = newton ? ds[d] : -gs[d];
        const double x = ctl_clip01(zs[d] + alpha * base);
        Hl[d * SIM_LANES] = x;
        const double step = x - zs[d];
        slope = slope + gs[d] * step;
        moved = moved || fabs(step) > 0;
    }
    return valid;
}

// The Armijo test of every lane's trial cost Ft and the first passing lane: Newton lanes first, -1 if none passes
__device__ __forceinline__ int ctl_first_passing(bool valid, bool moved, double Ft, double F, double slope, double noise)
{
    const bool ok = valid && moved && Ft <= (F + CTL_ARMIJO * (slope < 0 ? slope : 0.0)) + CTL_NOISE * noise;
    const unsigned long long passed = __ballot((int)ok);
    const unsigned int by_newton = (unsigned int)(passed & 0x7FFFFFFFull), by_descent = (unsigned int)((passed >> 32) & 0x7FFFFFFFull);
    if (by_newton == 0u && by_descent == 0u) return -1;
    return by_newton ? __builtin_ctz(by_newton) : 32 + __builtin_ctz(by_descent);
}

// Iteration `it` of every running solve b = draw * n_starts + start.  coef [draws][n_coef]; y0 [NS][draws]; z [solves][D];
// status (-1: running), iterations, descent (steps taken in a steepest-descent lane), cost, cost_start [solves]; work [max_iter + 1]: launch `it` found a running solve;
// first_F [solves], first_g [solves][D], first_H [solves][D][D] (or null): the tangent pass of iteration 0.
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void control_iterate_kernel(
    SimSystem sys, CtlProblem cp, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const int *__restrict__ norm_control, const int *__restrict__ seg_first,
    const double *__restrict__ ref, const double *__restrict__ coef, const double *__restrict__ forcing,
    const double *__restrict__ y0, double *__restrict__ z, int *__restrict__ status, int *__restrict__ iterations,
    int *__restrict__ descent, double *__restrict__ cost, double *__restrict__ cost_start, int *__restrict__ work,
    double *__restrict__ first_F,
    double *__restrict__ first_g, double *__restrict__ first_H, int it)
{
    const size_t b = blockIdx.x;
    if (status[b] >= 0) return;                                        // a finished solve returns at once
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    const CtlTables ct{norm_control, seg_first, ref};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, D = cp.D;
    const size_t e = b / (size_t)cp.n_starts;
    const CtlLds l = ctl_lds(lds, sys, D, lane);
    double *Hl = l.H + lane;                                           // Hl[d' * 64] = H[lane][d']
    if (lane == 0) work[it] = 1;
    ctl_tangent_load(sys, l, Hl, D, lane, coef + e * sys.n_coef, z + b * D);

    // ---- the tangent pass: F, noise (wave-uniform), g of this lane's direction, row `lane` of H ----
    double y0r[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0r[j] = y0[(size_t)j * cp.n_draws + e];
    double F, noise, g;
    ctl_tangent_pass<NS>(sys, cp, tab, ct, forcing, l, Hl, y0r, lane, F, noise, g);
    if (it == 0) {
        if (lane == 0) cost_start[b] = F;
        if (first_F) {
            if (lane == 0) first_F[b] = F;
            if (lane < D) {
                first_g[b * D + lane] = g;
                for (int d2 = 0; d2 < D; ++d2) first_H[(b * D + lane) * D + d2] = Hl[d2 * SIM_LANES];
            }
        }
    }
    if (lane == 0) cost[b] = F;

    // ---- the stop test ----
    const double zl = l.zs[lane];
    const int code = ctl_stop_code(cp, F, g, zl, lane, it);
    if (code >= 0) {
        if (lane == 0) {
            status[b] = code;
            iterations[b] = it;
        }
        return;
    }

    // ---- active set, modified Cholesky and the two solves; then every trial point at once ----
    ctl_newton_direction(l.H, l.ex, l.gs, l.ds, D, lane, zl, g);
    double slope;
    bool moved;
    const bool valid = ctl_trial_points(l.zs, l.gs, l.ds, Hl, D, lane, slope, moved);
    int unused = 0;
    const double Ft = ctl_value_pass<NS>(sys, cp, tab, ct, forcing, l.xn, l.fac, l.cf, Hl, y0r, lane, nullptr, unused);
    const int taken = ctl_first_passing(valid, moved, Ft, F, slope, noise);
    if (taken < 0) {
        if (lane == 0) {
            status[b] = CTL_STALLED;
            iterations[b] = it;
        }
        return;
    }
    if (lane < D) z[b * D + lane] = l.H[lane * SIM_LANES + taken];
    if (lane == 0 && taken >= 32) descent[b] = descent[b] + 1;
}

// The trajectory of draw e under z [draws][D]: members [draws][NS][n_steps + 1], first [draws]
template <int NS>
__global__ __launch_bounds__(SIM_LANES) void control_trajectory_kernel(
    SimSystem sys, CtlProblem cp, const int *__restrict__ norm_src, const double *__restrict__ norm_lo,
    const double *__restrict__ norm_span, const int *__restrict__ fac_norm, const int *__restrict__ fac_row,
    const int *__restrict__ fac_degree, const int4 *__restrict__ entries, const double *__restrict__ spline,
    const double *__restrict__ bern, const int *__restrict__ norm_control, const int *__restrict__ seg_first,
    const double *__restrict__ ref, const double *__restrict__ coef, const double *__restrict__ forcing,
    const double *__restrict__ y0, const double *__restrict__ z, double *__restrict__ members, int *__restrict__ first)
{
    const SimTables tab{norm_src, norm_lo, norm_span, fac_norm, fac_row, fac_degree, entries, spline, bern};
    const CtlTables ct{norm_control, seg_first, ref};
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, D = cp.D;
    const size_t e = blockIdx.x;
    const CtlLds l = ctl_lds(lds, sys, D, lane);
    double *Hl = l.H + lane;
    l.fac[0] = 1.0;
    for (int c = lane; c < sys.n_coef; c += SIM_LANES) l.cf[c] = coef[e * sys.n_coef + c];
    for (int d = 0; d < D; ++d) Hl[d * SIM_LANES] = z[e * D + d];
    __syncthreads();
    double y0r[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0r[j] = y0[(size_t)j * cp.n_draws + e];
    int saturated = -1;
    (void)ctl_value_pass<NS>(sys, cp, tab, ct, forcing, l.xn, l.fac, l.cf, Hl, y0r, lane,
                             members + e * (size_t)NS * (cp.n_steps + 1), saturated);
    if (lane == 0) first[e] = saturated;
}

}  // namespace fokl

namespace {

// What the control calls refuse of n_steps (sim_check's steps_test)
int ctl_steps_fit(fokl_ctx *ctx, const std::string &who, const fokl_system &s)
{
    if (s.n_steps < 1) return fail(ctx, FOKL_ERR_ARG, who + "no step at all: the horizon needs at least one step");
    if (s.n_steps > CTL_MAX_STEPS)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(s.n_steps) + " steps, a call handles at most " + std::to_string(CTL_MAX_STEPS));
    return FOKL_OK;
}

// Everything the three entry points refuse of their inputs (outputs_ok: the caller's test of its outputs, the first refusal),
// and the plan: sys, cp, the LDS bytes of a wavefront that runs a tangent or a value pass.
int ctl_plan(fokl_ctx *ctx, const std::string &who, const fokl_system *system, const fokl_control_problem *problem, bool outputs_ok,
             SimSystem &sys, CtlProblem &cp, size_t &lds_bytes, int &n_bern_factors)
{
    const bool own_ok = outputs_ok && problem && problem->seg_first && problem->norm_control && problem->ctl_lo &&
                        problem->ctl_width && problem->ref && problem->track_weight && problem->terminal_weight &&
                        problem->limit_lo && problem->limit_hi && problem->move_weight && problem->previous && problem->z0;
    if (const int refused = sim_check(ctx, who, system, own_ok, ctl_steps_fit)) return refused;
    const fokl_system &s = *system;
    const fokl_control_problem &c = *problem;
    if (const int refused = sim_plan(ctx, who, s, sys, n_bern_factors)) return refused;

    // ---- the decision values, their box and the cost ----
    const int n_states = s.n_states, n_controls = c.n_controls, n_segments = c.n_segments;
    const int64_t n_steps = s.n_steps;
    if (n_controls < 1 || n_segments < 1 || (int64_t)n_controls * n_segments > CTL_MAX_D)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(n_controls) + " controls x " + std::to_string(n_segments) +
                                           " segments: at least one and at most " + std::to_string(CTL_MAX_D) + " decision values");
    const int D = n_controls * n_segments;
    if (c.seg_first[0] != 0) return fail(ctx, FOKL_ERR_ARG, who + "the first segment must begin with step 0");
    for (int k = 1; k < n_segments; ++k)
        if (c.seg_first[k] <= c.seg_first[k - 1] || c.seg_first[k] >= n_steps)
            return fail(ctx, FOKL_ERR_ARG, who + "the segments' first steps must increase and lie below the number of steps");
    cp = CtlProblem{};
    for (int u = 0; u < n_controls; ++u) {
        if (!std::isfinite(c.ctl_lo[u]) || !std::isfinite(c.ctl_width[u]) || !(c.ctl_width[u] > 0))
            return fail(ctx, FOKL_ERR_ARG, who + "a control's box is empty or not finite");
        if (!(c.move_weight[u] >= 0) || !std::isfinite(c.move_weight[u]) || !std::isfinite(c.previous[u]))
            return fail(ctx, FOKL_ERR_ARG, who + "move weights must be non-negative and finite, previous finite");
        bool read = false;
        for (int n = 0; n < s.n_norm_forcing; ++n) {
            if (c.norm_control[n] != u) continue;
            read = true;
            const double a = (c.ctl_lo[u] - s.norm_lo[n]) / s.norm_span[n],
                         b = (c.ctl_lo[u] + c.ctl_width[u] - s.norm_lo[n]) / s.norm_span[n];
            if (a < -1e-9 || b > 1 + 1e-9)
                return fail(ctx, FOKL_ERR_ARG, who + "a control's box reaches outside the training range of a column that reads it");
        }
        if (!read) return fail(ctx, FOKL_ERR_ARG, who + "a control is read by no model");
        cp.lo[u] = c.ctl_lo[u];
        cp.width[u] = c.ctl_width[u];
        cp.move[u] = c.move_weight[u];
        cp.prev[u] = c.previous[u];
    }
    for (int n = 0; n < s.n_norm_forcing; ++n)
        if (c.norm_control[n] < -1 || c.norm_control[n] >= n_controls)
            return fail(ctx, FOKL_ERR_ARG, who + "a forcing input reads outside the controls");
    if (!(c.limit_weight >= 0) || !std::isfinite(c.limit_weight))
        return fail(ctx, FOKL_ERR_ARG, who + "the limit weight must be non-negative and finite");
    const int64_t n_points = n_steps + 1;
    bool any_residual = false;
    for (int j = 0; j < n_states; ++j) {
        if (!(c.track_weight[j] >= 0) || !std::isfinite(c.track_weight[j]) || !(c.terminal_weight[j] >= 0) ||
            !std::isfinite(c.terminal_weight[j]))
            return fail(ctx, FOKL_ERR_ARG, who + "negative weights are refused: tracking and terminal weights must be non-negative and finite");
        if (std::isnan(c.limit_lo[j]) || std::isnan(c.limit_hi[j]) || c.limit_lo[j] > c.limit_hi[j] || c.limit_lo[j] == INFINITY ||
            c.limit_hi[j] == -INFINITY)
            return fail(ctx, FOKL_ERR_ARG, who + "a state's limits must be lower <= upper (infinite: open)");
        for (int64_t q = 0; q < n_points; ++q) {
            const double r = c.ref[j * n_points + q];
            if (std::isinf(r)) return fail(ctx, FOKL_ERR_ARG, who + "a target is infinite (NaN: not tracked)");
            if (q > 0 && !std::isnan(r) && c.track_weight[j] > 0) any_residual = true;
        }
        if (c.terminal_weight[j] > 0) {
            if (std::isnan(c.ref[j * n_points + n_steps]))
                return fail(ctx, FOKL_ERR_ARG, who + "a terminal weight needs a target at the last point");
            any_residual = true;
        }
        if (c.limit_weight > 0 && (std::isfinite(c.limit_lo[j]) || std::isfinite(c.limit_hi[j]))) any_residual = true;
        cp.wt[j] = c.track_weight[j];
        cp.term[j] = c.terminal_weight[j];
        cp.lim_lo[j] = c.limit_lo[j];
        cp.lim_hi[j] = c.limit_hi[j];
    }
    for (int u = 0; u < n_controls; ++u)
        if (c.move_weight[u] > 0 && (n_segments > 1 || c.has_previous)) any_residual = true;
    if (!any_residual) return fail(ctx, FOKL_ERR_ARG, who + "no residual at all: nothing is tracked, limited or penalised");
    if (c.n_starts < 1) return fail(ctx, FOKL_ERR_ARG, who + "starts must be at least 1");
    if ((int64_t)s.n_members * c.n_starts > CTL_MAX_SOLVES)
        return fail(ctx, FOKL_ERR_ARG, who + std::to_string(s.n_members) + " draws x " + std::to_string(c.n_starts) +
                                           " starts: one call runs at most " + std::to_string(CTL_MAX_SOLVES) + " solves");
    if (c.max_iter < 0 || !(c.tol >= 0)) return fail(ctx, FOKL_ERR_ARG, who + "max_iter and tol must be non-negative");
    for (size_t i = 0; i < (size_t)c.n_starts * D; ++i)
        if (!(c.z0[i] >= 0.0 && c.z0[i] <= 1.0)) return fail(ctx, FOKL_ERR_ARG, who + "a start lies outside the box [0, 1]");
    for (size_t i = 0; i < (size_t)n_states * s.n_members; ++i)
        if (!std::isfinite(s.y0[i])) return fail(ctx, FOKL_ERR_ARG, who + "y0 is not finite");
    const size_t lds_lane_rows = 2 * ((size_t)1 + s.n_factors + (s.n_norm - s.n_norm_forcing)) + 4 + D;
    lds_bytes = lds_lane_rows * SIM_LANES * sizeof(double) + (size_t)s.n_coef * sizeof(double);
    if (lds_bytes > SIM_LDS_BUDGET)
        return fail(ctx, FOKL_ERR_ARG, who + "the system needs " + std::to_string(lds_bytes) + " bytes of LDS ((2 x (1 + " +
                                           std::to_string(s.n_factors) + " factors + " + std::to_string(s.n_norm - s.n_norm_forcing) +
                                           " normalised states) + 4 + " + std::to_string(D) + " decision values) x 64 x 8 + " +
                                           std::to_string(s.n_coef) + " coefficients x 8), a wavefront has " +
                                           std::to_string(SIM_LDS_BUDGET));
    cp.D = D;
    cp.n_controls = n_controls;
    cp.segments = n_segments;
    cp.n_starts = c.n_starts;
    cp.n_draws = s.n_members;
    cp.n_steps = (int)n_steps;
    cp.has_previous = c.has_previous ? 1 : 0;
    cp.max_iter = c.max_iter;
    cp.hl = c.limit_weight;
    cp.tol = c.tol;
    return FOKL_OK;
}

// The system's tables, the problem's and the draws' on the device
struct CtlDevice {
    SimTables tab;
    CtlTables ct;
    double *coef, *forcing, *y0;
};

hipError_t ctl_upload(DeviceBuffers &buf, const fokl_system &s, const fokl_control_problem &c, CtlDevice &d)
{
    int *norm_control = nullptr, *seg = nullptr;
    double *ref = nullptr;
    const size_t E = (size_t)s.n_members;
    hipError_t e;
    if ((e = sim_upload(buf, s, d.tab, d.forcing)) || (e = buf.upload(&norm_control, c.norm_control, (size_t)s.n_norm_forcing)) ||
        (e = buf.upload(&seg, c.seg_first, (size_t)c.n_segments)) ||
        (e = buf.upload(&ref, c.ref, (size_t)s.n_states * (s.n_steps + 1))) || (e = buf.upload(&d.coef, s.coef, E * s.n_coef)) ||
        (e = buf.upload(&d.y0, s.y0, E * s.n_states)))
        return e;
    d.ct = CtlTables{norm_control, seg, ref};
    return hipSuccess;
}

// Iteration `it` of every solve that is still running
hipError_t ctl_iterate(fokl_ctx *ctx, int n_states, int grid, size_t lds_bytes, const SimSystem &sys, const CtlProblem &cp,
                       const CtlDevice &d, double *z, int *status, int *iterations, int *descent, double *cost, double *cost_start,
                       int *work, double *first_F, double *first_g, double *first_H, int it)
{
    return sim_dispatch(n_states, [&](auto ns) {
        const auto kernel = control_iterate_kernel<decltype(ns)::value>;
        if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, cp, d.tab.norm_src, d.tab.norm_lo,
                           d.tab.norm_span, d.tab.fac_norm, d.tab.fac_row, d.tab.fac_degree, d.tab.entries, d.tab.spline, d.tab.bern,
                           d.ct.norm_control, d.ct.seg_first, d.ct.ref, (const double *)d.coef, (const double *)d.forcing,
                           (const double *)d.y0, z, status, iterations, descent, cost, cost_start, work, first_F, first_g, first_H,
                           it);
        return hipGetLastError();
    });
}

// Every draw's trajectory under z [grid][D], and the first step in which it saturated
hipError_t ctl_trajectory(fokl_ctx *ctx, int n_states, int grid, size_t lds_bytes, const SimSystem &sys, const CtlProblem &cp,
                          const CtlDevice &d, const double *z, double *members, int *first)
{
    return sim_dispatch(n_states, [&](auto ns) {
        const auto kernel = control_trajectory_kernel<decltype(ns)::value>;
        if (hipError_t e = lds_opt_in(kernel, lds_bytes, SIM_LDS_BUDGET)) return e;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(SIM_LANES), lds_bytes, ctx->stream, sys, cp, d.tab.norm_src, d.tab.norm_lo,
                           d.tab.norm_span, d.tab.fac_norm, d.tab.fac_row, d.tab.fac_degree, d.tab.entries, d.tab.spline, d.tab.bern,
                           d.ct.norm_control, d.ct.seg_first, d.ct.ref, (const double *)d.coef, (const double *)d.forcing,
                           (const double *)d.y0, z, members, first);
        return hipGetLastError();
    });
}

// The statuses are read back every FOKL_CONTROL_POLL iterations (0: never) so that a call may stop queuing early: an
// iteration without work changes nothing.  stopped: iteration `it` was polled and left no status running.
struct CtlPoll {
    const int every = std::max(0, env_int("FOKL_CONTROL_POLL", 8));
    std::vector<int32_t> seen;
    int operator()(fokl_ctx *ctx, int it, int max_iter, const int *d_status, size_t count, bool &stopped)
    {
        stopped = false;
        if (every == 0 || (it + 1) % every != 0 || it >= max_iter) return FOKL_OK;
        seen.resize(count);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(seen.data(), d_status, count * sizeof(int32_t), hipMemcpyDeviceToHost));
        stopped = std::none_of(seen.begin(), seen.end(), [](int32_t status) { return status < 0; });
        return FOKL_OK;
    }
};

// The start with the lowest finite cost among cost / status [n_starts] (a non-finite solve is never the best; none: 0)
int ctl_best_start(const double *cost, const int32_t *status, int n_starts)
{
    int best = 0;
    double best_key = INFINITY;
    for (int s = 0; s < n_starts; ++s) {
        const double key = (std::isfinite(cost[s]) && status[s] != CTL_NON_FINITE) ? cost[s] : INFINITY;
        if (key < best_key) {
            best_key = key;
            best = s;
        }
    }
    return best;
}

}  // namespace

extern "C" int fokl_control_report(const fokl_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return fail(nullptr, FOKL_ERR_ARG, "fokl_control_report: null argument");
    std::memcpy(out, ctx->control_report, sizeof ctx->control_report);
    return FOKL_OK;
}

extern "C" int fokl_control_solve(fokl_ctx *ctx, const fokl_system *system, const fokl_control_problem *problem, double *z,
                                  double *cost, double *cost_start, int32_t *status, int32_t *iterations,
                                  int32_t *descent_steps, int32_t *best_start, double *members, int32_t *first_saturation,
                                  double *first_F, double *first_g, double *first_H)
{
    const std::string who = "fokl_control_solve: ";
    if (!ctx) return fail(nullptr, FOKL_ERR_ARG, who + "null context");
    std::memset(ctx->control_report, 0, sizeof ctx->control_report);
    const bool outputs_ok = z && cost && cost_start && status && iterations && descent_steps && best_start && members &&
                            first_saturation && (first_F == nullptr) == (first_g == nullptr) &&
                            (first_F == nullptr) == (first_H == nullptr);
    SimSystem sys{};
    CtlProblem cp{};
    size_t lds_bytes = 0;
    int n_bern_factors = 0;
    if (const int refused = ctl_plan(ctx, who, system, problem, outputs_ok, sys, cp, lds_bytes, n_bern_factors)) return refused;
    const fokl_system &s = *system;
    const int D = cp.D, n_states = s.n_states, n_starts = cp.n_starts, max_iter = cp.max_iter;
    const int64_t n_steps = s.n_steps, n_points = n_steps + 1;
    const size_t E = (size_t)s.n_members, B = E * n_starts;

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buf;
    int *d_status = nullptr, *d_iterations = nullptr, *d_descent = nullptr, *d_work = nullptr, *d_first = nullptr;
    double *d_z = nullptr, *d_cost = nullptr, *d_cost_start = nullptr, *d_fF = nullptr, *d_fg = nullptr, *d_fH = nullptr,
           *d_zbest = nullptr, *d_members = nullptr;
    CtlDevice dev{};
    HIP_TRY(ctx, ctl_upload(buf, s, *problem, dev));
    std::vector<double> z_start(B * D);
    for (size_t b = 0; b < B; ++b) std::memcpy(z_start.data() + b * D, problem->z0 + (b % n_starts) * D, D * sizeof(double));
    std::vector<int32_t> h_status(B, -1), h_zero((size_t)max_iter + 1, 0);
    std::vector<double> h_nan(B, NAN);
    HIP_TRY(ctx, buf.upload(&d_z, z_start.data(), B * D));
    HIP_TRY(ctx, buf.upload(&d_status, h_status.data(), B));
    HIP_TRY(ctx, buf.upload(&d_iterations, h_status.data(), B));
    std::vector<int32_t> h_none(B, 0);
    HIP_TRY(ctx, buf.upload(&d_descent, h_none.data(), B));
    HIP_TRY(ctx, buf.upload(&d_cost, h_nan.data(), B));
    HIP_TRY(ctx, buf.upload(&d_cost_start, h_nan.data(), B));
    HIP_TRY(ctx, buf.upload(&d_work, h_zero.data(), h_zero.size()));
    if (first_F) {
        HIP_TRY(ctx, buf.get(&d_fF, B));
        HIP_TRY(ctx, buf.get(&d_fg, B * D));
        HIP_TRY(ctx, buf.get(&d_fH, B * D * D));
    }
    HIP_TRY(ctx, buf.get(&d_zbest, E * D));
    HIP_TRY(ctx, buf.get(&d_members, E * n_states * n_points));
    HIP_TRY(ctx, buf.get(&d_first, E));

    const double pass_flops = (double)SIM_LANES * (double)n_steps * 4.0 * (8.0 * sim_terms_per_stage(sys, n_states) + 20.0 * s.n_factors);
    CtlPoll poll;
    int64_t queued = 0;
    for (int it = 0; it <= max_iter; ++it) {
        {
            TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)B * (D + 4.0), (double)B * pass_flops * 3.0);
            HIP_TRY(ctx, ctl_iterate(ctx, n_states, (int)B, lds_bytes, sys, cp, dev, d_z, d_status, d_iterations, d_descent, d_cost,
                                     d_cost_start, d_work, d_fF, d_fg, d_fH, it));
            ++queued;
        }
        bool stopped = false;
        if (const int failed = poll(ctx, it, max_iter, d_status, B, stopped)) return failed;
        if (stopped) break;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(z, d_z, B * D * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cost, d_cost, B * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cost_start, d_cost_start, B * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(status, d_status, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(iterations, d_iterations, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(descent_steps, d_descent, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(h_zero.data(), d_work, h_zero.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (first_F) {
        HIP_TRY(ctx, hipMemcpy(first_F, d_fF, B * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(first_g, d_fg, B * D * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(first_H, d_fH, B * D * D * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (size_t b = 0; b < B; ++b)
        if (status[b] < 0) return fail(ctx, FOKL_ERR_HIP, who + "a solve was left running");
    int64_t worked = 0;
    for (int32_t w : h_zero) worked += w;

    // ---- the best start of every draw, and its trajectory ----
    std::vector<double> z_best(E * D);
    for (size_t e = 0; e < E; ++e) {
        best_start[e] = ctl_best_start(cost + e * n_starts, status + e * n_starts, n_starts);
        std::memcpy(z_best.data() + e * D, z + (e * n_starts + best_start[e]) * D, D * sizeof(double));
    }
    HIP_TRY(ctx, hipMemcpy(d_zbest, z_best.data(), E * D * sizeof(double), hipMemcpyHostToDevice));
    {
        TimedRegion timed(ctx, FOKL_K_INTEGRATE, 8.0 * (double)E * n_states * n_points, (double)E * pass_flops);
        HIP_TRY(ctx, ctl_trajectory(ctx, n_states, (int)E, lds_bytes, sys, cp, dev, d_zbest, d_members, d_first));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(members, d_members, E * n_states * n_points * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(first_saturation, d_first, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t *rep = ctx->control_report;
    rep[0] = n_states;
    rep[1] = (int64_t)B;
    rep[2] = D;
    rep[3] = (int64_t)lds_bytes;
    rep[4] = queued;
    rep[5] = worked;
    rep[6] = s.n_factors - n_bern_factors;
    rep[7] = n_bern_factors;
    return FOKL_OK;
}

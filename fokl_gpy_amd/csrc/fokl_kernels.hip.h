// Device kernels of libfokl_hip.so (gfx950 / CDNA4 only; 64-wide wavefronts, fp64 throughout).
//
//   K1  basis_build_reg_kernel  fused _inputs_to_phind + evaluate_basis + term products (HBM write bound);
//       basis_build_kernel      the same with the factor table in LDS (terms with more than 16 factors)
//   K2a gram_valu_kernel     Gram block with per-thread register tiles + wavefront reductions (tiny blocks)
//   K2c gram_tiles_kernel    ... as lists of 16 x 16 tiles, symmetric half skipped, register staging (1-2 tile blocks)
//       gram_tiles_dma_kernel  the same lists staged by LDS-DMA: what every larger block runs (HALF: + one 8 x 16
//                              half tile per wavefront on v_mfma_f64_4x4x4_4b_f64, for a ragged last row tile)
//   K3  resid_kernel         residual moments for the BIC
//       reduce_slabs_kernel  fixed-order combination of per-workgroup partial sums
//
// Retired paths (K2b gram_mfma_kernel, round-1 rectangular panels: `path` 3; K2d gram_tiles4s_kernel, the tile lists on
// v_mfma_f64_4x4x4: FOKL_GRAM_MFMA4=2) are kept for A/B runs in fokl_gram_dev.inc, which only development builds (make DEV=1)
// compile.
//
// Compiled with -ffp-contract=off: the reference rounds every product and sum separately
// (FoKLRoutines.py:836, 843) and K1 reproduces those roundings; fma() is used only where it is wanted
// (error-free products of the double-double power chain).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fokl {

constexpr int WAVE = 64;
constexpr int K1_THREADS = 256;
constexpr int K1_ROWS_PER_THREAD = 2;                       // 16-byte loads / stores per lane
constexpr int K1_MAX_LDS_SLABS = 4;                         // spline orders staged in LDS per launch

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

// Column pointers come out of a table in memory, so the compiler only knows them as generic ("flat") pointers and
// would emit flat_load / flat_store, which also count on the LDS counter (lgkmcnt) and so serialise against every
// ds_read wait.  All slot memory is hipMalloc'ed global memory: say so.
typedef __attribute__((address_space(1))) const d2 *global_cd2_ptr;
typedef __attribute__((address_space(1))) d2 *global_d2_ptr;
typedef __attribute__((address_space(1))) double *global_d_ptr;
typedef __attribute__((address_space(1))) const double *global_cd_ptr;

__device__ __forceinline__ d2 load_d2(const double *p) { return *(global_cd2_ptr)(p); }
// Stored basis columns are read ONCE per launch (K2's LDS-DMA pieces and staged loads, K3's column loads): 0.5-1.2 GB that
// used to pass through the 256 MB Infinity Cache and push the 64 MB of inputs out of it right before K1 read them again --
// K1's input reads then came from HBM in between its stores (a 1 : 7 read / write mix sustains less than stores alone).
// Marked non-temporal (global_load_lds aux = 2, nt on the register loads) they leave the inputs where they are: K1 in situ
// 0.587 -> 0.650 of the HBM roof with no extra launch, K2 / K3 unchanged within their spread (profiles/nt_column_stream_r05.txt).
// FOKL_STREAM_NT=0 (A/B builds, tools/k2_variants.sh): default-policy loads, as up to round 4.
#ifndef FOKL_STREAM_NT
#define FOKL_STREAM_NT 1
#endif
__device__ __forceinline__ d2 load_d2_stream(const double *p)
{
#if FOKL_STREAM_NT
    return __builtin_nontemporal_load((global_cd2_ptr)(p));
#else
    return *(global_cd2_ptr)(p);
#endif
}
#define FOKL_GD_AUX (FOKL_STREAM_NT ? 2 : 0)               /* aux of global_load_lds: 2 = nt */
// Basis columns are written once and are far larger than L2 before anybody reads them: non-temporal stores
// (measured on K1, N = 1e6: T = 56 Bernoulli 4.5 -> 5.2 TB/s, splines 3.5 -> 5.1 TB/s).
__device__ __forceinline__ void store_d2(double *p, d2 v) { __builtin_nontemporal_store(v, (global_d2_ptr)(p)); }
__device__ __forceinline__ void store_d1(double *p, double v) { *(global_d_ptr)(p) = v; }

// ---------------------------------------------------------------------------------------------------------
// K1: basis build
// ---------------------------------------------------------------------------------------------------------

// One launch builds T columns that share U distinct (input, order) factors.  The host plans the launch
// (fokl_hip.hip: launch_basis) and ships this descriptor in device memory.
struct BasisPlan {
    int n_fac;           // U
    int n_terms;         // T
    int n_slabs;         // distinct spline orders staged in LDS (0 => gather from global / L2)
    int pad;
    // followed in memory by int32 arrays (offsets in ints from the start of the arrays block):
    //   fac_input[U], fac_order[U] (1-based), fac_slab[U] (index into slab list or -1)
    //   slab_order[K1_MAX_LDS_SLABS]
    //   term_off[T + 1], term_fac[term_off[T]], term_slot[T]
};

__device__ __forceinline__ void dd_mul_d(double &hi, double &lo, double x)
{
    // (hi + lo) * x as an unevaluated sum, error ~ 2^-104 relative.
    double t = hi * x;
    double e = __builtin_fma(hi, x, -t);
    e = e + lo * x;
    double s = t + e;
    lo = e - (s - t);
    hi = s;
}

// Bernoulli basis of order `order` (order + 1 coefficients c[0 .. order]):  c0 + sum_{j>=1} c_j * RN(x**j),
// the sum taken from 0 in ascending j with every product and addition rounded (ref FR:843).
__device__ __forceinline__ double bernoulli_basis(const double *__restrict__ c, int order, double x)
{
    double ph = x, pl = 0.0;
    double s = c[1] * x;                    // 0 + c1*x
    for (int j = 2; j <= order; ++j) {
        dd_mul_d(ph, pl, x);                // ph = RN(x**j)
        s = s + c[j] * ph;
    }
    return c[0] + s;
}

// Cubic piece: c0 + c1*t + c2*RN(t**2) + c3*RN(t**3), left to right (ref FR:836).
__device__ __forceinline__ double cubic_basis(double c0, double c1, double c2, double c3, double t)
{
    double p2 = t * t;
    double e2 = __builtin_fma(t, t, -p2);
    double p3h = p2, p3l = e2;
    dd_mul_d(p3h, p3l, t);
    double r = c0 + c1 * t;
    r = r + c2 * p2;
    r = r + c3 * p3h;
    return r;
}

// Derivatives of the same basis functions (evaluate_basis with d = 1, 2; ref FR:837-847), again with the reference's
// operation order: `k * c[k] * (x ** (k - 1))` is ((k c_k) RN(x**(k-1))), sums start from 0 in ascending k.
__device__ __forceinline__ double bernoulli_basis_d1(const double *__restrict__ c, int order, double x)
{
    double s = 0.0;
    double ph = 1.0, pl = 0.0;              // x**(k-1), k = 2 -> x
    for (int k = 2; k <= order; ++k) {
        dd_mul_d(ph, pl, x);
        s = s + ((double)k * c[k]) * ph;
    }
    return c[1] + s;
}

__device__ __forceinline__ double bernoulli_basis_d2(const double *__restrict__ c, int order, double x)
{
    double s = 0.0;
    double ph = 1.0, pl = 0.0;              // x**(k-2), k = 2 -> 1
    for (int k = 2; k <= order; ++k) {
        if (k > 2) dd_mul_d(ph, pl, x);
        s = s + ((double)((k - 1) * k) * c[k]) * ph;
    }
    return s;
}

// c1 + 2 c2 t + 3 c3 t**2   and   2 c2 + 6 c3 t   (ref FR:838, FR:840)
__device__ __forceinline__ double cubic_basis_d1(double c1, double c2, double c3, double t)
{
    double r = c1 + (2.0 * c2) * t;
    return r + (3.0 * c3) * (t * t);
}

__device__ __forceinline__ double cubic_basis_d2(double c2, double c3, double t) { return 2.0 * c2 + (6.0 * c3) * t; }

// Spline piece index and local coordinate (ref FR:570-589): phind = ceil(x*l) (0 -> 1) - 1, xsm = l*x - phind.
// `twice_normalised` selects the other coordinate the reference derives from the same index, X = (x - phind r) / r
// with r = 1 / l (FR:584-586) -- the one bss_derivatives evaluates its basis functions at (FR:742, 778-781).
__device__ __forceinline__ void spline_locate(double x, int width, bool twice_normalised, int &piece, double &t)
{
    double xl = x * (double)width;
    int p = (int)ceil(xl);
    if (p == 0) p = 1;
    p -= 1;
    if (twice_normalised) {
        const double r = 1.0 / (double)width;
        t = (x - (double)p * r) / r;
    } else {
        t = xl - (double)p;
    }
    piece = min(max(p, 0), width - 1);      // host validated the range (FR:590-591); clamp guards the LDS read
}

// What a launch differentiates: the factor of input `input` is replaced by its `order`-th derivative divided by
// `div` (= (span / l) ** order, FR:758-759, 781-782); input < 0 = plain basis build.
struct DerivSpec {
    int input;
    int order;
    double div;
    int twice_normalised;
};

// One (input, order) factor for the two rows of a lane.  `sl` = the spline slab of this order (LDS or global).
// `sl` is either a pointer into the LDS slabs or an address-space-1 pointer into the global table: the two cases are
// separate instantiations so that the gathers are ds_read / global_load (a generic pointer would make them flat_load,
// which also counts on lgkmcnt and serialises against every LDS wait).
template <bool SPLINES, typename SlabPtr>
__device__ __forceinline__ void evaluate_factor(SlabPtr sl, const double *__restrict__ bern, int order,
                                                int width, d2 x, int p0, int p1, double t0, double t1, int deriv,
                                                double div, double &vx, double &vy)
{
    if (SPLINES) {
        if (deriv == 0) {
            vx = cubic_basis(sl[p0], sl[width + p0], sl[2 * width + p0], sl[3 * width + p0], t0);
            vy = cubic_basis(sl[p1], sl[width + p1], sl[2 * width + p1], sl[3 * width + p1], t1);
        } else if (deriv == 1) {
            vx = cubic_basis_d1(sl[width + p0], sl[2 * width + p0], sl[3 * width + p0], t0) / div;
            vy = cubic_basis_d1(sl[width + p1], sl[2 * width + p1], sl[3 * width + p1], t1) / div;
        } else {
            vx = cubic_basis_d2(sl[2 * width + p0], sl[3 * width + p0], t0) / div;
            vy = cubic_basis_d2(sl[2 * width + p1], sl[3 * width + p1], t1) / div;
        }
    } else {
        if (deriv == 0) {
            vx = bernoulli_basis(bern, order, x.x);
            vy = bernoulli_basis(bern, order, x.y);
        } else if (deriv == 1) {
            vx = bernoulli_basis_d1(bern, order, x.x) / div;
            vy = bernoulli_basis_d1(bern, order, x.y) / div;
        } else {
            vx = bernoulli_basis_d2(bern, order, x.x) / div;
            vy = bernoulli_basis_d2(bern, order, x.y) / div;
        }
    }
}

template <bool SPLINES>
__global__ __launch_bounds__(K1_THREADS) void basis_build_kernel(
    const double *__restrict__ xT, int64_t ld, int64_t n, const double *__restrict__ phis, int width,
    const BasisPlan *__restrict__ plan, const int *__restrict__ arr, double *const *__restrict__ slot_ptr,
    DerivSpec deriv)
{
    __builtin_amdgcn_s_setprio(3);   // ahead of the single-wavefront chain kernels that may share the CU (fokl_chain_device.inc)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int U = plan->n_fac, T = plan->n_terms, NS = plan->n_slabs;
    const int *fac_input = arr;
    const int *fac_order = arr + U;
    const int *fac_slab = arr + 2 * U;
    const int *slab_order = arr + 3 * U;
    const int *term_off = arr + 3 * U + K1_MAX_LDS_SLABS;
    const int *term_fac = term_off + (T + 1);
    const int *term_slot = term_fac + term_off[T];

    const int tid = threadIdx.x;
    const int nthr = blockDim.x;                                       // 64 .. K1_THREADS, chosen by the host for occupancy
    double *slabs = lds;                                               // [NS][4][width]
    const int slab_doubles = SPLINES ? ((NS * 4 * width + 1) & ~1) : 0; // keep the factor table 16-B aligned
    d2 *fac = reinterpret_cast<d2 *>(lds + slab_doubles);              // [U][nthr]

    if (SPLINES) {
        for (int s = 0; s < NS; ++s) {
            const double *src = phis + (size_t)(slab_order[s] - 1) * 4 * width;
            for (int i = tid; i < 4 * width; i += nthr) slabs[s * 4 * width + i] = src[i];
        }
        __syncthreads();
    }

    const int tile_rows = nthr * K1_ROWS_PER_THREAD;
    const int64_t n_tiles = (n + tile_rows - 1) / tile_rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r0 = tile * tile_rows + (int64_t)tid * K1_ROWS_PER_THREAD;
        // ld is a multiple of 64 rows and the buffers are ld long, so the 16-byte access at r0 stays in bounds
        // whenever r0 < ld; rows >= n hold unspecified values and are never stored.
        const bool in0 = r0 < n, in1 = r0 + 1 < n;

        // phase 1: every distinct (input, order) factor once per row, parked in LDS
        int cur_input = -1;
        d2 x = {0.0, 0.0};
        int p0 = 0, p1 = 0;
        double t0 = 0.0, t1 = 0.0;
        for (int u = 0; u < U; ++u) {
            const int k = fac_input[u], order = fac_order[u];
            if (k != cur_input) {                                      // factors are sorted by input: one load per input
                cur_input = k;
                if (in0) x = *reinterpret_cast<const d2 *>(xT + (size_t)k * ld + r0);
                if (SPLINES) {
                    spline_locate(x.x, width, deriv.twice_normalised != 0, p0, t0);
                    spline_locate(x.y, width, deriv.twice_normalised != 0, p1, t1);
                }
            }
            d2 v;
            {
                const int s = SPLINES ? fac_slab[u] : -1;
                const double *bern = SPLINES ? nullptr : phis + (size_t)(order - 1) * width;
                const int dv = k == deriv.input ? deriv.order : 0;
                double vx, vy;
                if (SPLINES && s < 0)                                  // wave-uniform: slab not staged, gather from L2
                    evaluate_factor<SPLINES>((global_cd_ptr)(phis + (size_t)(order - 1) * 4 * width), bern, order, width,
                                             x, p0, p1, t0, t1, dv, deriv.div, vx, vy);
                else
                    evaluate_factor<SPLINES>((const double *)(slabs + (SPLINES ? s : 0) * 4 * width), bern, order, width,
                                             x, p0, p1, t0, t1, dv, deriv.div, vx, vy);
                v.x = vx;
                v.y = vy;
            }
            fac[u * nthr + tid] = v;
        }

        // phase 2: T products of those factors, one 16-byte store per lane and column
        for (int j = 0; j < T; ++j) {
            const int b = term_off[j], e = term_off[j + 1];
            d2 phi = fac[term_fac[b] * nthr + tid];               // 1 * first factor
            for (int f = b + 1; f < e; ++f) {
                const d2 g = fac[term_fac[f] * nthr + tid];
                phi.x = phi.x * g.x;
                phi.y = phi.y * g.y;
            }
            double *col = slot_ptr[term_slot[j]];
            if (in1) {
                store_d2(col + r0, phi);
            } else if (in0) {
                store_d1(col + r0, phi.x);
            }
        }
    }
}

// Register-resident variant: when a launch has at most K1_REG_FACTORS distinct factors the per-lane factor table
// lives in VGPRs and is indexed with wave-uniform indices (hipcc lowers this to s_set_gpr_idx -- no scratch, no LDS),
// so LDS holds only the staged spline slabs and occupancy is bounded by registers instead of 16 B of LDS per lane
// and factor.  Same arithmetic, same operation order as basis_build_kernel.
constexpr int K1_REG_FACTORS = 16;

template <bool SPLINES>
__global__ __launch_bounds__(K1_THREADS) void basis_build_reg_kernel(
    const double *__restrict__ xT, int64_t ld, int64_t n, const double *__restrict__ phis, int width,
    const BasisPlan *__restrict__ plan, const int *__restrict__ arr, double *const *__restrict__ slot_ptr,
    DerivSpec deriv)
{
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int U = plan->n_fac, T = plan->n_terms, NS = plan->n_slabs;
    const int *fac_input = arr;
    const int *fac_order = arr + U;
    const int *fac_slab = arr + 2 * U;
    const int *slab_order = arr + 3 * U;
    const int *term_off = arr + 3 * U + K1_MAX_LDS_SLABS;
    const int *term_fac = term_off + (T + 1);
    const int *term_slot = term_fac + term_off[T];

    const int tid = threadIdx.x;
    const int nthr = blockDim.x;
    double *slabs = lds;                                               // [NS][4][width]
    if (SPLINES) {
        for (int s = 0; s < NS; ++s) {
            const double *src = phis + (size_t)(slab_order[s] - 1) * 4 * width;
            for (int i = tid; i < 4 * width; i += nthr) slabs[s * 4 * width + i] = src[i];
        }
        __syncthreads();
    }

    const int tile_rows = nthr * K1_ROWS_PER_THREAD;
    const int64_t n_tiles = (n + tile_rows - 1) / tile_rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r0 = tile * tile_rows + (int64_t)tid * K1_ROWS_PER_THREAD;
        const bool in0 = r0 < n, in1 = r0 + 1 < n;
        double fx[K1_REG_FACTORS], fy[K1_REG_FACTORS];

        int cur_input = -1;
        d2 x = {0.0, 0.0};
        int p0 = 0, p1 = 0;
        double t0 = 0.0, t1 = 0.0;
        for (int u = 0; u < U; ++u) {
            const int k = fac_input[u], order = fac_order[u];
            if (k != cur_input) {
                cur_input = k;
                if (in0) x = *reinterpret_cast<const d2 *>(xT + (size_t)k * ld + r0);
                if (SPLINES) {
                    spline_locate(x.x, width, deriv.twice_normalised != 0, p0, t0);
                    spline_locate(x.y, width, deriv.twice_normalised != 0, p1, t1);
                }
            }
            double vx, vy;
            {
                const int s = SPLINES ? fac_slab[u] : -1;
                const double *bern = SPLINES ? nullptr : phis + (size_t)(order - 1) * width;
                const int dv = k == deriv.input ? deriv.order : 0;
                if (SPLINES && s < 0)                                  // wave-uniform: slab not staged, gather from L2
                    evaluate_factor<SPLINES>((global_cd_ptr)(phis + (size_t)(order - 1) * 4 * width), bern, order, width,
                                             x, p0, p1, t0, t1, dv, deriv.div, vx, vy);
                else
                    evaluate_factor<SPLINES>((const double *)(slabs + (SPLINES ? s : 0) * 4 * width), bern, order, width,
                                             x, p0, p1, t0, t1, dv, deriv.div, vx, vy);
            }
            fx[u] = vx;
            fy[u] = vy;
        }

        for (int j = 0; j < T; ++j) {
            const int b = term_off[j], e = term_off[j + 1];
            const int a0 = term_fac[b];
            d2 phi = {fx[a0], fy[a0]};                               // 1 * first factor
            for (int f = b + 1; f < e; ++f) {
                const int g = term_fac[f];
                phi.x = phi.x * fx[g];
                phi.y = phi.y * fy[g];
            }
            double *col = slot_ptr[term_slot[j]];
            if (in1) {
                store_d2(col + r0, phi);
            } else if (in0) {
                store_d1(col + r0, phi.x);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// upload helpers
// ---------------------------------------------------------------------------------------------------------

// x [n, m] row-major -> xT [m][ld]; also fills the ones column and copies y.  bounds (or NULL): lows [m] | spans [m] --
// every value normalised on the way, (x - low) / span in two separately rounded operations (FoKL.clean, FR:436-437).
__global__ void transpose_inputs_kernel(const double *__restrict__ x, const double *__restrict__ y, int64_t n, int m,
                                        int64_t ld, double *__restrict__ xT, double *__restrict__ ones,
                                        double *__restrict__ ycol, const double *__restrict__ bounds)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += (int64_t)gridDim.x * blockDim.x) {
        const bool in = i < n;
        for (int k = 0; k < m; ++k) {
            double v = in ? x[(size_t)i * m + k] : 0.0;
            if (bounds && in) v = (v - bounds[k]) / bounds[m + k];
            xT[(size_t)k * ld + i] = v;
        }
        ones[i] = in ? 1.0 : 0.0;
        ycol[i] = in ? y[i] : 0.0;
    }
}

// xT [m][ld] -> rows [n, m]
__global__ void rows_from_columns_kernel(const double *__restrict__ xT, int64_t n, int m, int64_t ld, double *__restrict__ rows)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        for (int k = 0; k < m; ++k) rows[(size_t)i * m + k] = xT[(size_t)k * ld + i];
}

// Column minima / maxima of x [n, m] row-major (np.min / np.max per column: exact, NaN-propagating).  Lane t of `lanes`
// (a multiple of m) sweeps the elements t, t + lanes, ... -- all of column t mod m, consecutive lanes on consecutive
// addresses -- and leaves its (min, max) in part[t], part[lanes + t]; the finishing kernel folds the lanes of a column.
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

__global__ void column_bounds_kernel(const double *__restrict__ x, int64_t total, int m, int64_t lanes, double *__restrict__ part)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    double lo = x[t < total ? t : t % m], hi = lo;        // (fewer elements than lanes: the column's first value stands in)
    for (int64_t at = t + lanes; at < total; at += lanes) {
        const double v = x[at];
        lo = nan_min(lo, v);
        hi = nan_max(hi, v);
    }
    part[t] = lo;
    part[lanes + t] = hi;
}

__global__ void column_bounds_finish_kernel(const double *__restrict__ part, int64_t lanes, int m, double *__restrict__ out)
{
    __shared__ double lo_s[256], hi_s[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double lo = part[k], hi = part[lanes + k];
    for (int64_t t = k + (int64_t)tid * m; t < lanes; t += (int64_t)256 * m) {
        lo = nan_min(lo, part[t]);
        hi = nan_max(hi, part[lanes + t]);
    }
    lo_s[tid] = lo;
    hi_s[tid] = hi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            lo_s[tid] = nan_min(lo_s[tid], lo_s[tid + w]);
            hi_s[tid] = nan_max(hi_s[tid], hi_s[tid + w]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[k] = lo_s[0];
        out[m + k] = hi_s[0];
    }
}

// ---------------------------------------------------------------------------------------------------------
// block-level sum of a small per-thread vector: DPP/shuffle inside the wavefront, LDS across the 4 waves
// ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;   // valid in lane 0
}

// ---------------------------------------------------------------------------------------------------------
// K2a: Gram block, VALU register tiles + wavefront reductions
// ---------------------------------------------------------------------------------------------------------

constexpr int GV_THREADS = 256;
constexpr int GV_TI = 4, GV_TJ = 4;

// grid = (S row splits, ceil(nc / GV_TJ), ceil(nr / GV_TI)); slab layout [S][nr_pad][nc_pad]
__global__ __launch_bounds__(GV_THREADS) void gram_valu_kernel(double *const *__restrict__ slot_ptr,
                                                               const int *__restrict__ row_slots, int nr,
                                                               const int *__restrict__ col_slots, int nc, int64_t n,
                                                               double *__restrict__ slab, int nr_pad, int nc_pad)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ double red[GV_THREADS / WAVE][GV_TI * GV_TJ];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.z * GV_TI, j0 = blockIdx.y * GV_TJ;
    const double *a[GV_TI], *b[GV_TJ];
#pragma unroll
    for (int i = 0; i < GV_TI; ++i) a[i] = slot_ptr[row_slots[min(i0 + i, nr - 1)]];
#pragma unroll
    for (int j = 0; j < GV_TJ; ++j) b[j] = slot_ptr[col_slots[min(j0 + j, nc - 1)]];

    double acc[GV_TI][GV_TJ];
#pragma unroll
    for (int i = 0; i < GV_TI; ++i)
#pragma unroll
        for (int j = 0; j < GV_TJ; ++j) acc[i][j] = 0.0;

    const int64_t stride = (int64_t)gridDim.x * GV_THREADS * 2;
    for (int64_t r = ((int64_t)blockIdx.x * GV_THREADS + tid) * 2; r < n; r += stride) {
        d2 av[GV_TI], bv[GV_TJ];
        const bool two = r + 1 < n;
#pragma unroll
        for (int i = 0; i < GV_TI; ++i) {
            av[i] = load_d2_stream(a[i] + r);
            if (!two) av[i].y = 0.0;
        }
#pragma unroll
        for (int j = 0; j < GV_TJ; ++j) {
            bv[j] = load_d2_stream(b[j] + r);
            if (!two) bv[j].y = 0.0;
        }
#pragma unroll
        for (int i = 0; i < GV_TI; ++i)
#pragma unroll
            for (int j = 0; j < GV_TJ; ++j) acc[i][j] = __builtin_fma(av[i].y, bv[j].y, __builtin_fma(av[i].x, bv[j].x, acc[i][j]));
    }

    const int wave = tid / WAVE, lane = tid % WAVE;
#pragma unroll
    for (int i = 0; i < GV_TI; ++i)
#pragma unroll
        for (int j = 0; j < GV_TJ; ++j) {
            double s = wave_sum(acc[i][j]);
            if (lane == 0) red[wave][i * GV_TJ + j] = s;
        }
    __syncthreads();
    if (tid < GV_TI * GV_TJ) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < GV_THREADS / WAVE; ++w) s += red[w][tid];
        const int i = i0 + tid / GV_TJ, j = j0 + tid % GV_TJ;
        slab[((size_t)blockIdx.x * nr_pad + i) * nc_pad + j] = s;
    }
}

// out[e] = sum over the S partial slabs of slab[s][e], combined in a FIXED order (so results are bitwise
// reproducible) but not serially: a 256-thread block owns `epb` output elements and 256 / epb "parts"; part p
// sums the slabs p, p + parts, p + 2 parts, ... with four independent running sums (loads in flight), then the
// parts are added in ascending order through LDS.  Also compacts [nr_pad][nc_pad] -> [nr][nc].
constexpr int RD_THREADS = 256;

__global__ __launch_bounds__(RD_THREADS) void reduce_slabs_kernel(const double *__restrict__ slab, int S, int nr, int nc,
                                                                  int nr_pad, int nc_pad, int epb,
                                                                  double *__restrict__ out)
{
    __shared__ double part_sum[RD_THREADS];
    const int parts = RD_THREADS / epb;
    const int el = threadIdx.x % epb, part = threadIdx.x / epb;
    const int e = blockIdx.x * epb + el;
    const int total = nr * nc;
    double acc = 0.0;
    if (e < total) {
        const int i = e / nc, j = e % nc;
        const size_t plane = (size_t)nr_pad * nc_pad;
        const double *p = slab + (size_t)i * nc_pad + j;
        // eight independent running sums: eight loads in flight per thread (a thread's chain of dependent rounds, not
        // bandwidth, is what a reduction over a few hundred slabs costs)
        double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int k = part;
        for (; k + 7 * parts < S; k += 8 * parts) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + u * parts) * plane];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += v[u];
        }
        for (int u = 0; k < S; k += parts, ++u) a[u & 7] += p[(size_t)k * plane];
        acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    part_sum[threadIdx.x] = acc;
    __syncthreads();
    if (part == 0 && e < total) {
        double s = part_sum[el];
        for (int q = 1; q < parts; ++q) s += part_sum[q * epb + el];
        out[e] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------
// K2c: Gram block as lists of 16 x 16 MFMA tiles (round 2; the default MFMA path)
// ---------------------------------------------------------------------------------------------------------
//
// The host (fokl_hip.hip: plan_gram) puts the columns of a launch in an INTERNAL order -- the row-side columns first,
// then the column-side columns that are not among them -- so that the part of the block that is the Gram matrix of
// the row-side columns with themselves is symmetric about the diagonal of the internal tile grid: tile (it, jt) with
// jt < it is never computed, the reduction kernel reads its mirror image.  What is left is cut, band of four i-tiles
// by band, into groups of tiles; a workgroup takes one group and one row split:
//   * it stages, per chunk of R = 32 rb rows, the <= 16 column tiles (16 columns each) its tiles touch -- row-side
//     and column-side tiles share that list, on the diagonal they are the same columns -- as [column][R + 2] in LDS
//     (pitch R + 2: conflict-free 16-column x 4-row fragment reads for R a multiple of 32);
//   * its tiles are dealt over the four wavefronts (NT per wavefront, each an (a, b) pair of staged column tiles; a
//     list is padded with tiles whose result goes nowhere) -- balanced whatever the shape of the group, which the
//     fixed i-tile-per-wave map of gram_mfma_kernel is not once the tiles below the diagonal are gone;
//   * narrow blocks (one or two tiles in all) split the k-steps of a chunk over KS wavefronts per tile instead; the
//     wavefronts of a team write their partial tiles to KS different slabs and the slab reduction adds them;
//   * P = staging passes per chunk the kernel is compiled for (ct * rb <= P): narrow blocks take the small-P builds,
//     whose few registers let eight workgroups share a CU -- that, not the depth of a chunk, is what keeps enough
//     bytes in flight when a chunk has little MFMA work to hide its latency behind;
//   * DEPTH = 2 keeps the loads of two chunks in flight (HBM-bound shapes: few tiles, little MFMA work to hide a
//     chunk's latency behind).
// Operand maps as for gram_mfma_kernel.

constexpr int GT_THREADS = 256;
constexpr int GT_MAX_NT = 10;          // tiles per wavefront (2 NT fragment addresses + 8 NT accumulator registers)
constexpr int GT_MAX_CT = 16;          // staged column tiles per group
constexpr int GT_MAX_PASS = 16;        // staging passes per chunk (ct * rb): one 16-byte load per thread and pass
constexpr int GT_AHEAD = 3;            // fragment pairs read ahead of the MFMA that consumes them

constexpr int GT_MAX_WAVES = 4;        // wavefronts per workgroup

struct GramGroup {
    int32_t ct[GT_MAX_CT];                     // internal column tile staged at local index p (-1: none, reads as zeros)
    uint16_t oi[GT_MAX_WAVES][GT_MAX_NT];      // output tile coordinates per wavefront and list position; 0xFFFF: padding
    uint16_t oj[GT_MAX_WAVES][GT_MAX_NT];
    uint8_t a[GT_MAX_WAVES][GT_MAX_NT];        // local indices of the tile's row-side and column-side column tiles
    uint8_t b[GT_MAX_WAVES][GT_MAX_NT];
    // where every staged column lives, as its distance from the slot grid's base in units of 256 bytes (padding
    // columns: the zero column, flagged in bit 31) -- filled in by the host, so that a workgroup's prologue is one round of loads instead
    // of three dependent ones (descriptor -> slot number -> pointer)
    uint32_t col_units[GT_MAX_CT][16];
};

#if defined(FOKL_GT_STAMP) || defined(FOKL_GD_STAMP)
__device__ unsigned long long fokl_debug_stamps[8192];
#endif

template <int NT, int P, int DEPTH, int KS>
__global__ __launch_bounds__(GT_THREADS, 2) void gram_tiles_kernel(double *const *__restrict__ slot_ptr,
                                                                const int *__restrict__ icols, int nci,
                                                                const GramGroup *__restrict__ groups, int ct_count,
                                                                int rb_shift, int64_t n, double *__restrict__ slab,
                                                                int nr_pad, int nc_pad,
                                                                const double *__restrict__ zero_col,
                                                                const double *__restrict__ base)
{
    __builtin_amdgcn_s_setprio(3);
    static_assert(KS == 1 || NT == 1, "k-split teams hold one tile");
    extern __shared__ __attribute__((aligned(16))) double gt_tile[];
    const int rb = 1 << rb_shift, R = 32 << rb_shift, pitch = R + 2;
    const int passes = ct_count << rb_shift;
    const GramGroup &g = groups[blockIdx.y];
    const int tid = threadIdx.x, lane = tid % WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int phase = wave % KS;
    const int spair = tid & 15, scol = tid >> 4;

    // staging map: pass q = (column tile p = q >> rb_shift, sub-chunk s = q & (rb - 1)); thread t loads rows
    // 32 s + 2 (t & 15) + {0, 1} of column 16 p + (t >> 4) of the group's list
    // A column is remembered as its distance from `base` in units of 256 bytes: one register per pass instead of two
    // (the host checks that every slot and the zero column lie on that grid within 2^32 units above base, and writes the
    // distances into the group's descriptor: padding columns point at the zero column).
    uint32_t cb[P];
    uint32_t padding = 0;                                  // bit q: pass q stages a padding column, which re-reads the first
#pragma unroll                                             // 16 bytes of the zero column (a cache hit) instead of streaming it
    for (int q = 0; q < P; ++q) {
        const uint32_t u = q < passes ? g.col_units[q >> rb_shift][scol] : 0x80000000u;
        cb[q] = u & 0x7fffffffu;
        padding |= (u >> 31) << q;
    }

    // fragment addresses: lane part (column fm of a 16-column tile, row fk of a k-step) + the tile's offset
    int aoff[NT], boff[NT];
    const int fm = lane & 15, fk = lane >> 4;
    const int frag = fm * pitch + fk;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        aoff[k] = frag + 16 * (int)g.a[wave][k] * pitch;
        boff[k] = frag + 16 * (int)g.b[wave][k] * pitch;
    }
    d4 acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = (d4){0.0, 0.0, 0.0, 0.0};

    const int64_t n_chunks = (n + R - 1) / R;
    const int64_t stride = gridDim.x;
    d2 stage[DEPTH][P];

    auto issue = [&](d2(&st)[P], int64_t chunk) {
        const int64_t r0 = chunk * R + 2 * spair;
#pragma unroll
        for (int q = 0; q < P; ++q)
            if (q < passes) {
                const int64_t r = r0 + 32 * (q & (rb - 1));
                const int64_t rc = ((padding >> q) & 1u) || r >= n ? 0 : r;      // rows past the end are masked at commit
                uint32_t units = cb[q];
                asm volatile("" : "+v"(units));            // keeps the 64-bit address from being formed once and kept
                st[q] = load_d2_stream(base + ((size_t)units << 5) + rc);
            }
    };
    auto commit = [&](const d2(&st)[P], int64_t chunk) {
        const int64_t r0 = chunk * R + 2 * spair;
#pragma unroll
        for (int q = 0; q < P; ++q)
            if (q < passes) {
                const int s = q & (rb - 1);
                const int64_t r = r0 + 32 * s;
                d2 v = st[q];
                if (r >= n) v.x = 0.0;
                if (r + 1 >= n) v.y = 0.0;
                *reinterpret_cast<d2 *>(&gt_tile[(16 * (q >> rb_shift) + scol) * pitch + 32 * s + 2 * spair]) = v;
            }
    };
    // The MFMA phase is an explicit pipeline over the (k-step, tile) sequence of a sub-chunk: the fragments of step
    // t + GT_AHEAD are read before the MFMA of step t is issued, and the order is pinned.  Measured on the 56 x 176
    // block (N = 1e6): left to itself the scheduler either hoists all 2 NT fragment reads of a k-step and spills the
    // accumulators, or (reads fenced) waits for every pair right before its MFMA, 562 us; pinned, with the tile
    // offsets in scalar registers and one VALU add per read, 480 us; pinned with the 2 NT fragment addresses kept in
    // vector registers -- this form -- 407 us (rectangular panels of gram_mfma_kernel: 434 us).  Reading further ahead
    // (6, 10 pairs) changes nothing, and neither does leaving out most of the row-side fragment reads (a timing
    // experiment: lists whose tiles share their row-side tile would gain nothing).  The matrix pipe is busy 63 % of this
    // kernel (80 % with the staging compiled out) where an assembly loop fed from LDS holds it at 100 %: DESIGN.md section 3.
    auto multiply = [&]() {
        for (int s = 0; s < rb; ++s) {
            const double *lds = gt_tile + 32 * s;
            if (KS == 1) {
                constexpr int STEPS = 8 * NT;
                double af[GT_AHEAD], bf[GT_AHEAD];
                auto fragment = [&](int tile_off, int k0) { return lds[tile_off + k0]; };
#pragma unroll
                for (int t = 0; t < GT_AHEAD && t < STEPS; ++t) {
                    af[t] = fragment(aoff[t % NT], 4 * (t / NT));
                    bf[t] = fragment(boff[t % NT], 4 * (t / NT));
                }
#pragma unroll
                for (int t = 0; t < STEPS; ++t) {
                    const double a = af[t % GT_AHEAD], b = bf[t % GT_AHEAD];
                    const int u = t + GT_AHEAD;
                    if (u < STEPS) {
                        af[t % GT_AHEAD] = fragment(aoff[u % NT], 4 * (u / NT));
                        bf[t % GT_AHEAD] = fragment(boff[u % NT], 4 * (u / NT));
                    }
                    acc[t % NT] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t % NT], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int u = 0; u < 8 / KS; ++u) {
                    const int k0 = 4 * (u * KS + phase);
                    const double a = lds[aoff[0] + k0];
                    const double b = lds[boff[0] + k0];
                    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[0], 0, 0, 0);
                }
            }
        }
    };

    int64_t chunk = blockIdx.x;
#ifdef FOKL_GT_STAMP
    const unsigned long long stamp_c0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (chunk < n_chunks) issue(stage[0], chunk);
    if (DEPTH == 2 && chunk + stride < n_chunks) issue(stage[DEPTH - 1], chunk + stride);
    while (chunk < n_chunks) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            if (chunk < n_chunks) {                        // uniform over the workgroup
                commit(stage[d], chunk);
                __syncthreads();
                const int64_t ahead = chunk + DEPTH * stride;
                if (ahead < n_chunks) issue(stage[d], ahead);
                multiply();
                __syncthreads();
                chunk += stride;
            }
        }
    }

#ifdef FOKL_GT_STAMP
    // diagnostic build only (tools/k2_clock.sh; MI355X_MICROARCH.md, DVFS item 6): shader cycles and 100 MHz ticks this
    // workgroup spent in its loop, to a buffer nothing else reads
    if (tid == 0 && blockIdx.y == 0 && blockIdx.x < 4096) {
        fokl_debug_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - stamp_c0;
        fokl_debug_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - stamp_r0;
    }
#endif
    double *out = slab + ((size_t)blockIdx.x * KS + phase) * nr_pad * nc_pad;
    asm volatile("" ::: "memory");                          // the output coordinates are fetched here, not before the loop
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int oi = g.oi[wave][k], oj = g.oj[wave][k];
        if (oi != 0xFFFF) {
#pragma unroll
            for (int v = 0; v < 4; ++v) out[(size_t)(16 * oi + fk + 4 * v) * nc_pad + 16 * oj + fm] = acc[k][v];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// K2c': the tile lists with LDS-DMA staging (global_load_lds_dwordx4) -- for the launches the matrix pipe bounds
// ---------------------------------------------------------------------------------------------------------
//
// gram_tiles_kernel keeps the fp64 matrix pipe busy 63 % of the time: its staging costs every thread some twenty
// VALU / LDS / VMEM instructions per pass, which share the SIMD's issue slots with the MFMA stream, and two barriers
// per 32-row chunk.  Here the staging is one instruction per KiB: a wavefront's global_load_lds_dwordx4 moves 64 x 16
// bytes from 64 per-lane SOURCE addresses to 1 KiB of consecutive LDS -- no staging registers, no ds_write, no row
// masks.  The LDS image keeps gram_tiles_kernel's layout ([column][34 doubles]: conflict-free fragment reads); as a
// byte stream it is 256 bytes of column 0, 16 of pad, 256 of column 1, ...: lane L of piece k lands on byte
// 1024 k + 16 L, so it loads rows 2 j, 2 j + 1 of the column that byte belongs to (pad bytes and padding columns: the
// first 16 bytes of the zero column).  One workgroup of 8 wavefronts per CU, two LDS buffers, one barrier per chunk:
// every wavefront issues its share of the next chunk's pieces (one in eight), multiplies the current chunk, waits
// for its pieces, barrier.  The last chunk of the rows arrives like the others (a column's allocation covers the
// chunk) and has its rows past the end zeroed in LDS before it is used.  Tile lists as for gram_tiles_kernel, the
// four lists of a group dealt over eight wavefronts (wavefront w takes every other entry of list w & 3).  HALF: entries 0
// and 1 of every list are half-tile slots (see below), the ordinary entries start at 2.

constexpr int GD_THREADS = 512;
constexpr int GD_MAX_PIECES = 9;       // per wavefront: 16 column tiles x 16 columns x 272 bytes / 1 KiB / 8 wavefronts

typedef __attribute__((address_space(3))) void *lds_void_ptr;
typedef __attribute__((address_space(1))) const void *global_cvoid_ptr;

#ifndef FOKL_GD_SPREAD
#define FOKL_GD_SPREAD 1               // 0: the pieces of the next chunk in one burst at the head of a chunk (A/B builds)
#endif
#ifndef FOKL_GD_SPREAD_EVERY
#define FOKL_GD_SPREAD_FIRST 1         // piece i goes out after MFMA step FIRST + EVERY * i of the chunk
#define FOKL_GD_SPREAD_EVERY 1
#endif


// LW > 0: LW LOADER wavefronts next to the eight matrix wavefronts (blockDim = 512 + 64 LW).  A wavefront issues in
// order, and an LDS-DMA load whose requests find the memory pipeline backed up holds its wavefront at that instruction --
// a matrix wavefront then issues no MFMA either (the "200 cycles per piece" of the phase stamps; compiled out, the pieces
// are worth 15 % of a flop-bound launch although the instruction itself costs the matrix stream nothing:
// profiles/k2_where_the_rest_goes_r03.txt, profiles/mfma_f64_issue_r03.txt).  The loaders issue ALL pieces of the next
// chunk, wait for them and meet the others at the chunk barrier; the matrix wavefronts never touch vector memory.
template <int NT, int NBUF, bool HALF, int LW = 0>
__global__ __launch_bounds__(GD_THREADS + LW * WAVE, LW && NT >= 4 ? 1 : 2)
void gram_tiles_dma_kernel(const GramGroup *__restrict__ groups, int ct_count, int pieces, int64_t n,
                           double *__restrict__ slab, int nr_pad, int nc_pad, const double *__restrict__ base,
                           uint32_t zero_units)
{
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ __attribute__((aligned(1024))) double gd_tile[];
    constexpr int R = 32, pitch = R + 2;
    const GramGroup &g = groups[blockIdx.y];
    const int tid = threadIdx.x, lane = tid % WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int buf_doubles = pieces * 128;                       // whole KiB pieces per buffer
    const int64_t n_chunks = (n + R - 1) / R;
    const int64_t stride = gridDim.x;

    if (LW > 0 && wave >= GD_THREADS / WAVE) {
        static_assert(LW == 0 || NBUF == 2, "the loaders follow the two-buffer schedule");
        constexpr int LWD = LW > 0 ? LW : 1;
        constexpr int MAXP = (8 * GD_MAX_PIECES + LWD - 1) / LWD;          // pieces of one loader
        const int lw = wave - GD_THREADS / WAVE;
        const double *from[MAXP];
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const int piece = lw + LWD * i;
            const int byte = 1024 * piece + 16 * lane;
            const int col = byte / (8 * pitch), within = byte % (8 * pitch);
            uint32_t u = 0x80000000u;
            if (piece < pieces && col < 16 * ct_count) u = g.col_units[col >> 4][col & 15];
            const bool pad = (u >> 31) || within >= 8 * R;
            from[i] = base + ((size_t)(pad ? zero_units : u) << 5) + (pad ? 0 : within / 8) + (int64_t)blockIdx.x * R;
        }
        const int64_t step = stride * R;
        const int mine = __builtin_amdgcn_readfirstlane(lw < pieces ? (pieces - lw + LWD - 1) / LWD : 0);
        auto issue_all = [&](int buf) {
#pragma unroll
            for (int i = 0; i < MAXP; ++i)
                if (i < mine) {                                 // wave-uniform
                    __builtin_amdgcn_global_load_lds((global_cvoid_ptr)from[i],
                                                     (lds_void_ptr)(gd_tile + buf * buf_doubles + 128 * (lw + LWD * i)), 16, 0, FOKL_GD_AUX);
                    from[i] += step;
                }
        };
        int64_t chunk = blockIdx.x;
        if (chunk < n_chunks) issue_all(0);
        __syncthreads();                                        // (vmcnt(0), then the barrier)
        int buf = 0;
        while (chunk < n_chunks) {
            if (chunk + stride < n_chunks) issue_all(buf ^ 1);
            if (chunk == n_chunks - 1 && n % R != 0) __syncthreads();      // (the matrix wavefronts trim the last chunk)
            __syncthreads();
            chunk += stride;
            buf ^= 1;
        }
        return;
    }

    // This lane's part in the pieces its wavefront issues (piece wave, wave + 8, ...): the address it reads next.  The
    // addresses are formed once and then only advance -- every workgroup walks down the rows in steps of gridDim.x chunks,
    // padding lanes walk down the zero column alongside -- so a piece costs ONE 64-bit add per chunk.  It used to cost eight
    // VALU instructions (distance -> address, row offset, the padding select), and a matrix wavefront's VALU instructions
    // are not free: gfx950 issues the fp64 MFMA through the SIMD's vector datapath, and two integer adds per MFMA take a
    // sixth off its rate (tools/mfma_f64_issue.hip, profiles/mfma_f64_issue_r03.txt).
    const double *src[GD_MAX_PIECES];
#pragma unroll
    for (int i = 0; i < GD_MAX_PIECES; ++i) {
        const int piece = wave + 8 * i;
        const int byte = 1024 * piece + 16 * lane;
        const int col = byte / (8 * pitch), within = byte % (8 * pitch);
        uint32_t u = 0x80000000u;                              // (flag: padding, the zero column)
        if (piece < pieces && col < 16 * ct_count) u = g.col_units[col >> 4][col & 15];
        const bool pad = (u >> 31) || within >= 8 * R;
        src[i] = base + ((size_t)(pad ? zero_units : u) << 5) + (pad ? 0 : within / 8) + (int64_t)blockIdx.x * R;
    }
    const int64_t src_step = stride * R;                        // rows between two chunks of this workgroup
#define FOKL_GD_ISSUE_PIECE(i, row0, buf)                      /* (row0: where src[i] points by construction) */     \
    do {                                                                                                   \
        if (LW == 0 && wave + 8 * (i) < pieces) {              /* wave-uniform; LW: the loaders' job */    \
            __builtin_amdgcn_global_load_lds((global_cvoid_ptr)src[i],                                     \
                                             (lds_void_ptr)(gd_tile + (buf) * buf_doubles + 128 * (wave + 8 * (i))), 16, 0, FOKL_GD_AUX); \
            src[i] += src_step;                                                                            \
        }                                                                                                  \
    } while (0)
    auto issue = [&](int64_t chunk, int buf) {                  // (chunk: the one the addresses point at)
        (void)chunk;
#pragma unroll
        for (int i = 0; i < GD_MAX_PIECES; ++i) FOKL_GD_ISSUE_PIECE(i, chunk * R, buf);
    };

    // tiles: list w & 3 of the group, every other entry
    const int fm = lane & 15, fk = lane >> 4;
    const int frag = fm * pitch + fk;
    const int row = wave & 3, first = wave >> 2;
    constexpr int E0 = HALF ? 2 : 0;                           // first ordinary entry of a list
    // the next chunk's pieces issued among the MFMA steps (below) where a chunk has 24 steps or more; shorter loops leave
    // the pieces too little time to land (8 x 40: 56 -> 65 us with the spread issue, 56 x 176: 338 -> 325 us)
    constexpr bool SPREAD = FOKL_GD_SPREAD != 0 && 8 * (NT + (HALF ? 1 : 0)) >= 24;
    int aoff[NBUF][NT], boff[NBUF][NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int j = E0 + 2 * k + first;
        const bool have = j < GT_MAX_NT;
#pragma unroll
        for (int bf_ = 0; bf_ < NBUF; ++bf_) {
            aoff[bf_][k] = frag + 16 * (have ? (int)g.a[row][j] : 0) * pitch + bf_ * buf_doubles;
            boff[bf_][k] = frag + 16 * (have ? (int)g.b[row][j] : 0) * pitch + bf_ * buf_doubles;
        }
    }
    d4 acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = (d4){0.0, 0.0, 0.0, 0.0};
    int real_tiles = 0;                                        // lists are packed: real tiles first, padding behind
#pragma unroll
    for (int k = 0; k < NT; ++k)
        real_tiles += (E0 + 2 * k + first < GT_MAX_NT && g.oi[row][E0 + 2 * k + first] != 0xFFFF) ? 1 : 0;
    real_tiles = __builtin_amdgcn_readfirstlane(real_tiles);
    // HALF: entry `first` of the list is this wavefront's half tile -- a tile of the ragged last row tile, of which only
    // rows 0 .. 7 are asked for.  Per k-step two v_mfma_f64_4x4x4_4b_f64 (16 cycles each, where the 16x16x4 form takes
    // 64): D_blk[i][j] += sum_k A[4 q + i][k] B[k][4 blk + j] for q = 0, 1 -- the four blocks share the row-side operand
    // (lane i + 4 blk + 16 k reads column 4 q + i, row k of the staged tile), the ordinary column-side fragment is their
    // four operands side by side, and lane j + 4 blk + 16 i ends up with row 4 q + i, column 4 blk + j of the tile.
    int hoff[NBUF][2] = {}, hboff[NBUF] = {};
    double hacc[2] = {0.0, 0.0};
    const bool half_real = HALF && __builtin_amdgcn_readfirstlane((int)g.oi[row][first]) != 0xFFFF;
    if (HALF) {
#pragma unroll
        for (int bf_ = 0; bf_ < NBUF; ++bf_) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
                hoff[bf_][q] = (16 * (half_real ? (int)g.a[row][first] : 0) + 4 * q + (lane & 3)) * pitch + fk + bf_ * buf_doubles;
            hboff[bf_] = frag + 16 * (half_real ? (int)g.b[row][first] : 0) * pitch + bf_ * buf_doubles;
        }
    }

    // The pieces of a later chunk are issued from INSIDE the loop, one per MFMA step from step 1 on: issued in a burst at
    // the head of the chunk they cost every wavefront ~ 200 cycles apiece -- a fifth to a quarter of the chunk, the DMA
    // itself never being waited for (tools/k2_phases.sh) -- among MFMAs a little of that overlaps: 2-4 % on the 56-row
    // blocks.  (Not kept: only the second wavefront of every SIMD issuing, so that the first never stalls: 10-25 % slower.)
    // next_buf < 0: nothing to issue.
    auto multiply = [&](const int (&ao)[NT], const int (&bo)[NT], const int (&ho)[2], const int hb, const int64_t next_row0,
                        const int next_buf) {
        constexpr int W = NT + (HALF ? 1 : 0);                 // MFMA steps per k-step: the half tile first
        constexpr int STEPS = 8 * W;
#ifndef FOKL_GD_AHEAD
#define FOKL_GD_AHEAD 3
#endif
        // (three-tile kernels with loaders read two fragment pairs ahead instead of three: the six registers are what
        // lets a CU host two of their 12-wavefront workgroups)
        constexpr int AHEAD = LW > 0 && NT == 3 ? 2 : FOKL_GD_AHEAD;
        double af[AHEAD], bf[AHEAD], cf[HALF ? AHEAD : 1];
#define FOKL_GD_FETCH(u)                                                                                   \
    do {                                                                                                   \
        if (HALF && (u) % W == 0) {                                                                        \
            af[(u) % AHEAD] = gd_tile[ho[0] + 4 * ((u) / W)];                                              \
            cf[HALF ? (u) % AHEAD : 0] = gd_tile[ho[1] + 4 * ((u) / W)];                                   \
            bf[(u) % AHEAD] = gd_tile[hb + 4 * ((u) / W)];                                                 \
        } else {                                                                                           \
            af[(u) % AHEAD] = gd_tile[ao[(u) % W - (HALF ? 1 : 0)] + 4 * ((u) / W)];                       \
            bf[(u) % AHEAD] = gd_tile[bo[(u) % W - (HALF ? 1 : 0)] + 4 * ((u) / W)];                       \
        }                                                                                                  \
    } while (0)
#pragma unroll
        for (int t = 0; t < AHEAD && t < STEPS; ++t) FOKL_GD_FETCH(t);
#pragma unroll
        for (int t = 0; t < STEPS; ++t) {
            const double a = af[t % AHEAD], b = bf[t % AHEAD], c = cf[HALF ? t % AHEAD : 0];
            if (t + AHEAD < STEPS) FOKL_GD_FETCH(t + AHEAD);
            if (HALF && t % W == 0) {
                if (half_real) {                               // wave-uniform
                    hacc[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, hacc[0], 0, 0, 0);
                    hacc[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(c, b, hacc[1], 0, 0, 0);
                }
            } else if (t % W - (HALF ? 1 : 0) < real_tiles) {  // wave-uniform: a padding entry costs its reads only (the two
                acc[t % W - (HALF ? 1 : 0)] =                  // wavefronts of a SIMD share a list)
                    __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t % W - (HALF ? 1 : 0)], 0, 0, 0);
            }
            if (SPREAD && next_buf >= 0) {                     // wave-uniform
#pragma unroll
                for (int i = 0; i < GD_MAX_PIECES; ++i)
                    if (t == (FOKL_GD_SPREAD_FIRST + FOKL_GD_SPREAD_EVERY * i < STEPS ? FOKL_GD_SPREAD_FIRST + FOKL_GD_SPREAD_EVERY * i : STEPS - 1))
                        FOKL_GD_ISSUE_PIECE(i, next_row0, next_buf);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#undef FOKL_GD_FETCH
    };
    // rows past the end of the data, in the last chunk: zero them where they landed
    auto trim = [&](int64_t chunk, int buf) {
        if (chunk != n_chunks - 1 || n % R == 0) return;
        const int keep = (int)(n - chunk * R);
        for (int c = tid; c < 16 * ct_count; c += GD_THREADS)
            for (int r = keep; r < R; ++r) gd_tile[buf * buf_doubles + c * pitch + r] = 0.0;
        __syncthreads();
    };
    // NBUF = 2: the next chunk's pieces are issued, this chunk multiplied, then all pieces waited for and a barrier.
    // NBUF = 3: the pieces of the chunk after next are issued instead and stay in flight across the barrier -- a counted
    // s_waitcnt vmcnt(this wavefront's pieces per chunk) retires the older chunk only, and the barrier is a raw s_barrier
    // (__syncthreads() would drain every LDS-DMA write first).
    int my_pieces = 0;
#pragma unroll
    for (int i = 0; i < GD_MAX_PIECES; ++i) my_pieces += wave + 8 * i < pieces ? 1 : 0;
    my_pieces = __builtin_amdgcn_readfirstlane(my_pieces);
    auto wait_all_but_newest = [&](bool newest_in_flight) {
        if (!newest_in_flight) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            return;
        }
        switch (my_pieces) {
            case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
            case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
            case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
            case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
            case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
            case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
            case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
            case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        }
    };
    auto raw_barrier = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    int64_t chunk = blockIdx.x;
#ifdef FOKL_GT_STAMP
    // diagnostic build only (tools/k2_clock.sh; MI355X_MICROARCH.md, DVFS item 6): shader cycles and 100 MHz ticks around
    // this workgroup's loop, to a buffer nothing else reads
    const unsigned long long stamp_c0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef FOKL_GD_STAMP
    // diagnostic build only (tools/k2_phases.sh): shader cycles of wavefronts 0 and 7 in the four phases of a chunk
    unsigned long long ph_issue = 0, ph_mult = 0, ph_wait = 0, ph_bar = 0;
#define FOKL_GD_NOW() __builtin_amdgcn_s_memtime()
#endif
    if (NBUF == 2) {
        auto one_chunk = [&](int64_t c, int buf) {
#ifdef FOKL_GD_STAMP
            const unsigned long long t0 = FOKL_GD_NOW();
#endif
            const bool more = c + stride < n_chunks;
            if (!SPREAD && more) issue(c + stride, buf ^ 1);
#ifdef FOKL_GD_STAMP
            const unsigned long long t1 = FOKL_GD_NOW();
#endif
            trim(c, buf);
            multiply(aoff[buf], boff[buf], hoff[buf], hboff[buf], (c + stride) * R, more ? buf ^ 1 : -1);
#ifdef FOKL_GD_STAMP
            const unsigned long long t2 = FOKL_GD_NOW();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned long long t3 = FOKL_GD_NOW();
#endif
            __syncthreads();                                   // (waits for this wavefront's pieces: vmcnt(0), then the barrier)
#ifdef FOKL_GD_STAMP
            const unsigned long long t4 = FOKL_GD_NOW();
            ph_issue += t1 - t0;
            ph_mult += t2 - t1;
            ph_wait += t3 - t2;
            ph_bar += t4 - t3;
#endif
        };
        if (chunk < n_chunks) issue(chunk, 0);
        __syncthreads();
        while (chunk < n_chunks) {
            one_chunk(chunk, 0);
            chunk += stride;
            if (chunk >= n_chunks) break;
            one_chunk(chunk, 1);
            chunk += stride;
        }
    } else {
        auto one_chunk = [&](int64_t c, int buf) {
            const bool ahead = c + 2 * stride < n_chunks;
            if (!SPREAD && ahead) issue(c + 2 * stride, (buf + 2) % 3);
            trim(c, buf);
            multiply(aoff[buf % NBUF], boff[buf % NBUF], hoff[buf % NBUF], hboff[buf % NBUF], (c + 2 * stride) * R,
                     ahead ? (buf + 2) % 3 : -1);
            wait_all_but_newest(ahead);
            raw_barrier();
        };
        if (chunk < n_chunks) issue(chunk, 0);
        const bool second = chunk + stride < n_chunks;
        if (second) issue(chunk + stride, 1);
        wait_all_but_newest(second);
        raw_barrier();
        while (chunk < n_chunks) {
            one_chunk(chunk, 0);
            chunk += stride;
            if (chunk >= n_chunks) break;
            one_chunk(chunk, 1);
            chunk += stride;
            if (chunk >= n_chunks) break;
            one_chunk(chunk, 2);
            chunk += stride;
        }
    }

#ifdef FOKL_GT_STAMP
    if (tid == 0 && blockIdx.y == 0 && blockIdx.x < 4096) {
        fokl_debug_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - stamp_c0;
        fokl_debug_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - stamp_r0;
    }
#endif
#ifdef FOKL_GD_STAMP
    if (lane == 0 && (wave == 0 || wave == 7) && blockIdx.y == 0 && blockIdx.x < 512) {
        unsigned long long *st = fokl_debug_stamps + 8 * blockIdx.x + (wave == 7 ? 4 : 0);
        st[0] = ph_issue;
        st[1] = ph_mult;
        st[2] = ph_wait;
        st[3] = ph_bar;
    }
#endif
    double *out = slab + (size_t)blockIdx.x * nr_pad * nc_pad;
    asm volatile("" ::: "memory");
    if (half_real) {                                           // rows 4 q + fk of the tile; its rows 8 .. 15 are nobody's
        const int oi = g.oi[row][first], oj = g.oj[row][first];
#pragma unroll
        for (int q = 0; q < 2; ++q) out[(size_t)(16 * oi + 4 * q + fk) * nc_pad + 16 * oj + fm] = hacc[q];
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int j = E0 + 2 * k + first;
        if (j < GT_MAX_NT) {
            const int oi = g.oi[row][j], oj = g.oj[row][j];
            if (oi != 0xFFFF) {
#pragma unroll
                for (int v = 0; v < 4; ++v) out[(size_t)(16 * oi + fk + 4 * v) * nc_pad + 16 * oj + fm] = acc[k][v];
            }
        }
    }
}

// reduce_slabs_kernel for gram_tiles_kernel's slabs: element (i, j) of the caller's block sits at internal column
// perm[j]; a position in a tile below the diagonal of the internal tile grid was not computed and is read from its
// mirror image (both indices are then row-side columns).  Same fixed summation order.
__global__ __launch_bounds__(RD_THREADS) void reduce_slabs_sym_kernel(const double *__restrict__ slab, int S, int nr,
                                                                      int nc, int nr_pad, int nc_pad, int epb,
                                                                      const int *__restrict__ perm,
                                                                      double *__restrict__ out)
{
    __shared__ double part_sum[RD_THREADS];
    const int parts = RD_THREADS / epb;
    const int el = threadIdx.x % epb, part = threadIdx.x / epb;
    const int e = blockIdx.x * epb + el;
    const int total = nr * nc;
    double acc = 0.0;
    if (e < total) {
        int i = e / nc, c = perm[e % nc];
        if ((c >> 4) < (i >> 4)) {
            const int t = i;
            i = c;
            c = t;
        }
        const size_t plane = (size_t)nr_pad * nc_pad;
        const double *p = slab + (size_t)i * nc_pad + c;
        // eight independent running sums: eight loads in flight per thread (a thread's chain of dependent rounds, not
        // bandwidth, is what a reduction over a few hundred slabs costs)
        double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int k = part;
        for (; k + 7 * parts < S; k += 8 * parts) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + u * parts) * plane];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += v[u];
        }
        for (int u = 0; k < S; k += parts, ++u) a[u & 7] += p[(size_t)k * plane];
        acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    part_sum[threadIdx.x] = acc;
    __syncthreads();
    if (part == 0 && e < total) {
        double s = part_sum[el];
        for (int q = 1; q < parts; ++q) s += part_sum[q * epb + el];
        out[e] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------
// K3: residual moments  r = y - sum_j beta_j X_j ;  partial (sum r, sum r^2) per workgroup
// ---------------------------------------------------------------------------------------------------------

constexpr int RS_THREADS = 256;
constexpr int RS_BATCH = 256;      // columns whose (pointer, coefficient) pairs sit in LDS at a time

struct ResidCol {
    const double *ptr;
    double beta;
};

// Every lane owns two consecutive rows (one 16-byte load per column); the per-column pointer and coefficient
// are wave-uniform and come from LDS as one broadcast ds_read_b128, so the column loop is a stream of
// independent global loads + 2 FMAs with no dependent scalar pointer chase.
__global__ __launch_bounds__(RS_THREADS) void resid_kernel(double *const *__restrict__ slot_ptr,
                                                           const int *__restrict__ slots, int nc,
                                                           const double *__restrict__ beta,
                                                           const double *__restrict__ y, int64_t n,
                                                           double *__restrict__ slab)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ __attribute__((aligned(16))) ResidCol cols[RS_BATCH];
    __shared__ double red[RS_THREADS / WAVE][2];
    const int tid = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    const int64_t n_tiles = (n + RS_THREADS * 2 - 1) / (RS_THREADS * 2);
    const bool single_batch = nc <= RS_BATCH;
    if (single_batch) {
        for (int j = tid; j < nc; j += RS_THREADS) cols[j] = ResidCol{slot_ptr[slots[j]], beta[j]};
        __syncthreads();
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = (tile * RS_THREADS + tid) * 2;
        const bool in0 = r < n, in1 = r + 1 < n;
        d2 fit = {0.0, 0.0};
        for (int c0 = 0; c0 < nc; c0 += RS_BATCH) {
            const int cnt = min(RS_BATCH, nc - c0);
            if (!single_batch) {
                __syncthreads();
                for (int j = tid; j < cnt; j += RS_THREADS) cols[j] = ResidCol{slot_ptr[slots[c0 + j]], beta[c0 + j]};
                __syncthreads();
            }
            if (in0) {
#pragma unroll 8
                for (int j = 0; j < cnt; ++j) {
                    const ResidCol c = cols[j];
                    const d2 xv = load_d2_stream(c.ptr + r);
                    fit.x = __builtin_fma(c.beta, xv.x, fit.x);
                    fit.y = __builtin_fma(c.beta, xv.y, fit.y);
                }
            }
        }
        if (in0) {
            const d2 yv = *reinterpret_cast<const d2 *>(y + r);
            const double r0 = yv.x - fit.x;
            const double r1 = in1 ? yv.y - fit.y : 0.0;
            s1 += r0 + r1;
            s2 += r0 * r0 + r1 * r1;
        }
    }
    const int wave = tid / WAVE, lane = tid % WAVE;
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        red[wave][0] = s1;
        red[wave][1] = s2;
    }
    __syncthreads();
    if (tid < 2) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < RS_THREADS / WAVE; ++w) s += red[w][tid];
        slab[(size_t)blockIdx.x * 2 + tid] = s;
    }
}


// ---------------------------------------------------------------------------------------------------------
// K3, matrix-free: the residual moments as a quadratic form in the model's distinct factors
// ---------------------------------------------------------------------------------------------------------
//
// A residual pass over stored columns reads 8 N (P + 2) bytes; the columns are products of a handful of basis
// functions of the inputs, and the inputs (8 N M_used bytes, resident in the 256 MB Infinity Cache at the headline size)
// are all it takes to form them again.  With f_0 .. f_{U-1} the model's distinct (input, order) factors at a row, a model
// of one- and two-factor terms is
//
//     fit = c0 + sum_a f_a * ( l_a + sum_{b > a} Q_ab f_b )          l_a = beta of the term {a}, Q_ab = beta of {a, b}
//
// -- U (U + 1) / 2 fused multiply-adds per row whatever the number of terms, on operands with COMPILE-TIME register
// numbers: factor slot = GM inputs x KM orders per input, every loop below is unrolled, the coefficients are wave-uniform
// scalar loads (s_load, SGPR operands of v_fma_f64: no VGPR, no LDS).  Round 2-4's form of this pass walked the term list
// and fetched each term's factors from a per-lane table in VGPRs through s_set_gpr_idx -- some thirty instructions per
// term, 0.23 of its roof; this one is bounded by the input stream.  The factors are evaluated with K1's separately
// rounded operations (so f_a is the stored column's value bit for bit); the SUM is associated differently from
// resid_kernel's fit = fma(beta_j, column_j, fit) in column order, so the two passes agree to rounding, not to the bit
// (tests/test_gpu_parity.py: 1e-13 of the moments' scale).  Models with a three-factor term, or whose factors do not fit
// a slot layout, take the stored-column pass (fokl_bic_resid_terms_launch says FOKL_ERR_ARG; engine.resid_terms_supported).

constexpr int RT_MAX_ORDER = 8;            // Bernoulli orders the matrix-free pass handles (coefficient row: 9 doubles)
constexpr int RT_COEF_STRIDE = 10;         // doubles per factor: c[0 .. 8] + the order (as a double; 0 = empty slot)
constexpr int RQ_MAX_SLOTS = 32;

struct ResidQuadTable {
    int32_t n_groups;                      // inputs used (<= GM of the kernel the host picked)
    int32_t pad;
    int32_t input[RQ_MAX_SLOTS];           // group g reads input column input[g]
    int32_t omax[RQ_MAX_SLOTS];            // largest order among the group's factors
    double c0;                             // the intercept's coefficient (+ any term without factors)
    double coef[RQ_MAX_SLOTS][RT_COEF_STRIDE];   // slot g * KM + k: the k-th order of group g (splines: [9] = order only)
    double lin[RQ_MAX_SLOTS];
    double quad[RQ_MAX_SLOTS * (RQ_MAX_SLOTS - 1) / 2];   // pairs a < b of different groups, in the kernel's loop order
};

// position of the pair (a, b), a < b, in ResidQuadTable::quad for a layout of KM orders per input (host and device)
__host__ __device__ constexpr int resid_quad_index(int a, int b, int UM, int KM)
{
    int q = 0;
    for (int i = 0; i < UM; ++i)
        for (int j = i + 1; j < UM; ++j) {
            if (i / KM == j / KM) continue;
            if (i == a && j == b) return q;
            ++q;
        }
    return -1;
}

typedef __attribute__((address_space(4))) const ResidQuadTable *const_quad_ptr;      // constant address space: scalar loads

// OT: the highest Bernoulli order the instance evaluates (2, 4 or RT_MAX_ORDER).  Everything a row does between its loads and
// its two sums is straight-line code: a factor of lower order carries zero coefficients beyond its own (val + 0 * x**j
// leaves val as it is), an empty slot carries only zeros -- so the scalar loads of the coefficients are scheduled ahead in
// bulk (s_load_dwordx8 / x16) instead of one by one inside wave-uniform branches, each waited for on the spot.
template <bool SPLINES, int GM, int KM, int OT>
__global__ __launch_bounds__(RS_THREADS) void resid_quadratic_kernel(
    const double *__restrict__ xT, int64_t ld, int64_t n, const double *__restrict__ phis, int width,
    const ResidQuadTable *__restrict__ table, const double *__restrict__ y, double *__restrict__ slab)
{
    constexpr int UM = GM * KM;
    static_assert(UM <= RQ_MAX_SLOTS && OT >= 2 && OT <= RT_MAX_ORDER, "slot layout");
    __builtin_amdgcn_s_setprio(3);
    __shared__ double red[RS_THREADS / WAVE][2];
    const const_quad_ptr tab = (const_quad_ptr)(uintptr_t)table;
    const int tid = threadIdx.x;
    const int G = tab->n_groups;

    double s1 = 0.0, s2 = 0.0;
    const int64_t n_tiles = (n + RS_THREADS * 2 - 1) / (RS_THREADS * 2);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = (tile * RS_THREADS + tid) * 2;
        const bool in0 = r < n, in1 = r + 1 < n;
        if (!in0) continue;                                     // ld is a multiple of 64 rows: the pair stays in bounds
        // every input of the model first (all loads in flight together), y with them; an unused group reads the first
        // group's column again (a cache hit) and multiplies it by zeros
        d2 xv[GM];
#pragma unroll
        for (int g = 0; g < GM; ++g) xv[g] = load_d2(xT + (size_t)tab->input[g < G ? g : 0] * ld + r);
        const d2 yv = load_d2(y + r);

        double f[UM][2];
#pragma unroll
        for (int g = 0; g < GM; ++g) {
            const double x[2] = {xv[g].x, xv[g].y};
            if (SPLINES) {
                int piece[2];
                double t[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) spline_locate(x[q], width, false, piece[q], t[q]);
#pragma unroll
                for (int k = 0; k < KM; ++k) {
                    const int order = (int)tab->coef[g * KM + k][9];          // 0: empty slot (evaluated as order 1, times 0)
                    const global_cd_ptr sl = (global_cd_ptr)(phis + (size_t)((order > 0 ? order : 1) - 1) * 4 * width);
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const double v = cubic_basis(sl[piece[q]], sl[width + piece[q]], sl[2 * width + piece[q]],
                                                     sl[3 * width + piece[q]], t[q]);
                        f[g * KM + k][q] = order > 0 ? v : 0.0;
                    }
                }
            } else {
                // RN(x**j), j = 1 .. OT (double-double chain, as bernoulli_basis forms them)
                double pw[OT + 1][2];
                {
                    double ph[2], pl[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        pw[1][q] = ph[q] = x[q];
                        pl[q] = 0.0;
                    }
#pragma unroll
                    for (int j = 2; j <= OT; ++j) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            dd_mul_d(ph[q], pl[q], x[q]);
                            pw[j][q] = ph[q];
                        }
                    }
                }
                // c0 + sum_{j>=1} c_j RN(x**j), the sum taken from 0 in ascending j with every product and addition
                // rounded (bernoulli_basis)
#pragma unroll
                for (int k = 0; k < KM; ++k) {
                    double val[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) val[q] = tab->coef[g * KM + k][1] * pw[1][q];
#pragma unroll
                    for (int j = 2; j <= OT; ++j) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) val[q] = val[q] + tab->coef[g * KM + k][j] * pw[j][q];
                    }
#pragma unroll
                    for (int q = 0; q < 2; ++q) f[g * KM + k][q] = tab->coef[g * KM + k][0] + val[q];
                }
            }
        }

        double fit[2] = {tab->c0, tab->c0};
        int q = 0;
#pragma unroll
        for (int a = 0; a < UM; ++a) {
            double inner[2] = {tab->lin[a], tab->lin[a]};
#pragma unroll
            for (int b = a + 1; b < UM; ++b) {
                if (a / KM == b / KM) continue;                 // two orders of one input never meet in a term
                const double c = tab->quad[q++];
                inner[0] = __builtin_fma(c, f[b][0], inner[0]);
                inner[1] = __builtin_fma(c, f[b][1], inner[1]);
            }
            fit[0] = __builtin_fma(f[a][0], inner[0], fit[0]);
            fit[1] = __builtin_fma(f[a][1], inner[1], fit[1]);
        }
        const double r0 = yv.x - fit[0];
        const double r1 = in1 ? yv.y - fit[1] : 0.0;
        s1 += r0 + r1;
        s2 += r0 * r0 + r1 * r1;
    }
    const int wave = tid / WAVE, lane = tid % WAVE;
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        red[wave][0] = s1;
        red[wave][1] = s2;
    }
    __syncthreads();
    if (tid < 2) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < RS_THREADS / WAVE; ++w) s += red[w][tid];
        slab[(size_t)blockIdx.x * 2 + tid] = s;
    }
}

}  // namespace fokl
